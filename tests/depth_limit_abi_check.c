/* Compiled as C99 by tests/test_depth_limit_cpu.py: adanerf_set_depth_limit, adanerf_compact_depth_limit, adanerf_blend_behind and
 * adanerf_host_sphere_zc are declared by the plain-C header and exported by the shared library.  No device is needed: a NULL context is
 * refused before anything touches one, and the sphere is host code. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*set_limit)(adanerf_ctx*, const float*) = adanerf_set_depth_limit;
  int (*compact)(adanerf_ctx*, const float*, int32_t, int32_t, float, const float*, const float*, const float[3], const float[9], int32_t*, int32_t*,
                 uint32_t*, float*, int32_t*) = adanerf_compact_depth_limit;
  int (*blend)(adanerf_ctx*, const float*, const float*, const float*, int32_t, float*, void*) = adanerf_blend_behind;
  int (*sphere)(int32_t, int32_t, float, const float[3], const float[9], const float[3], float, float*) = adanerf_host_sphere_zc;
  const float pos[3] = {0.f, 0.f, 0.f}, rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, center[3] = {0.f, 0.f, -3.f};
  float zc = 0.f;
  int rc[4];
  rc[0] = set_limit(NULL, NULL);
  rc[1] = compact(NULL, NULL, 0, 8, 0.2f, NULL, NULL, pos, rot, NULL, NULL, NULL, NULL, NULL);
  rc[2] = blend(NULL, NULL, NULL, NULL, 0, NULL, NULL);
  rc[3] = sphere(1, 1, 10.f, pos, rot, center, 1.f, &zc);
  printf("set_depth_limit(NULL) rc=%d compact_depth_limit(NULL) rc=%d blend_behind(NULL) rc=%d sphere_zc rc=%d zc=%g abi=%d\n", rc[0], rc[1], rc[2], rc[3],
         (double)zc, adanerf_abi_version());
  if (rc[0] != ADANERF_EINVAL || rc[1] != ADANERF_EINVAL || rc[2] != ADANERF_EINVAL || rc[3] != ADANERF_OK) return 1;
  if (zc != 2.f) return 3;                                                /* straight ahead, centre at 3, radius 1 */
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* added entry points, no struct change */
  return 0;
}
