/* Compiled as C99 by tests/test_sparse_temporal_cpu.py: the phased density entry points, the phase cycle and
 * adanerf_temporal_resolve_sparse are declared by the plain-C header and exported by the shared library.  No device is needed: a NULL
 * context is refused before anything touches one, and the host mask and the cycle are host code. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*mask)(adanerf_ctx*, float, float, int32_t, const int32_t*, const int32_t*, int32_t, int32_t, uint8_t*) = adanerf_foveate_density_phased;
  int (*fill)(adanerf_ctx*, const uint8_t*, int32_t, int32_t, int32_t, int32_t, float*, float*, float*, void*, int32_t*) = adanerf_fill_density_phased;
  int (*host)(int32_t, int32_t, float, float, int32_t, const int32_t*, const int32_t*, int32_t, int32_t, uint8_t*) = adanerf_host_density_mask_phased;
  int (*cycle)(int32_t, int32_t*, int32_t*) = adanerf_host_density_phase;
  int (*resolve)(adanerf_ctx*, const uint8_t*, int32_t, int32_t, const float*, const float*, const float*, const float*, const float*, const float*,
                 const float*, const uint8_t*, const float*, const float*, float, float, float, int32_t, float*, float*, uint8_t*, void*, uint8_t*,
                 int32_t*) = adanerf_temporal_resolve_sparse;
  const int32_t radius[1] = {1}, stride[2] = {1, 2};
  const float pos[3] = {0.f, 0.f, 0.f}, rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  uint8_t m[12];
  float img[36];
  int32_t unfilled = -7, rejected = -7, px = -7, py = -7;
  int rc[5], k;
  rc[0] = mask(NULL, 0.f, 0.f, 1, radius, stride, 1, 1, m);
  rc[1] = fill(NULL, m, 4, 3, 1, 1, NULL, NULL, NULL, NULL, &unfilled);
  rc[2] = host(4, 3, 1.5f, 1.5f, 1, radius, stride, 1, 1, m);
  rc[3] = cycle(27, &px, &py);
  rc[4] = resolve(NULL, m, 1, 1, img, img, img, pos, rot, NULL, NULL, NULL, NULL, NULL, 0.1f, 0.02f, 0.5f, 0, img, NULL, m, NULL, NULL, &rejected);
  printf("foveate_density_phased(NULL) rc=%d fill_density_phased(NULL) rc=%d unfilled=%d host_density_mask_phased rc=%d "
         "host_density_phase(27) rc=%d %d %d temporal_resolve_sparse(NULL) rc=%d rejected=%d abi=%d\n",
         rc[0], rc[1], (int)unfilled, rc[2], rc[3], (int)px, (int)py, rc[4], (int)rejected, adanerf_abi_version());
  for (k = 0; k < 12; ++k) printf("%d%s", (int)m[k], k == 11 ? "\n" : " ");
  if (rc[0] != ADANERF_EINVAL || rc[1] != ADANERF_EINVAL || rc[2] != ADANERF_OK || rc[3] != ADANERF_OK || rc[4] != ADANERF_EINVAL) return 1;
  if (unfilled != -7 || rejected != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* added entry points, no struct change */
  return 0;
}
