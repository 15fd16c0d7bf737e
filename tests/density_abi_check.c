/* Compiled as C99 by tests/test_density_cpu.py: adanerf_foveate_density, adanerf_fill_density and adanerf_host_density_mask are declared by
 * the plain-C header and exported by the shared library.  No device is needed: a NULL context is refused before anything touches one, and
 * the host mask is host code. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*mask)(adanerf_ctx*, float, float, int32_t, const int32_t*, const int32_t*, uint8_t*) = adanerf_foveate_density;
  int (*fill)(adanerf_ctx*, const uint8_t*, int32_t, int32_t, float*, float*, float*, void*, int32_t*) = adanerf_fill_density;
  int (*host)(int32_t, int32_t, float, float, int32_t, const int32_t*, const int32_t*, uint8_t*) = adanerf_host_density_mask;
  const int32_t radius[1] = {1}, stride[2] = {1, 2};
  uint8_t m[12];
  int32_t unfilled = -7;
  int rc[3], k;
  rc[0] = mask(NULL, 0.f, 0.f, 1, radius, stride, m);
  rc[1] = fill(NULL, m, 4, 3, NULL, NULL, NULL, NULL, &unfilled);
  rc[2] = host(4, 3, 1.5f, 1.5f, 1, radius, stride, m);
  printf("foveate_density(NULL) rc=%d fill_density(NULL) rc=%d unfilled=%d host_density_mask rc=%d abi=%d\n", rc[0], rc[1], (int)unfilled, rc[2],
         adanerf_abi_version());
  for (k = 0; k < 12; ++k) printf("%d%s", (int)m[k], k == 11 ? "\n" : " ");
  if (rc[0] != ADANERF_EINVAL || rc[1] != ADANERF_EINVAL || rc[2] != ADANERF_OK || unfilled != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* added entry points, no struct change */
  return 0;
}
