/* Compiled as C99 by tests/test_contrast_cpu.py: adanerf_contrast_mask, adanerf_accumulate_masked, adanerf_resolve_mean_masked and
 * adanerf_host_contrast_mask are declared by the plain-C header and exported by the shared library.  No device is needed: a NULL context
 * is refused before anything touches one, and the host mask is host code. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*mask)(adanerf_ctx*, const float*, int32_t, int32_t, float, uint8_t*, int32_t*) = adanerf_contrast_mask;
  int (*acc)(adanerf_ctx*, const float*, const uint8_t*, uint32_t, int32_t, float*, int32_t) = adanerf_accumulate_masked;
  int (*res)(adanerf_ctx*, const float*, const uint8_t*, uint32_t, int32_t, int32_t, void*, float*) = adanerf_resolve_mean_masked;
  int (*host)(const float*, int32_t, int32_t, float, uint8_t*, int32_t*) = adanerf_host_contrast_mask;
  /* 4 x 1: a step of 0.5 between the second and the third pixel */
  const float rgb[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.5f, 0.f, 0.f, 0.5f, 0.f, 0.f};
  float sum[12] = {0};
  uint8_t m[4] = {9, 9, 9, 9};
  int32_t flagged = -7;
  int rc[4], k;
  rc[0] = mask(NULL, rgb, 4, 1, 0.25f, m, &flagged);
  rc[1] = acc(NULL, rgb, m, 1u, 4, sum, 1);
  rc[2] = res(NULL, sum, m, 1u, 4, 4, NULL, sum);
  printf("contrast_mask(NULL) rc=%d flagged=%d accumulate_masked(NULL) rc=%d resolve_mean_masked(NULL) rc=%d", rc[0], (int)flagged, rc[1], rc[2]);
  if (rc[0] != ADANERF_EINVAL || rc[1] != ADANERF_EINVAL || rc[2] != ADANERF_EINVAL || flagged != -7) return 1;
  for (k = 0; k < 4; ++k)
    if (m[k] != 9) return 1;
  rc[3] = host(rgb, 4, 1, 0.25f, m, &flagged);
  printf(" host_contrast_mask rc=%d flagged=%d abi=%d\n", rc[3], (int)flagged, adanerf_abi_version());
  for (k = 0; k < 4; ++k) printf("%d%s", (int)m[k], k == 3 ? "\n" : " ");
  if (rc[3] != ADANERF_OK || flagged != 2) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* added entry points, no struct change */
  return 0;
}
