/* Compiled as C99 by tests/test_upsample_cpu.py: adanerf_temporal_upsample is declared by the plain-C header and exported by the shared
 * library, without a struct change.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*upsample)(adanerf_ctx*, int32_t, const float*, const float*, const float*, float, float, const float*, const float*, const float*, const float*,
                  const uint8_t*, const float*, const float*, float, float, float, int32_t, float*, float*, uint8_t*, void*, uint8_t*, int32_t*) =
      adanerf_temporal_upsample;
  const float pos[3] = {0.f, 0.f, 0.f}, rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  int32_t sizes[3] = {0, 0, 0}, rejected = -7;
  int rc = upsample(NULL, 2, NULL, NULL, NULL, 0.25f, -0.25f, pos, rot, NULL, NULL, NULL, pos, rot, 0.1f, 0.02f, 0.5f, ADANERF_TEMPORAL_CLAMP, NULL, NULL, NULL,
                    NULL, NULL, &rejected);
  printf("temporal_upsample(NULL) rc=%d rejected=%d abi=%d clamp=%d\n", rc, (int)rejected, adanerf_abi_version(), ADANERF_TEMPORAL_CLAMP);
  if (rc != ADANERF_EINVAL || rejected != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* one added entry point, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 3;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 4;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  return 0;
}
