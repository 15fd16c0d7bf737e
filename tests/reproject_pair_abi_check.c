/* Compiled as C99 by tests/test_reproject_pair_cpu.py: adanerf_reproject_pair and adanerf_host_pair_weight are declared by the plain-C
 * header and exported by the shared library.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*pair)(adanerf_ctx*, const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*, const float*,
              const float*, const float*, const float*, float, float, float, uint32_t, int32_t, float*, void*, float*, uint8_t*, uint8_t*, int32_t*) =
      adanerf_reproject_pair;
  int (*weight)(const float*, const float*, const float*, float*) = adanerf_host_pair_weight;
  const float pos[3] = {0.f, 0.f, 0.f}, one[3] = {1.f, 0.f, 0.f}, half[3] = {0.5f, 0.f, 0.f}, rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  int32_t sizes[3] = {0, 0, 0}, holes = -7;
  float w = -1.f;
  int rc = pair(NULL, NULL, NULL, NULL, pos, rot, NULL, NULL, NULL, one, rot, half, rot, 0.5f, 0.5f, 0.05f, 0u, ADANERF_REPROJECT_FILL, NULL, NULL, NULL, NULL, NULL,
                &holes);
  printf("reproject_pair(NULL) rc=%d holes=%d abi=%d fill=%d\n", rc, (int)holes, adanerf_abi_version(), ADANERF_REPROJECT_FILL);
  if (rc != ADANERF_EINVAL || holes != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* two added entry points, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 3;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 4;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  if (weight(half, pos, one, &w) != ADANERF_OK || w != 0.5f) return 5;
  if (weight(half, pos, one, NULL) != ADANERF_EINVAL) return 6;
  printf("pair_weight %g\n", (double)w);
  return 0;
}
