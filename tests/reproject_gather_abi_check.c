/* Compiled as C99 by tests/test_reproject_gather_cpu.py: adanerf_reproject_gather and its flag are declared by the plain-C header and
 * exported by the shared library.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*gather)(adanerf_ctx*, const float*, const float*, const float*, const float*, const float*, const float*, const float*, float, float, int32_t,
                uint32_t, int32_t, float*, void*, float*, uint8_t*, int32_t*) = adanerf_reproject_gather;
  const float pos[3] = {0.f, 0.f, 0.f}, rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  int32_t sizes[3] = {0, 0, 0}, holes = -7;
  int rc = gather(NULL, NULL, NULL, NULL, pos, rot, pos, rot, 0.5f, 0.05f, 3, 0u, ADANERF_GATHER_GUESS, NULL, NULL, NULL, NULL, &holes);
  printf("reproject_gather(NULL) rc=%d holes=%d abi=%d guess=%d\n", rc, (int)holes, adanerf_abi_version(), ADANERF_GATHER_GUESS);
  if (rc != ADANERF_EINVAL || holes != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* one added entry point, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 3;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 4;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  return 0;
}
