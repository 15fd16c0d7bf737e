/* Compiled as C99 by tests/test_reproject_cpu.py: adanerf_reproject and its flag are declared by the plain-C header and exported by the
 * shared library.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*reproject)(adanerf_ctx*, const void*, const float*, const float*, const float*, const float*, const float*, const float*, float, uint32_t,
                   int32_t, void*, float*, uint8_t*, int32_t*) = adanerf_reproject;
  const float pos[3] = {0.f, 0.f, 0.f}, rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  int32_t sizes[3] = {0, 0, 0}, holes = -7;
  int rc = reproject(NULL, NULL, NULL, NULL, pos, rot, pos, rot, 0.5f, 0u, ADANERF_REPROJECT_FILL, NULL, NULL, NULL, &holes);
  printf("reproject(NULL) rc=%d holes=%d abi=%d fill=%d\n", rc, (int)holes, adanerf_abi_version(), ADANERF_REPROJECT_FILL);
  if (rc != ADANERF_EINVAL || holes != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* one added entry point, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 3;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 4;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  return 0;
}
