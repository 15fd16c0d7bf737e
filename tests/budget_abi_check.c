/* Compiled as C99 by tests/test_budget_cpu.py: adanerf_set_budget_map, adanerf_foveate and adanerf_compact_budget are declared by the
 * plain-C header and exported by the shared library.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*set_map)(adanerf_ctx*, const uint8_t*, const float*) = adanerf_set_budget_map;
  int (*foveate)(adanerf_ctx*, float, float, int32_t, const int32_t*, const int32_t*, const float*, uint8_t*, float*) = adanerf_foveate;
  int (*compact)(adanerf_ctx*, const float*, int32_t, int32_t, float, const uint8_t*, const float*, int32_t*, int32_t*, uint32_t*, float*,
                 int32_t*) = adanerf_compact_budget;
  const int32_t radius[1] = {10}, n[2] = {8, 2};
  const float thr[2] = {0.2f, 0.4f};
  int rc[3];
  rc[0] = set_map(NULL, NULL, NULL);
  rc[1] = foveate(NULL, 1.0f, 2.0f, 1, radius, n, thr, NULL, NULL);
  rc[2] = compact(NULL, NULL, 0, 8, 0.2f, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
  printf("set_budget_map(NULL) rc=%d foveate(NULL) rc=%d compact_budget(NULL) rc=%d abi=%d\n", rc[0], rc[1], rc[2], adanerf_abi_version());
  if (rc[0] != ADANERF_EINVAL || rc[1] != ADANERF_EINVAL || rc[2] != ADANERF_EINVAL) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* added entry points, no struct change */
  return 0;
}
