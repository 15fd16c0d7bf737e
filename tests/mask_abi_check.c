/* Compiled as C99 by tests/test_render_masked_cpu.py: adanerf_render_masked and the two buffer constants of its ray list are declared by the
 * plain-C header and the entry point is exported by the shared library, without a struct change.  No device is needed: a NULL context is
 * refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*masked)(adanerf_ctx*, const uint8_t*, uint32_t, void*, float*, adanerf_stats*, int32_t*) = adanerf_render_masked;
  int32_t sizes[3] = {0, 0, 0}, rendered = -7;
  int rc = masked(NULL, NULL, 1u, NULL, NULL, NULL, &rendered);
  printf("render_masked(NULL) rc=%d rendered=%d abi=%d list=%d count=%d\n", rc, (int)rendered, adanerf_abi_version(), (int)ADANERF_BUF_RAY_LIST,
         (int)ADANERF_BUF_RAY_LIST_COUNT);
  if (rc != ADANERF_EINVAL || rendered != -7) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* one added entry point, two constants, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 3;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 4;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  return 0;
}
