/* Compiled as C99 by tests/test_set_selection_cpu.py: adanerf_set_selection is declared by the plain-C header and exported by the
 * shared library.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*fn)(adanerf_ctx*, int32_t, float) = adanerf_set_selection;
  int rc = fn(NULL, 8, 0.2f);
  printf("set_selection(NULL) rc=%d abi=%d\n", rc, adanerf_abi_version());
  if (rc != ADANERF_EINVAL) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* an added entry point, no struct change */
  return 0;
}
