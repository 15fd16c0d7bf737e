/* Compiled as C99 by tests/test_set_frame_size_cpu.py: adanerf_set_frame_size and adanerf_present are declared by the plain-C header and
 * exported by the shared library.  No device is needed: a NULL context is refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*resize)(adanerf_ctx*, int32_t, int32_t) = adanerf_set_frame_size;
  int (*present)(adanerf_ctx*, const void*, int32_t, int32_t, void*, int32_t, int32_t, int32_t) = adanerf_present;
  int32_t sizes[3] = {0, 0, 0};
  int rc0 = resize(NULL, 64, 48);
  int rc1 = present(NULL, NULL, 1, 1, NULL, 1, 1, ADANERF_PRESENT_FLIP_Y | ADANERF_PRESENT_LINEAR);
  printf("set_frame_size(NULL) rc=%d present(NULL) rc=%d abi=%d flags=%d,%d,%d\n", rc0, rc1, adanerf_abi_version(), ADANERF_PRESENT_FLIP_Y,
         ADANERF_PRESENT_NEAREST, ADANERF_PRESENT_LINEAR);
  if (rc0 != ADANERF_EINVAL || rc1 != ADANERF_EINVAL) return 1;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 2;   /* two added entry points, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 3;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 4;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  return 0;
}
