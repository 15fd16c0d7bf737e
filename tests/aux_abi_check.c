/* Compiled as C99 by tests/test_host_cpu.py: adanerf_composite_aux, adanerf_composite_classic_aux and adanerf_disp_map are declared by the
 * plain-C header with the signatures a binding expects and exported by the shared library.  No device is needed: a NULL context is
 * refused before anything touches one. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*composite_aux)(adanerf_ctx*, const float*, const float*, const int32_t*, const int32_t*, const uint32_t*, int32_t, float*, void*, float*,
                       float*) = adanerf_composite_aux;
  int (*classic_aux)(adanerf_ctx*, const float*, const float*, const float*, int32_t, int32_t, float*, void*, float*, float*) =
      adanerf_composite_classic_aux;
  int (*disp_map)(adanerf_ctx*, const float*, const float*, int32_t, float*) = adanerf_disp_map;
  /* the entries they extend keep their signatures */
  int (*composite)(adanerf_ctx*, const float*, const float*, const int32_t*, const int32_t*, int32_t, float*, void*) = adanerf_composite;
  int (*classic)(adanerf_ctx*, const float*, const float*, const float*, int32_t, int32_t, float*, void*) = adanerf_composite_classic;
  int32_t sizes[3] = {0, 0, 0};
  float depth = -7.f, acc = -7.f, disp = -7.f;
  int rc0 = composite_aux(NULL, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL, &depth, &acc);
  int rc1 = classic_aux(NULL, NULL, NULL, NULL, 1, 1, NULL, NULL, &depth, &acc);
  int rc2 = disp_map(NULL, &depth, &acc, 1, &disp);
  printf("aux(NULL) rc=%d %d %d maps=%g %g %g abi=%d\n", rc0, rc1, rc2, depth, acc, disp, adanerf_abi_version());
  if (rc0 != ADANERF_EINVAL || rc1 != ADANERF_EINVAL || rc2 != ADANERF_EINVAL) return 1;
  if (depth != -7.f || acc != -7.f || disp != -7.f) return 2;
  if (composite(NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL) != ADANERF_EINVAL || classic(NULL, NULL, NULL, NULL, 0, 1, NULL, NULL) != ADANERF_EINVAL) return 3;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4) return 4;   /* three added entry points, no struct change */
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 5;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 6;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  return 0;
}
