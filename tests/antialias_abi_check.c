/* Compiled as C99 by tests/test_antialias_cpu.py: the anti-aliasing entry points and ADANERF_PRESENT_AREA are declared by the plain-C
 * header and exported by the shared library, without a struct change.  No device is needed: a NULL context is refused before anything
 * touches one, and adanerf_host_subpixel_grid is host-only. */
#include <stdio.h>

#include "../include/adanerf_hip.h"

int main(void) {
  int (*set_offset)(adanerf_ctx*, float, float) = adanerf_set_pixel_offset;
  int (*get_offset)(const adanerf_ctx*, float*) = adanerf_get_pixel_offset;
  int (*accumulate)(adanerf_ctx*, const float*, int32_t, float*, int32_t) = adanerf_accumulate;
  int (*resolve)(adanerf_ctx*, const float*, int32_t, int32_t, void*, float*) = adanerf_resolve_mean;
  int (*grid)(int32_t, int32_t, float*, float*) = adanerf_host_subpixel_grid;
  float out[2] = {-7.f, -7.f}, dx = -7.f, dy = -7.f, img[3] = {1.f, 2.f, 3.f}, sum[3] = {0.f, 0.f, 0.f};
  int32_t sizes[3] = {0, 0, 0};
  const int rc[5] = {set_offset(NULL, 0.25f, -0.25f), get_offset(NULL, out), accumulate(NULL, img, 1, sum, 1), resolve(NULL, sum, 1, 1, NULL, sum),
                     adanerf_present(NULL, img, 1, 1, sum, 1, 1, ADANERF_PRESENT_AREA)};
  printf("null rc=%d %d %d %d %d out=%g sum=%g abi=%d area=%d\n", rc[0], rc[1], rc[2], rc[3], rc[4], (double)out[0], (double)sum[0], adanerf_abi_version(),
         ADANERF_PRESENT_AREA);
  for (int k = 0; k < 5; ++k)
    if (rc[k] != ADANERF_EINVAL) return 1;
  if (out[0] != -7.f || sum[0] != 0.f) return 2;
  if (adanerf_abi_version() != 4 || ADANERF_ABI_VERSION != 4 || ADANERF_PRESENT_AREA != 8) return 3;   /* entry points and one flag added, no struct change */
  if (ADANERF_PRESENT_FLIP_Y != 1 || ADANERF_PRESENT_NEAREST != 2 || ADANERF_PRESENT_LINEAR != 4) return 4;
  if (adanerf_struct_sizes(sizes) != ADANERF_OK) return 5;
  if (sizes[0] != (int32_t)sizeof(adanerf_options) || sizes[1] != (int32_t)sizeof(adanerf_info) || sizes[2] != (int32_t)sizeof(adanerf_stats)) return 6;
  printf("sizes %d %d %d\n", (int)sizes[0], (int)sizes[1], (int)sizes[2]);
  if (grid(2, 3, &dx, &dy) != ADANERF_OK || dx != 0.25f || dy != 0.25f) return 7;
  if (grid(0, 0, &dx, &dy) != ADANERF_EINVAL || grid(9, 0, &dx, &dy) != ADANERF_EINVAL || grid(2, 4, &dx, &dy) != ADANERF_EINVAL ||
      grid(2, 0, NULL, &dy) != ADANERF_EINVAL || dx != 0.25f)
    return 8;
  printf("grid(2,3) %g %g\n", (double)dx, (double)dy);
  return 0;
}
