// N11: adaptive supersampling -- which pixels of a rendered frame sit on an edge (adanerf_contrast_mask).  The rule is contrast_rule.hpp,
// shared with the host mirror: a pixel is flagged (byte 0) iff the display values of one of its up to 8 neighbours differ from its own by
// more than the threshold in some channel.  A 3 x 3 stencil over an interleaved [h, w, 3] fp32 image: 12 bytes read, 1 byte written per pixel.
//   contrast_mask_kernel   64 x 16 pixel tiles, 256 threads.  The tile and its one-pixel halo are staged in LDS as CLAMPED values, one plane
//                          per channel: consecutive threads read consecutive floats of a staged row (198 contiguous floats of the image per
//                          row), so a value comes from global memory once per block plus the halo (1.16 x the image) and is clamped once.
//                          Then a wave works on one row of 64 pixels at a time, consecutive lanes on consecutive pixels: every stencil read
//                          is 64 consecutive floats of one plane, free of bank conflicts at any pitch.  The staging writes scatter a run of
//                          floats over the three planes; the plane stride is 11 mod 32, so the ~11 pixels x 3 channels that 32 lanes hold
//                          land on distinct banks.  The halo outside the image is never read (the rule tests the bounds), so it is
//                          not staged.
//                          The flags of a row segment are gathered with one __ballot; lane k then packs the bytes of pixels 4 k .. 4 k + 3
//                          behind the first 4-byte aligned address of the segment into one word (a wave writes its 64 bytes as 16 words,
//                          not 64 bytes), and the up to 3 + 3 bytes in front of it and at the ragged end go out as single bytes -- for any
//                          alignment of the mask and any width.  The flagged pixels are counted with one atomicAdd per wave and row that
//                          has any.
// Each difference is one rounded fp32 subtraction (-ffp-contract=off; nothing to fuse), so the kernel is exact against a numpy float32
// restatement (tests/contrast_reference.py).
#pragma once
#include "k_common.hip.hpp"
#include "contrast_rule.hpp"

namespace adanerf {

constexpr int kContrastTileW = 64, kContrastTileH = 16;                     // 256 threads: a wave is one row of 64 pixels, four rows per wave
constexpr int kContrastPitch = kContrastTileW + 2;                          // a staged row of one plane: the tile and its halo
constexpr int kContrastRows = kContrastTileH + 2;
constexpr int kContrastRowFloats = kContrastPitch * 3;                      // the same row in the image: 198 contiguous floats
constexpr int kContrastPlane = kContrastRows * kContrastPitch + (32 + 11 - (kContrastRows * kContrastPitch) % 32) % 32;      // 11 mod 32
static_assert(kContrastPlane % 32 == 11 && kContrastTileW == 64 && kContrastTileH % 4 == 0, "one wave per row of the tile; the planes 11 banks apart");

__global__ __launch_bounds__(256) void contrast_mask_kernel(const float* __restrict__ rgb, int w, int h, float threshold, uint8_t* __restrict__ mask,
                                                            int32_t* __restrict__ n_flagged) {
  __shared__ float tile[3 * kContrastPlane];
  const int tid = static_cast<int>(threadIdx.x);
  const int x_first = static_cast<int>(blockIdx.x) * kContrastTileW, y_first = static_cast<int>(blockIdx.y) * kContrastTileH;

  for (int i = tid; i < kContrastRows * kContrastRowFloats; i += 256) {
    const int r = i / kContrastRowFloats, c = i - r * kContrastRowFloats;
    const int col = c / 3, ch = c - 3 * col;
    const int px = x_first - 1 + col, py = y_first - 1 + r;
    if (px >= 0 && px < w && py >= 0 && py < h)      // w * h <= 2^28 (sides <= 16384): 3 w h fits 32 bits unsigned, the offset is formed in 64
      tile[ch * kContrastPlane + r * kContrastPitch + col] = contrast_display(rgb[(static_cast<size_t>(py) * w + px) * 3 + ch]);
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  const int x = x_first + lane;
  const int nv = w - x_first < kContrastTileW ? w - x_first : kContrastTileW;      // the pixels of this block's row segments: 1..64
  const auto plane = [&](int ch) {
    return [=](int qx, int qy) { return tile[ch * kContrastPlane + (qy - y_first + 1) * kContrastPitch + (qx - x_first + 1)]; };
  };
  for (int k = 0; k < kContrastTileH / 4; ++k) {
    const int y = y_first + wave * (kContrastTileH / 4) + k;
    if (y >= h) break;      // uniform over the wave
    const bool flagged = lane < nv && contrast_mask_byte(x, y, w, h, threshold, plane(0), plane(1), plane(2)) == 0;
    const uint64_t flags = __ballot(flagged);
    uint8_t* const row = mask + static_cast<size_t>(y) * w + x_first;
    int head = static_cast<int>((4 - (reinterpret_cast<uintptr_t>(row) & 3)) & 3);      // single bytes up to the first aligned address
    if (head > nv) head = nv;
    const int n_words = (nv - head) >> 2, tail = head + 4 * n_words;
    if (lane < n_words) {
      const uint32_t bits = static_cast<uint32_t>(flags >> (head + 4 * lane)) & 15u;
      const uint32_t set = (bits & 1u) | ((bits & 2u) << 7) | ((bits & 4u) << 14) | ((bits & 8u) << 21);      // bit j -> byte j
      *reinterpret_cast<uint32_t*>(row + head + 4 * lane) = 0x01010101u ^ set;
    }
    if (lane < head || (lane >= tail && lane < nv)) row[lane] = flagged ? 0 : 1;
    if (n_flagged && flags && lane == __ffsll(static_cast<unsigned long long>(flags)) - 1) atomicAdd(n_flagged, __popcll(flags));
  }
}

}  // namespace adanerf
