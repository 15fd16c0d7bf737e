// A4b: per-ray sample budgets (adanerf_set_budget_map / adanerf_foveate).  The selection rule keeps a prefix of one order -- values
// descending, lower bin first on ties -- so for n_r <= N and thr_r >= thr the selection at (n_r, thr_r) is a trim of the row the
// selection at (N, thr) already left in selbin / selw: the first n_r entries of that order whose value is >= thr_r, the first of the order
// if none is; a row of one entry stays.  trim_rows_kernel / trim_rows_wave_kernel run between the selection and expand_kernel: rows
// rewritten in place (compacted, bins still ascending), counts[r] replaced, and the segment totals expand_kernel reads recomputed from
// the new counts -- integer sums in a fixed order, no atomics: the same inputs give the same bytes.  foveate_kernel fills the two maps from a
// gaze point and concentric rings, in integers.  Every row is read once, only the rows that shrink are written; at N = 8 the thread-per-ray form
// is bound by its rank comparison (unrolled for 16 entries), not by bytes: 24 us for 640 000 rays, DESIGN 3.3.
// Device code only (gfx950, wave64); part of kernels.hip.hpp.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

constexpr int kTrimThreadMaxN = 16;      // rows up to this long live in one thread's registers (k_select_pair's kPairMaxN); longer: a wave per ray
constexpr int kFoveaMaxRings = 8;

// the per-ray budget: 0 or anything above the context's N is N, a threshold that is not above the context's (a NaN too) is the context's
__device__ __forceinline__ int budget_n(const uint8_t* __restrict__ n_map, int i, int n_max) {
  if (!n_map) return n_max;
  const int m = n_map[i];
  return (m == 0 || m > n_max) ? n_max : m;
}
__device__ __forceinline__ float budget_thr(const float* __restrict__ thr_map, int i, float thr) {
  if (!thr_map) return thr;
  const float t = thr_map[i];
  return t > thr ? t : thr;
}

// One thread per ray, n_max <= kTrimThreadMaxN; 2^seg_shift rays per entry of seg_total (32 after the pair / fused selection, 64 after
// select_kernel): a segment is half a wave or a wave, so its total is a DPP scan.  Rows of n_max % 4 == 0 entries are read as 16-byte /
// 4-byte words (the row stride is 4 n_max / n_max bytes: consecutive lanes then cover whole cache lines in n_max / 4 loads).  Entries at
// and beyond counts[r] are never looked at.  map_first: index of ray 0 of this batch in the two maps.
__global__ __launch_bounds__(256) void trim_rows_kernel(int32_t* __restrict__ counts, uint8_t* __restrict__ selbin, float* __restrict__ selw,
                                                        const uint8_t* __restrict__ n_map, const float* __restrict__ thr_map, int map_first,
                                                        int n_rays, int n_max, float thr, int seg_shift, int32_t* __restrict__ seg_total) {
  constexpr int M = kTrimThreadMaxN;
  const int r = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  const int c = r < n_rays ? min(counts[r], n_max) : 0;
  int kept = c;
  if (c > 1) {
    const int n_r = budget_n(n_map, map_first + r, n_max);
    const float thr_r = budget_thr(thr_map, map_first + r, thr);
    const size_t o = static_cast<size_t>(r) * n_max;
    float w[M];
    uint32_t b[M];
    if ((n_max & 3) == 0) {
#pragma unroll
      for (int q = 0; q < M / 4; ++q) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        uint32_t u = 0u;
        if (4 * q < c) {      // 4 q + 3 < n_max: inside the row
          v = *reinterpret_cast<const float4*>(selw + o + 4 * q);
          u = *reinterpret_cast<const uint32_t*>(selbin + o + 4 * q);
        }
        w[4 * q] = v.x;
        w[4 * q + 1] = v.y;
        w[4 * q + 2] = v.z;
        w[4 * q + 3] = v.w;
        b[4 * q] = u & 255u;
        b[4 * q + 1] = (u >> 8) & 255u;
        b[4 * q + 2] = (u >> 16) & 255u;
        b[4 * q + 3] = u >> 24;
      }
    } else {
#pragma unroll
      for (int k = 0; k < M; ++k) {
        w[k] = k < c ? selw[o + k] : 0.f;
        b[k] = k < c ? selbin[o + k] : 0u;
      }
    }
    // rank of entry k in the order (value descending, entry = bin ascending): the entries in front of it
    uint32_t keep = 0u, top = 0u;
#pragma unroll
    for (int k = 0; k < M; ++k) {
      int rank = 0;
#pragma unroll
      for (int j = 0; j < M; ++j) rank += (j < c && (w[j] > w[k] || (w[j] == w[k] && j < k))) ? 1 : 0;
      if (k < c) {
        if (rank == 0) top = 1u << k;
        if (rank < n_r && w[k] >= thr_r) keep |= 1u << k;
      }
    }
    if (!keep) keep = top;
    kept = __popc(keep);
    if (kept != c) {
      int pos = 0;      // pos <= k: an entry never overwrites one that is still to move (all of them are in registers anyway)
#pragma unroll
      for (int k = 0; k < M; ++k)
        if ((keep >> k) & 1u) {
          selw[o + pos] = w[k];
          selbin[o + pos] = static_cast<uint8_t>(b[k]);
          ++pos;
        }
      counts[r] = kept;
    }
  }
  const int x = seg_shift == 5 ? wave_incl_sum_dpp_i32<32>(kept) : wave_incl_sum_dpp_i32<64>(kept);
  const int last = (1 << seg_shift) - 1;
  if ((static_cast<int>(threadIdx.x) & last) == last && (r & ~last) < n_rays) seg_total[r >> seg_shift] = x;
}

// One wave per ray, any n_max <= 128 (lane: entries lane and lane + 64); a workgroup of 4 waves owns the 2^seg_shift rays behind one entry
// of seg_total, as select_kernel's does.  Ranks by a loop over the row with the value of entry j broadcast from its lane (v_readlane).
__global__ __launch_bounds__(256) void trim_rows_wave_kernel(int32_t* __restrict__ counts, uint8_t* __restrict__ selbin, float* __restrict__ selw,
                                                             const uint8_t* __restrict__ n_map, const float* __restrict__ thr_map, int map_first,
                                                             int n_rays, int n_max, float thr, int seg_shift, int32_t* __restrict__ seg_total) {
  __shared__ int wave_tot[4];
  const int lane = lane_id();
  const int wave = static_cast<int>(threadIdx.x) >> 6;
  const int rpw = (1 << seg_shift) >> 2;      // rays per wave
  const int base = (blockIdx.x << seg_shift) + wave * rpw;
  int total = 0;
  for (int i = 0; i < rpw; ++i) {
    const int r = base + i;
    if (r >= n_rays) break;      // wave-uniform
    const int c = min(__builtin_amdgcn_readfirstlane(counts[r]), min(n_max, 128));
    int kept = c;
    if (c > 1) {      // wave-uniform
      const int n_r = budget_n(n_map, map_first + r, n_max);
      const float thr_r = budget_thr(thr_map, map_first + r, thr);
      const size_t o = static_cast<size_t>(r) * n_max;
      const bool h0 = lane < c, h1 = lane + 64 < c;
      const float w0 = h0 ? selw[o + lane] : 0.f, w1 = h1 ? selw[o + 64 + lane] : 0.f;
      const uint8_t b0 = h0 ? selbin[o + lane] : 0, b1 = h1 ? selbin[o + 64 + lane] : 0;
      int rank0 = 0, rank1 = 0;
      for (int j = 0; j < c; ++j) {
        const int src = __builtin_bit_cast(int, j < 64 ? w0 : w1);
        const float wj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(src, j & 63));
        rank0 += (wj > w0 || (wj == w0 && j < lane)) ? 1 : 0;
        rank1 += (wj > w1 || (wj == w1 && j < lane + 64)) ? 1 : 0;
      }
      uint64_t m0 = __ballot(h0 && rank0 < n_r && w0 >= thr_r), m1 = __ballot(h1 && rank1 < n_r && w1 >= thr_r);
      if ((m0 | m1) == 0) {      // nothing reaches thr_r: the first of the order alone
        m0 = __ballot(h0 && rank0 == 0);
        m1 = m0 ? 0 : __ballot(h1 && rank1 == 0);
        m0 &= ~m0 + 1;
        m1 &= ~m1 + 1;
      }
      const int c0 = __popcll(m0);
      kept = c0 + __popcll(m1);
      if (kept != c) {      // every lane's entries are in registers by now (the ballots needed them)
        if ((m0 >> lane) & 1) {
          const int p = mbcnt64(m0);
          selw[o + p] = w0;
          selbin[o + p] = b0;
        }
        if ((m1 >> lane) & 1) {
          const int p = c0 + mbcnt64(m1);
          selw[o + p] = w1;
          selbin[o + p] = b1;
        }
        if (lane == 0) counts[r] = kept;
      }
    }
    total += kept;
  }
  if (lane == 0) wave_tot[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) seg_total[blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
}

// Foveation: pixel (x, y) of local ray i (the ray generator's strip mapping, ray_pixel) against a gaze point and concentric rings, all in
// integers at half-pixel resolution: q = (2 x + 1 - gx2)^2 + (2 y + 1 - gy2)^2 is four times the squared distance of the pixel centre
// from the gaze; ring k contains the pixel iff q <= r2x4[k] = (2 radius_k)^2.  The pixel gets entry k of the first ring that contains it,
// the entry behind the last ring outside them all.  The host fills the slots behind the rings in use: r2x4 = 2^64 - 1 and the outside
// entry, so the kernel walks all kFoveaMaxRings with constant indices.  |gx2|, |gy2| <= 2^31 and x, y < 2^25: q < 2^64.
struct FoveaParams {
  int64_t gx2, gy2;
  uint64_t r2x4[kFoveaMaxRings];
  float thr[kFoveaMaxRings + 1];
  uint8_t n[kFoveaMaxRings + 1];
};

__global__ __launch_bounds__(256) void foveate_kernel(RayGenParams g, FoveaParams f, int n_rays, uint8_t* __restrict__ n_map,
                                                      float* __restrict__ thr_map) {
  const int i = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  if (i >= n_rays) return;
  int x, y;
  ray_pixel(g, i, &x, &y);
  const int64_t dx = 2 * static_cast<int64_t>(x) + 1 - f.gx2, dy = 2 * static_cast<int64_t>(y) + 1 - f.gy2;
  const uint64_t q = static_cast<uint64_t>(dx * dx) + static_cast<uint64_t>(dy * dy);
  uint8_t nv = f.n[0];
  float tv = f.thr[0];
#pragma unroll
  for (int j = 0; j < kFoveaMaxRings; ++j)      // radii ascend: the rings that do not contain the pixel come first
    if (q > f.r2x4[j]) {
      nv = f.n[j + 1];
      tv = f.thr[j + 1];
    }
  if (n_map) n_map[i] = nv;
  if (thr_map) thr_map[i] = tv;
}

}  // namespace adanerf
