// A4d: a hard upper bound on the samples a batch may shade (adanerf_set_sample_cap).  The third user of the seam between the selection and
// expand_kernel, after the budget trim (k_budget.hip.hpp) and the depth limit (k_depth_limit.hip.hpp): the threshold is raised by exactly as
// much as the bound needs, on the device, in the same frame, with no read-back.
// Rule, in integers on the values' bits: row r has c_r entries v_rk in selw; kept_r(t) = 0 if c_r == 0, else max(1, #{k < c_r : v_rk >= t})
// (an fp32 >=: a NaN never passes, -0 equals +0); T(t) = sum_r kept_r(t), T_now = sum_r c_r.  T_now <= C: nothing is written.  Otherwise t* is the
// smallest non-NaN value present in the rows with T(t*) <= C (+inf if none has), and every row is trimmed at (N, t*) by the unchanged
// trim_rows_kernel / trim_rows_wave_kernel: cap_fill_kernel writes t* into a context-owned threshold map and launch_trim follows.
// Mechanism: key(v) is the order-preserving u32 of the value's bits (-0 taken as +0; NaN has none), so v >= t iff key(v) >= key(t), and
//   T(t) = A(t) + nonempty - M(t),   A(t) = non-NaN entries >= t,   M(t) = non-empty rows whose largest non-NaN value is >= t.
// T never grows with t and changes only at present values, so t* is the present value that follows p, the largest present key with
// T(p) > C: an exact radix selection of p over the 32-bit keys in three levels of 11 + 11 + 10 bits.  Per level cap_hist_kernel builds two integer
// histograms (entries, row maxima) of the keys inside the bucket chosen so far, privatised in LDS and flushed with integer atomicAdd (sums of integers
// do not depend on their order: the same inputs give the same bits; no floating-point atomic anywhere), and cap_search_kernel, one workgroup,
// takes suffix sums and picks the digit.  The last level also takes the smallest key above the final bucket (an integer atomicMax of ~key), where
// p's successor lies when its own bucket holds none.  No workgroup waits on another: every pass is a launch, ordered by the stream.
// If the non-NaN entries alone already fit (T_now exceeds C only by NaN entries of multi-entry rows, which no selection writes), t* is the
// smallest present value: the search then walks to the lowest occupied bucket of every level.
// Device code only (gfx950, wave64); part of kernels.hip.hpp.
#pragma once
#include "k_common.hip.hpp"

namespace adanerf {

constexpr int kCapBins = 2048;           // bins of one histogram: 11 bits (the last level uses the lower 1024)
constexpr int kCapLevels = 3;            // 11 + 11 + 10 bits
constexpr int kCapThreadMaxN = 16;       // rows up to this long are walked by one thread (kTrimThreadMaxN); longer: a wave per ray

// Per batch, zeroed together with the kCapLevels x 2 x kCapBins uint32 histogram words behind it before the first pass.
struct CapState {
  uint32_t t_now, nonempty;              // sum of the counts, rows with c_r > 0 (level 0)
  uint32_t active;                       // T_now > C and t* not found yet: the later passes have work
  uint32_t minmode;                      // the non-NaN entries fit: t* is the smallest present key
  uint32_t prefix;                       // key bits chosen so far
  uint32_t above_e, above_m;             // entries / row maxima in the buckets above the chosen one
  uint32_t succ_inv;                     // ~(smallest key above the final 10-bit bucket), 0: none (level 2)
  uint32_t pad[8];
};
static_assert(sizeof(CapState) == 64, "CapState is 16 words");

// Context-owned, read back only by adanerf_sample_cap_report: the batch's outcome and the running figures of the frame.
struct CapRecord {
  float tstar;                           // t* of the last batch, -inf if nothing was trimmed
  int32_t t_now, t_new;                  // its samples before and after
  int32_t trimmed;
  float thr_max;                         // the frame: largest t*, -inf if no batch was trimmed
  int32_t batches_trimmed;
  int64_t selected, kept;
};
static_assert(sizeof(CapRecord) == 40, "CapRecord is mirrored by the host");

// order-preserving key of a value; 0: a NaN (every other key is >= 0x007FFFFF, the key of -inf)
__device__ __forceinline__ uint32_t cap_key(float v) {
  uint32_t u = __builtin_bit_cast(uint32_t, v);
  if ((u << 1) == 0u) u = 0u;                                   // -0 is +0
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cap_value(uint32_t key) {
  return __builtin_bit_cast(float, (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ uint32_t cap_wave_max_u32(uint32_t v) {      // every lane gets it
  int x = static_cast<int>(v);
#define ADN_CAP_MAX(ctrl)                                                             \
  {                                                                                   \
    const uint32_t y = static_cast<uint32_t>(dpp_i32<ctrl>(x, x));                    \
    x = static_cast<int>(max(static_cast<uint32_t>(x), y));                           \
  }
  ADN_CAP_MAX(0xB1)
  ADN_CAP_MAX(0x4E)
  ADN_CAP_MAX(0x141)
  ADN_CAP_MAX(0x140)
#undef ADN_CAP_MAX
  const uint32_t r0 = __builtin_amdgcn_readlane(x, 0), r1 = __builtin_amdgcn_readlane(x, 16);
  const uint32_t r2 = __builtin_amdgcn_readlane(x, 32), r3 = __builtin_amdgcn_readlane(x, 48);
  return max(max(r0, r1), max(r2, r3));
}

__device__ __forceinline__ int cap_shift(int level) { return level == 0 ? 21 : (level == 1 ? 10 : 0); }

// One level's two histograms of the keys inside the bucket st->prefix names (level 0: all keys).  hist: [2][kCapBins] words of this level, zero
// on entry.  WAVE: a wave per ray (lane: entries lane and lane + 64), else a thread per ray; both walk the rays with the grid's stride.
// Entries at and beyond counts[r] are never looked at.
template <bool WAVE>
__global__ __launch_bounds__(256) void cap_hist_kernel(const int32_t* __restrict__ counts, const float* __restrict__ selw, int n_rays, int n_max,
                                                       int level, CapState* __restrict__ st, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[2 * kCapBins];
  __shared__ uint32_t s_succ, s_tn, s_ne;
  if (level > 0 && st->active == 0u) return;      // uniform: nothing to trim, nothing is written
  const int t = static_cast<int>(threadIdx.x);
  for (int i = t; i < 2 * kCapBins; i += 256) h[i] = 0u;
  if (t == 0) s_succ = s_tn = s_ne = 0u;
  __syncthreads();
  const int shift = cap_shift(level);
  const int mshift = level == 1 ? 21 : 10;      // the bits above this level's digit
  const uint32_t mask = level == 2 ? 1023u : 2047u;
  const uint32_t want = level == 0 ? 0u : st->prefix >> mshift;
  uint32_t tn = 0u, ne = 0u, succ = 0u;
  if (!WAVE) {
    constexpr int M = kCapThreadMaxN;
    for (int r = blockIdx.x * 256 + t; r < n_rays; r += static_cast<int>(gridDim.x) * 256) {
      const int c = min(counts[r], min(n_max, M));
      if (c <= 0) continue;
      tn += static_cast<uint32_t>(c);
      ne += 1u;
      const float* row = selw + static_cast<size_t>(r) * n_max;
      // the whole row first, as trim_rows_kernel reads it (16-byte words where the stride allows): the loads are in flight together
      float w[M];
      if ((n_max & 3) == 0) {
#pragma unroll
        for (int q = 0; q < M / 4; ++q) {
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (4 * q < c) v = *reinterpret_cast<const float4*>(row + 4 * q);      // 4 q + 3 < n_max: inside the row
          w[4 * q] = v.x;
          w[4 * q + 1] = v.y;
          w[4 * q + 2] = v.z;
          w[4 * q + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < M; ++k) w[k] = k < c ? row[k] : 0.f;
      }
      uint32_t rmax = 0u, run_d = 0u, run_n = 0u;      // equal digits in a row of one ray go out as one add
#pragma unroll
      for (int k = 0; k < M; ++k) {
        if (k >= c) continue;
        const uint32_t key = cap_key(w[k]);
        if (key == 0u) continue;
        rmax = max(rmax, key);
        if (level == 2 && (key >> 10) > want) succ = max(succ, ~key);
        if (level != 0 && (key >> mshift) != want) continue;
        const uint32_t d = (key >> shift) & mask;
        if (run_n != 0u && d != run_d) {
          atomicAdd(&h[run_d], run_n);
          run_n = 0u;
        }
        run_d = d;
        ++run_n;
      }
      if (run_n != 0u) atomicAdd(&h[run_d], run_n);
      if (rmax != 0u && (level == 0 || (rmax >> mshift) == want)) atomicAdd(&h[kCapBins + ((rmax >> shift) & mask)], 1u);
    }
  } else {
    const int lane = lane_id();
    for (int r = blockIdx.x * 4 + (t >> 6); r < n_rays; r += static_cast<int>(gridDim.x) * 4) {      // wave-uniform
      const int c = min(__builtin_amdgcn_readfirstlane(counts[r]), min(n_max, 128));
      if (c <= 0) continue;
      if (lane == 0) {
        tn += static_cast<uint32_t>(c);
        ne += 1u;
      }
      const float* row = selw + static_cast<size_t>(r) * n_max;
      const uint32_t k0 = lane < c ? cap_key(row[lane]) : 0u, k1 = lane + 64 < c ? cap_key(row[64 + lane]) : 0u;
      const uint32_t rmax = cap_wave_max_u32(max(k0, k1));
      if (level == 2) {
        if (k0 != 0u && (k0 >> 10) > want) succ = max(succ, ~k0);
        if (k1 != 0u && (k1 >> 10) > want) succ = max(succ, ~k1);
      }
      if (k0 != 0u && (level == 0 || (k0 >> mshift) == want)) atomicAdd(&h[(k0 >> shift) & mask], 1u);
      if (k1 != 0u && (level == 0 || (k1 >> mshift) == want)) atomicAdd(&h[(k1 >> shift) & mask], 1u);
      if (lane == 0 && rmax != 0u && (level == 0 || (rmax >> mshift) == want)) atomicAdd(&h[kCapBins + ((rmax >> shift) & mask)], 1u);
    }
  }
  // one global atomic per workgroup and counter: every workgroup adds to the same two words
  if (level == 0) {
    tn = static_cast<uint32_t>(wave_sum_dpp_i32(static_cast<int>(tn)));
    ne = static_cast<uint32_t>(wave_sum_dpp_i32(static_cast<int>(ne)));
    if ((t & 63) == 0 && ne != 0u) {
      atomicAdd(&s_tn, tn);
      atomicAdd(&s_ne, ne);
    }
  }
  if (level == 2) {
    succ = cap_wave_max_u32(succ);
    if ((t & 63) == 0 && succ != 0u) atomicMax(&s_succ, succ);
  }
  __syncthreads();
  for (int i = t; i < 2 * kCapBins; i += 256) {
    const uint32_t v = h[i];
    if (v != 0u) atomicAdd(&hist[i], v);
  }
  if (level == 0 && t == 0 && s_ne != 0u) {
    atomicAdd(&st->t_now, s_tn);
    atomicAdd(&st->nonempty, s_ne);
  }
  if (level == 2 && t == 0 && s_succ != 0u) atomicMax(&st->succ_inv, s_succ);
}

// One workgroup: the digit of this level.  With g(d) = T at the lower end of bin d = above_e + SE(d) + nonempty - above_m - SM(d) (SE, SM: suffix sums
// of the two histograms), g never grows with d, g(0) > C and g(kCapBins) <= C hold on entry of every level (at level 0 because C >= n_rays), and the
// digit is the largest d with g(d) > C.  Level 0 also decides whether anything is trimmed at all; level 2 ends the selection and writes the record.
__global__ __launch_bounds__(1024) void cap_search_kernel(int level, long long cap_total, CapState* __restrict__ st, const uint32_t* __restrict__ hist,
                                                          CapRecord* __restrict__ rec) {
  __shared__ uint32_t se[1024], sm[1024];
  __shared__ int s_mode, s_digit, s_next;
  __shared__ long long s_tnew;
  const int t = static_cast<int>(threadIdx.x);
  const uint32_t t_now = st->t_now, nonempty = st->nonempty, active = st->active, prefix = st->prefix, above_e = st->above_e, above_m = st->above_m;
  const uint32_t minmode = st->minmode, succ_inv = st->succ_inv;
  if (level == 0) {
    if (static_cast<long long>(t_now) <= cap_total) {      // uniform: the batch fits
      if (t == 0) {
        rec->tstar = -INFINITY;
        rec->t_now = static_cast<int32_t>(t_now);
        rec->t_new = static_cast<int32_t>(t_now);
        rec->trimmed = 0;
        rec->selected += t_now;
        rec->kept += t_now;
      }
      return;
    }
  } else if (active == 0u) return;
  const uint32_t e0 = hist[2 * t], e1 = hist[2 * t + 1], m0 = hist[kCapBins + 2 * t], m1 = hist[kCapBins + 2 * t + 1];
  const int j = 1023 - t;      // suffix sums over t are prefix sums over j
  se[j] = e0 + e1;
  sm[j] = m0 + m1;
  if (t == 0) {
    s_mode = static_cast<int>(minmode);
    s_digit = -1;
    s_next = 1 << 30;
    s_tnew = 0;
  }
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const uint32_t a = j >= off ? se[j - off] : 0u, b = j >= off ? sm[j - off] : 0u;
    __syncthreads();
    se[j] += a;
    sm[j] += b;
    __syncthreads();
  }
  const long long base = static_cast<long long>(above_e) + nonempty - above_m;
  const uint32_t sE = se[j], sM = sm[j];      // over bins 2 t .. kCapBins - 1
  const long long g0 = base + sE - sM, g1 = base + (sE - e0) - (sM - m0), g2 = base + (sE - e0 - e1) - (sM - m0 - m1);      // g(2 t), g(2 t + 1), g(2 t + 2)
  if (level == 0 && t == 0 && g0 <= cap_total) {
    s_mode = 1;
    s_tnew = g0;
  }
  __syncthreads();
  const bool mode_min = s_mode != 0;
  if (!mode_min) {
    if (g1 > cap_total && g2 <= cap_total) {           // bin 2 t + 1 is the digit
      s_digit = 2 * t + 1;
      s_tnew = g2;
      if (level < 2) {
        st->above_e = above_e + (sE - e0 - e1);
        st->above_m = above_m + (sM - m0 - m1);
      }
    } else if (g0 > cap_total && g1 <= cap_total) {    // bin 2 t
      s_digit = 2 * t;
      s_tnew = g1;
      if (level < 2) {
        st->above_e = above_e + (sE - e0);
        st->above_m = above_m + (sM - m0);
      }
    }
  } else {                                             // the lowest occupied bin
    if (e0 != 0u) atomicMin(&s_next, 2 * t);
    else if (e1 != 0u) atomicMin(&s_next, 2 * t + 1);
  }
  __syncthreads();
  if (!mode_min && level == 2) {                       // p's successor inside its own bucket: the lowest occupied bin above the digit
    const int d = s_digit;
    if (2 * t > d && e0 != 0u) atomicMin(&s_next, 2 * t);
    else if (2 * t + 1 > d && e1 != 0u) atomicMin(&s_next, 2 * t + 1);
    __syncthreads();
  }
  if (t != 0) return;
  const int shift = cap_shift(level);
  const int digit = mode_min ? s_next : s_digit;
  long long t_new = mode_min ? (level == 0 ? s_tnew : static_cast<long long>(st->pad[0])) : s_tnew;
  bool done = level == 2, inf = false;
  uint32_t key = prefix;
  if (digit < 0 || (mode_min && digit >= kCapBins)) {      // no non-NaN entry at all (the other case cannot happen): only +inf is left
    done = inf = true;
    t_new = nonempty;
  } else {
    key = prefix | (static_cast<uint32_t>(digit) << shift);
    if (level == 2 && !mode_min) {
      if (s_next < kCapBins) key = prefix | static_cast<uint32_t>(s_next);
      else if (succ_inv != 0u) key = ~succ_inv;
      else inf = true;
    }
  }
  if (!done) {
    st->active = 1u;
    st->minmode = mode_min ? 1u : 0u;
    st->prefix = key;
    st->pad[0] = static_cast<uint32_t>(t_new);
    return;
  }
  const float ts = inf ? INFINITY : cap_value(key);
  st->active = 0u;
  rec->tstar = ts;
  rec->t_now = static_cast<int32_t>(t_now);
  rec->t_new = static_cast<int32_t>(t_new);
  rec->trimmed = 1;
  rec->thr_max = fmaxf(rec->thr_max, ts);
  rec->batches_trimmed += 1;
  rec->selected += t_now;
  rec->kept += t_new;
}

// the threshold map of the batch for the unchanged trim kernels: t*, or -inf (the context's threshold) when nothing is trimmed
__global__ __launch_bounds__(256) void cap_fill_kernel(const CapRecord* __restrict__ rec, int n_rays, float* __restrict__ thr_map) {
  const int i = blockIdx.x * 256 + static_cast<int>(threadIdx.x);
  if (i < n_rays) thr_map[i] = rec->tstar;
}

// the record of a frame before its first batch
__global__ void cap_reset_kernel(CapRecord* __restrict__ rec) {
  rec->tstar = -INFINITY;
  rec->t_now = rec->t_new = rec->trimmed = 0;
  rec->thr_max = -INFINITY;
  rec->batches_trimmed = 0;
  rec->selected = rec->kept = 0;
}

}  // namespace adanerf
