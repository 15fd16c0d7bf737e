// the two networks in any topology the reference's model classes can export (BaseNet / NeRF,
// src/models.py:18-82, 199-277: depth 2..8, width 64 / 128 / 256 (512: the wide form at the end), trunk skips at any layers or none) and the
// raySampleInput oracle input (src/features.py:876-888; viewer: updateSpherePosDirBatchedUnrolledEnc with additional
// samples, adanerf_real_time_viewer/src/cuda/base_cuda_kernels.cu:99-145) -- on the exact-fp32 MFMA engine
// (v_mfma_f32_32x32x2_f32, k_mlp_f32.hip.hpp) with a run-time loop over the hidden layers.  Every shipped config is
// 8 x 256 / skip 4 and runs on the specialised kernels instead; these exist so that other exports load and render
// (at the fp32-MFMA rate, 1/16 of the 16-bit engines' peak, on networks that are several times smaller).
// Device code only (gfx950, wave64); compiled in launch_f32.hip (without -amdgpu-mfma-vgpr-form).
#pragma once
#include "k_mlp16.hip.hpp"
#include "k_mlp_f32.hip.hpp"

namespace adanerf {

// Layer 0 of a sampling net with raySampleInput: K = [dir PE | pos PE | A x PE(point a)].  The A points are walked in a
// run-time loop with all MT accumulators live (K-major fragments, pack.cpp emit_ray_samples); the first part is the usual
// tile-major block.  PE(point) = encode((p + d z_a) / d1) with the identity slots scaled back by d1, as the reference does.
template <int FP, int Q0, int MT>
__device__ __forceinline__ void layer0_ray_samples(const u32x4* __restrict__ w0, const u32x4* __restrict__ wr, const float* __restrict__ bias,
                                                   int lane, const float* in0, const float p[3], const float d[3], const GenericTopo& t,
                                                   float* out) {
  constexpr int QP = pe_slots(FP);
  const int h = lane >> 5;
  f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const float4* bp = reinterpret_cast<const float4*>(bias + (m * 2 + h) * 16);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 b = bp[g];
      acc[m][4 * g + 0] = b.x;
      acc[m][4 * g + 1] = b.y;
      acc[m][4 * g + 2] = b.z;
      acc[m][4 * g + 3] = b.w;
    }
#pragma unroll
    for (int s4 = 0; s4 < Q0 / 4; ++s4) {
      const f32x4 a = reinterpret_cast<const f32x4*>(w0)[(m * (Q0 / 4) + s4) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], in0[4 * s4 + e], acc[m], 0, 0, 0);
    }
  }
#pragma unroll 1
  for (int a = 0; a < t.ray_samples; ++a) {
    const float z = t.rsi_z[a];
    float x[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = __fadd_rn(p[i], __fmul_rn(d[i], z)) / t.rsi_d1;
    float tt[QP];
    pe_eval<FP, true>(x, h, tt);
    tt[3 * FP] = __fmul_rn(tt[3 * FP], t.rsi_d1);             // enc[..., :3] *= d1  (src/features.py:886)
    tt[3 * FP + 1] = __fmul_rn(tt[3 * FP + 1], t.rsi_d1);
    const f32x4* wa = reinterpret_cast<const f32x4*>(wr) + static_cast<size_t>(a) * (QP / 4) * MT * 64 + lane;
#pragma unroll
    for (int s4 = 0; s4 < QP / 4; ++s4)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const f32x4 f = wa[(s4 * MT + m) * 64];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(f[e], tt[4 * s4 + e], acc[m], 0, 0, 0);
      }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) out[16 * m + r] = fmaxf(acc[m][r], 0.f);
}

// A1+A2+A3 for any sampling-net topology.  One wave = 32 rays, 4 waves per workgroup, like sample_mlp_kernel.
template <int FP, int FD, int W>
__global__ __launch_bounds__(256) void sample_mlp_gen_kernel(SampleArgs a, GenericTopo t) {
  constexpr int QD = pe_slots(FD), QP = pe_slots(FP), Q0 = QD + QP, QW = W / 2, MT = W / 32;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int blk = blockIdx.x * 4 + wave;
  if (blk * 32 >= a.n_rays) return;
  const int local = blk * 32 + j;
  const bool valid = local < a.n_rays;
  const int ray = a.first_ray + (valid ? local : a.n_rays - 1);
  float nds[3], p[3], u[3];
  sample_ray(a.g, ray, nds, p, u);

  float in0[Q0], bufA[QW], bufB[QW];
  pe_eval<FD, true>(u, h, in0);          // [dir PE | pos PE]  (src/features.py:868-874)
  pe_eval<FP, true>(p, h, in0 + QD);
  const u32x4* w = a.net.w;
  const float* b = a.net.bias;
  if (t.ray_samples > 0)
    layer0_ray_samples<FP, Q0, MT>(w + a.net.w_off[0], w + t.rsi_w_off, b + a.net.b_off[0], lane, in0, p, nds, t, bufB);
  else
    layer_f32<Q0, 0, MT, true>(w + a.net.w_off[0], b + a.net.b_off[0], lane, in0, in0, bufB);
#pragma unroll 1
  for (int l = 1; l + 1 < t.depth; ++l) {
    asm volatile("" : "+v"(w), "+v"(b));   // keep the fragment loads inside the loop (see shade_mlp32_kernel)
    layer_f32<QW, 0, MT, true>(w + a.net.w_off[l], b + a.net.b_off[l], lane, bufB, bufB, bufA);
#pragma unroll
    for (int i = 0; i < QW; ++i) bufB[i] = bufA[i];
  }
  float out[64];
  layer_f32<QW, 0, 4, false>(w + a.net.w_off[t.depth - 1], b + a.net.b_off[t.depth - 1], lane, bufB, bufB, out);

  if (valid) {
    if (a.oracle_out) {
      float* o = a.oracle_out + static_cast<size_t>(local) * kBins;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(o + 32 * m + 8 * g + 4 * h) =
              make_float4(out[16 * m + 4 * g], out[16 * m + 4 * g + 1], out[16 * m + 4 * g + 2], out[16 * m + 4 * g + 3]);
    }
    if (a.rays_out) {
      float ro[3] = {p[0], p[1], p[2]}, rd[3] = {nds[0], nds[1], nds[2]};
      if (a.g.use_ndc) ndc_ray(a.g, p, nds, ro, rd);
      float4* r = reinterpret_cast<float4*>(a.rays_out + static_cast<size_t>(local) * 8);
      if (h == 0) r[0] = make_float4(ro[0], ro[1], ro[2], 0.f);
      else r[1] = make_float4(rd[0], rd[1], rd[2], 0.f);
    }
  }
}

// A5+A6 for any shading-net topology (NeRF trunk of t.depth layers of width W, skip after layer t.skip, then
// feature (+ alpha row), views, rgb).
template <int FP, int FD, int W>
__global__ __launch_bounds__(256) void shade_mlp32_gen_kernel(ShadeArgs a, GenericTopo t) {
  constexpr int QP = pe_slots(FP), QD = pe_slots(FD), QW = W / 2, MT = W / 32;
  constexpr int TILE = 4 * 32;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int j = lane & 31, h = lane >> 5;
  int total = a.total ? *a.total : a.max_samples;
  if (total > a.max_samples) total = a.max_samples;
  const u32x4* w = a.net.w;
  const float* b = a.net.bias;

  for (int tile = blockIdx.x; tile * TILE < total; tile += gridDim.x) {
    const int s = tile * TILE + wave * 32 + j;
    if (tile * TILE + wave * 32 >= total) continue;
    asm volatile("" : "+v"(w), "+v"(b));
    float x[3], dpe[3];
    const uint64_t outside = load_sample(a, s, total, x, dpe);
    float pts[QP], dirs[QD], hA[QW], hB[QW + 16];      // hB also receives the (MT + 1)-tile feature (+ alpha) layer
    pe_eval<FP, true>(x, h, pts);
    pe_eval<FD, true>(dpe, h, dirs);
    layer_f32<QP, 0, MT, true>(w + a.net.w_off[0], b + a.net.b_off[0], lane, pts, pts, hA);
#pragma unroll 1
    for (int l = 1; l < t.depth; ++l) {
      asm volatile("" : "+v"(w), "+v"(b));
      if ((t.cat_mask >> l) & 1) layer_f32<QP, QW, MT, true>(w + a.net.w_off[l], b + a.net.b_off[l], lane, pts, hA, hB);      // cat([pts, h])
      else layer_f32<QW, 0, MT, true>(w + a.net.w_off[l], b + a.net.b_off[l], lane, hA, hA, hB);
#pragma unroll
      for (int i = 0; i < QW; ++i) hA[i] = hB[i];
    }
    const int lf = t.depth;
    layer_f32<QW, 0, MT + 1, false>(w + a.net.w_off[lf], b + a.net.b_off[lf], lane, hA, hA, hB);        // feature (+ alpha row)
    const float alpha = hB[QW];
    layer_f32<QW, QD, MT / 2, true>(w + a.net.w_off[lf + 1], b + a.net.b_off[lf + 1], lane, hB, dirs, hA);   // cat([feature, dir])
    float rgb[16];
    layer_f32<QW / 2, 0, 1, false>(w + a.net.w_off[lf + 2], b + a.net.b_off[lf + 2], lane, hA, hA, rgb);
    if (h == 0 && s < total) store_raw_f32(a, s, rgb[0], rgb[1], rgb[2], alpha, outside_lane(outside));
  }
}

// ---- wide form: hidden width 512 (layout.hpp act_feature_wide) ----------------------------------------------------------------------
// The 32x32x2 form above keeps W / 2 fp32 activations per lane and buffer: hA[256] + hB[272] at W = 512, more than the register file.
// v_mfma_f32_16x16x4_f32 on 16-sample blocks halves that (W / 4 = 128 per buffer) at the same rate (64 FLOP / clk / SIMD) and the same
// arithmetic: both f32 forms accumulate every product into the fp32 sum with one fma, in k order (no scratch, exact fp32).
// Fragments [m][s4][lane][4] of 16-row tiles, bias blocks [m][g][4] (pack.cpp emit_wide).

// encoding slots of lane group g: slot q is the 32-row form's slot 2 q + (g >> 1) of lane-half g & 1 -- the values pe_eval computes
template <int F, bool SMALL>
__device__ __forceinline__ void pe_wide_slots(const float x[3], int h, bool hi, float* out) {
  auto arg = [&](int q) { return x[q % 3] * static_cast<float>(1 << (q / 3)); };
  auto trig = [&](float v) { return SMALL ? sin_or_cos_small(v, h) : sin_or_cos(v, h); };
  auto ident = [&](int q) { return q == 3 * F ? (h ? x[2] : x[0]) : (q == 3 * F + 1 ? (h ? 0.f : x[1]) : 0.f); };
#pragma unroll
  for (int s = 0; s < pe_slots(F) / 2; ++s) {
    const int q0 = 2 * s, q1 = 2 * s + 1;
    if (q1 < 3 * F) out[s] = trig(hi ? arg(q1) : arg(q0));
    else if (q0 < 3 * F) {
      const float v = trig(arg(q0));
      out[s] = hi ? ident(q1) : v;
    } else {
      out[s] = hi ? ident(q1) : ident(q0);
    }
  }
}
template <int F>
__device__ __forceinline__ void pe_eval_wide(const float x[3], int g, float* out) {
  const float amax = fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fabsf(x[2])) * static_cast<float>(1 << (F > 0 ? F - 1 : 0));
  const bool small = __builtin_amdgcn_ballot_w64(!(amax < 1.0e5f)) == 0ull;      // as pe_eval: one wave-uniform range test
  if (small) pe_wide_slots<F, true>(x, g & 1, (g >> 1) != 0, out);
  else pe_wide_slots<F, false>(x, g & 1, (g >> 1) != 0, out);
}

// One layer for one 16-sample block: Q1 + Q2 input slots per lane group (two register segments), MT output tiles of 16 rows.
template <int Q1, int Q2, int MT, bool RELU>
__device__ __forceinline__ void layer_f32_wide(const u32x4* __restrict__ w, const float* __restrict__ bias, int lane, const float* in1,
                                               const float* in2, float* out) {
  constexpr int QS = Q1 + Q2;
  static_assert(Q1 % 4 == 0 && Q2 % 4 == 0, "fp32 engine groups 4 k-steps per 16-byte fragment");
  const int g = lane >> 4;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    f32x4 acc = *reinterpret_cast<const f32x4*>(bias + m * 16 + 4 * g);
#pragma unroll
    for (int s4 = 0; s4 < QS / 4; ++s4) {
      const f32x4 a = reinterpret_cast<const f32x4*>(w)[(m * (QS / 4) + s4) * 64 + lane];      // float vector: see layer_f32
      const float* in = (4 * s4 < Q1) ? (in1 + 4 * s4) : (in2 + (4 * s4 - Q1));
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], in[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], in[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], in[2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], in[3], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) out[4 * m + r] = RELU ? fmaxf(acc[r], 0.f) : acc[r];
  }
}

// A1+A2+A3 for a sampling net of width 512 (no raySampleInput).  One wave = 16 rays, 4 waves per workgroup (64 rays).
template <int FP, int FD>
__global__ __launch_bounds__(256) void sample_mlp_gen_wide_kernel(SampleArgs a, GenericTopo t) {
  constexpr int QD = pe_slots(FD) / 2, QP = pe_slots(FP) / 2, Q0 = QD + QP, QW = kWideWidth / 4, MT = kWideWidth / 16;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int blk = blockIdx.x * 4 + wave;
  if (blk * 16 >= a.n_rays) return;
  const int local = blk * 16 + j;
  const bool valid = local < a.n_rays;
  const int ray = a.first_ray + (valid ? local : a.n_rays - 1);
  float nds[3], p[3], u[3];
  sample_ray(a.g, ray, nds, p, u);

  float bufA[QW], bufB[QW];
  {
    float in0[Q0];
    pe_eval_wide<FD>(u, g, in0);          // [dir PE | pos PE]  (src/features.py:868-874)
    pe_eval_wide<FP>(p, g, in0 + QD);
    layer_f32_wide<Q0, 0, MT, true>(a.net.w + a.net.w_off[0], a.net.bias + a.net.b_off[0], lane, in0, in0, bufB);
  }
  const u32x4* w = a.net.w;
  const float* b = a.net.bias;
#pragma unroll 1
  for (int l = 1; l + 1 < t.depth; ++l) {
    asm volatile("" : "+v"(w), "+v"(b));   // keep the fragment loads inside the loop (see shade_mlp32_kernel)
    layer_f32_wide<QW, 0, MT, true>(w + a.net.w_off[l], b + a.net.b_off[l], lane, bufB, bufB, bufA);
#pragma unroll
    for (int i = 0; i < QW; ++i) bufB[i] = bufA[i];
  }
  float out[32];      // bins 16 m + 4 g + r of tile m = 0..7
  layer_f32_wide<QW, 0, kBins / 16, false>(w + a.net.w_off[t.depth - 1], b + a.net.b_off[t.depth - 1], lane, bufB, bufB, out);

  if (valid) {
    if (a.oracle_out) {
      float* o = a.oracle_out + static_cast<size_t>(local) * kBins;
#pragma unroll
      for (int m = 0; m < kBins / 16; ++m)
        *reinterpret_cast<float4*>(o + 16 * m + 4 * g) = make_float4(out[4 * m], out[4 * m + 1], out[4 * m + 2], out[4 * m + 3]);
    }
    if (a.rays_out && g < 2) {
      float ro[3] = {p[0], p[1], p[2]}, rd[3] = {nds[0], nds[1], nds[2]};
      if (a.g.use_ndc) ndc_ray(a.g, p, nds, ro, rd);
      float4* r = reinterpret_cast<float4*>(a.rays_out + static_cast<size_t>(local) * 8);
      if (g == 0) r[0] = make_float4(ro[0], ro[1], ro[2], 0.f);
      else r[1] = make_float4(rd[0], rd[1], rd[2], 0.f);
    }
  }
}

// A5+A6 for a shading net (or either net of coarse/fine mode) of width 512 in fp32.  One wave = 16 samples.  The position encoding is
// evaluated again at every skip layer and the direction encoding where it is consumed: neither stays live across the layer stack.
template <int FP, int FD>
__global__ __launch_bounds__(256) void shade_mlp32_gen_wide_kernel(ShadeArgs a, GenericTopo t) {
  constexpr int QP = pe_slots(FP) / 2, QD = pe_slots(FD) / 2, QW = kWideWidth / 4, MT = kWideWidth / 16;
  constexpr int TILE = 4 * 16;
  const int lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int j = lane & 15, g = lane >> 4;
  int total = a.total ? *a.total : a.max_samples;
  if (total > a.max_samples) total = a.max_samples;
  const u32x4* w = a.net.w;
  const float* b = a.net.bias;

  for (int tile = blockIdx.x; tile * TILE < total; tile += gridDim.x) {
    const int s = tile * TILE + wave * 16 + j;
    if (tile * TILE + wave * 16 >= total) continue;
    asm volatile("" : "+v"(w), "+v"(b));
    float x[3], dpe[3];
    const uint64_t outside = load_sample(a, s, total, x, dpe);
    float hA[QW], hB[QW + 4];      // hB also receives the (MT + 1)-tile feature (+ alpha) layer
    {
      float pts[QP];
      pe_eval_wide<FP>(x, g, pts);
      layer_f32_wide<QP, 0, MT, true>(w + a.net.w_off[0], b + a.net.b_off[0], lane, pts, pts, hA);
    }
#pragma unroll 1
    for (int l = 1; l < t.depth; ++l) {
      asm volatile("" : "+v"(w), "+v"(b));
      if ((t.cat_mask >> l) & 1) {      // cat([pts, h])
        float pts[QP];
        pe_eval_wide<FP>(x, g, pts);
        layer_f32_wide<QP, QW, MT, true>(w + a.net.w_off[l], b + a.net.b_off[l], lane, pts, hA, hB);
      } else {
        layer_f32_wide<QW, 0, MT, true>(w + a.net.w_off[l], b + a.net.b_off[l], lane, hA, hA, hB);
      }
#pragma unroll
      for (int i = 0; i < QW; ++i) hA[i] = hB[i];
    }
    const int lf = t.depth;
    layer_f32_wide<QW, 0, MT + 1, false>(w + a.net.w_off[lf], b + a.net.b_off[lf], lane, hA, hA, hB);        // feature (+ alpha row)
    const float alpha = hB[QW];      // tile MT, row 0: group 0
    {
      float dirs[QD];
      pe_eval_wide<FD>(dpe, g, dirs);
      layer_f32_wide<QW, QD, MT / 2, true>(w + a.net.w_off[lf + 1], b + a.net.b_off[lf + 1], lane, hB, dirs, hA);   // cat([feature, dir])
    }
    float rgb[4];
    layer_f32_wide<QW / 2, 0, 1, false>(w + a.net.w_off[lf + 2], b + a.net.b_off[lf + 2], lane, hA, hA, rgb);
    if (g == 0 && s < total) store_raw_f32(a, s, rgb[0], rgb[1], rgb[2], alpha, outside_lane(outside));
  }
}

}  // namespace adanerf
