// Launchers of the two kernels that run on the fp32 MFMA engine (v_mfma_f32_32x32x2_f32).  They live in their own
// translation unit (launch_f32.hip) because the rest of the library is compiled with -mllvm -amdgpu-mfma-vgpr-form=1
// (MFMA accumulators in architectural VGPRs: good for the 16-bit kernels' VALU epilogues, 1.48 -> 1.35 ms in the
// split-precision sampling kernel) and that option slows these two down (fp32 sampling 5.3 -> 9.6 ms, fp32 shading
// 60 -> 67 ms): their accumulators belong in AGPRs.
#pragma once
#include "launch.hpp"

namespace adanerf {
struct SampleArgs;
struct ShadeArgs;
struct GenericTopo;

// sample_mlp_kernel<10,4> (enc = kEnc10_4) or <2,2> (kEnc2_2); grid = ceil(n_rays / 128) workgroups of 256 threads
hipError_t launch_sample_mlp_f32(const SampleArgs& a, int enc, unsigned grid, hipStream_t stream);
// shade_mlp32_kernel<10,4> over `tiles` 128-sample tiles on its persistent grid
hipError_t launch_shade_mlp_f32(GridCache& gc, const ShadeArgs& a, int tiles, hipStream_t stream);

// Generic-topology kernels (k_generic_f32.hip.hpp): width 64 / 128 / 256, run-time depth / skip / raySampleInput; width 512 (kWideWidth)
// in the wide form: 16-sample blocks, 64 rays / samples per workgroup (the sampling launcher sizes that grid itself; the shading
// caller counts its tiles in 64 samples), no raySampleInput.
// enc: slot layout of the positional encodings the network was packed with (params.hpp) -- kEnc10_4, kEnc2_2 (sampling nets only) or
// kEncMax.  hipErrorInvalidValue for a width / layout without an instantiation.
hipError_t launch_sample_mlp_gen(const SampleArgs& a, const GenericTopo& t, int enc, int width, unsigned grid, hipStream_t stream);
hipError_t launch_shade_mlp_gen(GridCache& gc, const ShadeArgs& a, const GenericTopo& t, int enc, int width, int tiles, hipStream_t stream);

// Measurement hook (k_probe.hip.hpp; include/adanerf_hip.h adanerf_probe_mfma): register-only v_mfma_f32_32x32x16_{bf16,f16} loops on every
// CU for ~target_ms, operands 0 zero / 1 constant / 2 random / 3 relu-like, two accumulator chains per wave and one wave per SIMD (the
// shading kernel's form).  Synchronises the stream.
hipError_t probe_mfma_rate(int operands, bool f16, double target_ms, int compute_units, hipStream_t stream, double* tflops, double* mhz);
}  // namespace adanerf
