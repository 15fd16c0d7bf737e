// See launch_f32.hpp: the fp32-MFMA kernels, compiled WITHOUT -amdgpu-mfma-vgpr-form.
#include "launch_f32.hpp"

#include "k_mlp16.hip.hpp"     // shade_mlp32_kernel (shares ShadeArgs / load_sample with the 16-bit shading kernel)
#include "k_mlp_f32.hip.hpp"   // sample_mlp_kernel
#include "k_generic_f32.hip.hpp"
#include "k_probe.hip.hpp"

namespace adanerf {

hipError_t probe_mfma_rate(int operands, bool f16, double target_ms, int compute_units, hipStream_t stream, double* tflops, double* mhz) {
  using namespace probe;
  float* sink = nullptr;
  uint64_t* clocks = nullptr;
  hipError_t rc = hipMalloc(reinterpret_cast<void**>(&sink), 64);
  if (rc != hipSuccess) return rc;
  if ((rc = hipMalloc(reinterpret_cast<void**>(&clocks), 64)) != hipSuccess) {
    (void)hipFree(sink);
    return rc;
  }
  rc = dispatch<false, true>(f16, [&](auto f) {
    return dispatch<kZero, kConstant, kRandom, kRelu>(operands, [&](auto mode) {
      return mfma_rate<2, f(), mode()>(compute_units, target_ms, stream, sink, clocks, tflops, mhz);
    }, hipErrorInvalidValue);
  }, hipErrorInvalidValue);
  (void)hipFree(sink);
  (void)hipFree(clocks);
  return rc;
}

hipError_t launch_sample_mlp_f32(const SampleArgs& a, int enc, unsigned grid, hipStream_t stream) {
  return dispatch<kEnc10_4, kEnc2_2>(enc, [&](auto e) {
    hipLaunchKernelGGL((sample_mlp_kernel<enc_fp(e()), enc_fd(e())>), dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
  }, hipErrorInvalidValue);
}

hipError_t launch_shade_mlp_f32(GridCache& gc, const ShadeArgs& a, int tiles, hipStream_t stream) {
  return launch_persistent(gc, shade_mlp32_kernel<10, 4>, tiles, 256, stream, a);
}

hipError_t launch_sample_mlp_gen(const SampleArgs& a, const GenericTopo& t, int enc, int width, unsigned grid, hipStream_t stream) {
  if (width == kWideWidth && t.ray_samples > 0) return hipErrorInvalidValue;      // the packer refuses raySampleInput at this width
  return dispatch<kEnc10_4, kEnc2_2, kEncMax>(enc, [&](auto e) {
    constexpr int FP = enc_fp(e()), FD = enc_fd(e());
    if (width == kWideWidth) {      // 16-ray blocks: 64 rays per workgroup (grid: the caller's, counted in 128-ray workgroups)
      hipLaunchKernelGGL((sample_mlp_gen_wide_kernel<FP, FD>), dim3((a.n_rays + 63) / 64), dim3(256), 0, stream, a, t);
      return hipGetLastError();
    }
    return dispatch<64, 128, 256>(width, [&](auto w) {
      hipLaunchKernelGGL((sample_mlp_gen_kernel<FP, FD, w()>), dim3(grid), dim3(256), 0, stream, a, t);
      return hipGetLastError();
    }, hipErrorInvalidValue);
  }, hipErrorInvalidValue);
}

hipError_t launch_shade_mlp_gen(GridCache& gc, const ShadeArgs& a, const GenericTopo& t, int enc, int width, int tiles, hipStream_t stream) {
  return dispatch<kEnc10_4, kEncMax>(enc, [&](auto e) {
    constexpr int FP = enc_fp(e()), FD = enc_fd(e());
    if (width == kWideWidth) return launch_persistent(gc, shade_mlp32_gen_wide_kernel<FP, FD>, tiles, 256, stream, a, t);
    return dispatch<64, 128, 256>(width, [&](auto w) { return launch_persistent(gc, shade_mlp32_gen_kernel<FP, FD, w()>, tiles, 256, stream, a, t); },
                                  hipErrorInvalidValue);
  }, hipErrorInvalidValue);
}

}  // namespace adanerf
