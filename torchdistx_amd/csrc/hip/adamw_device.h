// Device helpers shared by the fused AnyPrecisionAdamW kernels
// (anyprecision_adamw.hip, anyprecision_adamw_q8.hip): the runtime dtype
// tag, the rounding barrier and the fp64 momentum. Each kernel file pulls
// the names into its anonymous namespace.

#pragma once

#include <hip/hip_runtime.h>

namespace tdx {
namespace adamw_device {

enum class DT : int { kF32 = 0, kBF16 = 1, kF16 = 2 };

// Pins the f32 rounding step before narrowing conversions, so every
// code path (generic, vectorized, batched) rounds identically — the
// compiler otherwise fuses fma+convert (v_fma_mix*) in some shapes only
// (see init_kernels.hip from_float).
__device__ __forceinline__ float roundBarrier(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// m + w * (g - m), rounded once. Where g is close to -m * (1 - w) / w
// (g ~ -9 m at beta1 = 0.9) the result cancels, and the fp32 rounding
// errors of g - m and of the product, a few 2^-24 (|m| + |g|), would be
// thousands of ulps of it; the update is step_size * exp_avg / denom and
// would inherit them, which next to a parameter much smaller than the
// update is far outside the fp32 rounding of that parameter. Two fp32
// operands differ and multiply exactly enough in fp64 (full rate on
// CDNA), so the momentum alone is formed there: five VALU ops.
__device__ __forceinline__ float lerpMomentum(float m, float g, float w) {
  const double md = m;
  return static_cast<float>(
      fma(static_cast<double>(w), static_cast<double>(g) - md, md));
}

}  // namespace adamw_device
}  // namespace tdx
