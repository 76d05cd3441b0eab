// Device helpers shared by the fused AnyPrecisionAdamW kernels
// (anyprecision_adamw.hip, anyprecision_adamw_q8.hip, grad_norm.hip): the
// runtime dtype tag, the rounding barrier, the fp64 momentum, the gradient
// scale and the 8-elements-per-lane load. Each kernel file pulls the names
// into its anonymous namespace. Everything here is written with the
// compiler's own types and builtins (no HIP header wrappers), so it inlines
// into functions compiled without the packed fp32 instructions too.

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

// g * scale, one fp32 rounding: the gradient under the device-resident
// clip coefficient (grad_norm.hip). A plain product on purpose: written so
// that the compiler cannot see through it, the kernels' scaled variants
// vectorize and contract the arithmetic after it differently from the
// unscaled ones, and a coefficient of exactly 1 is then no longer
// invisible in the last bit of exp_avg_sq.
__device__ __forceinline__ float scaleGrad(float g, float scale) {
  return g * scale;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float asFloat(uint32_t b) {
  return __builtin_bit_cast(float, b);
}
__device__ __forceinline__ uint32_t asBits(float v) {
  return __builtin_bit_cast(uint32_t, v);
}

// The bf16 code of the fp32 value v under stochastic rounding with the 16
// random bits rand16, in integers on the sign-magnitude encoding: the carry
// of low16(bits) + rand16 moves the kept half one code away from zero, with
// probability low16(bits) / 65536 exactly, so a representable value never
// moves. inf and NaN convert as the plain store does; a finite value never
// becomes an infinity (it stays at the largest finite bf16).
__device__ __forceinline__ uint32_t bf16BitsStochastic(float v,
                                                       uint32_t rand16) {
  const uint32_t b = asBits(roundBarrier(v));
  if ((b & 0x7f800000u) == 0x7f800000u) {
    return static_cast<uint32_t>(
        __builtin_bit_cast(uint16_t, static_cast<__bf16>(asFloat(b))));
  }
  const uint32_t b2 = b + rand16;
  if ((b2 & 0x7f800000u) == 0x7f800000u) {
    return ((b >> 16) & 0x8000u) | 0x7f7fu;
  }
  return b2 >> 16;
}

// tag: a DT as int (the q8 kernel continues the numbering with its fp8
// formats, which never reach these two).
__device__ __forceinline__ float loadOne(const void* p, int tag, int64_t i) {
  if (tag == static_cast<int>(DT::kF32)) {
    return static_cast<const float*>(p)[i];
  }
  if (tag == static_cast<int>(DT::kBF16)) {
    return asFloat(
        static_cast<uint32_t>(static_cast<const uint16_t*>(p)[i]) << 16);
  }
  return static_cast<float>(static_cast<const _Float16*>(p)[i]);
}

// 8 elements of one lane as fp32. `wide` (all 8 inside the tensor, base
// pointer 16-byte aligned) takes one 16-byte access for a 16-bit dtype and
// two for fp32; otherwise the first `count` elements load one by one and
// the rest read as zero.
__device__ __forceinline__ void load8Plain(const void* p, int tag, int64_t e0,
                                           int count, bool wide, float* out) {
  if (!wide) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      out[j] = j < count ? loadOne(p, tag, e0 + j) : 0.0f;
    }
    return;
  }
  if (tag == static_cast<int>(DT::kF32)) {
    const f32x4* q =
        reinterpret_cast<const f32x4*>(static_cast<const float*>(p) + e0);
    const f32x4 a = q[0];
    const f32x4 b = q[1];
    out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
    out[4] = b.x; out[5] = b.y; out[6] = b.z; out[7] = b.w;
    return;
  }
  const u32x4 pk = *reinterpret_cast<const u32x4*>(
      static_cast<const uint16_t*>(p) + e0);
  const uint32_t w[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (tag == static_cast<int>(DT::kBF16)) {
      out[2 * k] = asFloat(w[k] << 16);
      out[2 * k + 1] = asFloat(w[k] & 0xffff0000u);
    } else {
      const half2v h = __builtin_bit_cast(half2v, w[k]);
      out[2 * k] = static_cast<float>(h.x);
      out[2 * k + 1] = static_cast<float>(h.y);
    }
  }
}

}  // namespace adamw_device
}  // namespace tdx
