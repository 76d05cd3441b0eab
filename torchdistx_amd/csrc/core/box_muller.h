// Constants and the sqrt fix-up of the normal fill's Box-Muller transform,
// shared between the CDNA4 kernels (csrc/hip/init_kernels.hip) and the
// host test that proves them (tests/cc/test_philox_mulhilo.cc). Header-only
// and host/device-compilable; compiler builtins only.

#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define TDX_BM_HD __host__ __device__ __forceinline__
#else
#define TDX_BM_HD inline
#endif

namespace tdx {
namespace box_muller {

// The Box-Muller angle 2*pi*u2 straight from the random integer:
// u2 * 2*pi = (k * 2^-s) * 2*pi, and scaling by a power of two commutes
// with rounding (nothing here is near the denormal range), so
// fl(fl(k * 2^-s) * 2pi_f32) == fl(k * fl(2pi_f32 * 2^-s)) for every k —
// one multiply instead of two. The constants are derived in double and
// rounded once; the host test pins them to fl(2pi_f32 * 2^-s) bit for bit
// and checks the identity for every k.
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr float kTwoPiF = static_cast<float>(kTwoPi);
constexpr float kAngleScale24 = static_cast<float>(kTwoPi / 16777216.0);
constexpr float kAngleScale16 = static_cast<float>(kTwoPi / 65536.0);

// -2 * ln 2: r^2 = -2 ln(u1) = kNeg2Ln2 * log2(u1).
constexpr float kNeg2Ln2 = -1.3862943611198906f;

// The +-1 ulp fix-up that turns a sqrt estimate `s` of `x` (v_sqrt_f32,
// good to 1 ulp) into the correctly rounded root. Exactly the compiler's
// own sqrtf expansion (same fma operands, same two compares, same order)
// minus the parts of it that Box-Muller's argument can never reach: the
// 2^32 pre-scale / 2^-16 post-scale taken for x < 2^-96, and the class
// select returning x for 0 and +inf. Here x = kNeg2Ln2 * log2(u1), and
// after the FLT_MIN guard on u1
//   16-bit path: u1 in {FLT_MIN} U [2^-16, 1 - 2^-16]
//   f32 path:    u1 in {FLT_MIN} U [2^-24, 1 - 2^-24]
// so the smallest x is kNeg2Ln2 * log2(1 - 2^-24) ~ 1.19e-7 (2.2e-5 on
// the 16-bit path), the largest regular one kNeg2Ln2 * -24 ~ 33.3 (22.2),
// and a zero draw gives u1 = FLT_MIN, log2 = -126, x ~ 174.7: always
// inside [1.1e-7, 175], never below 2^-96 ~ 1.3e-29, never 0, never inf.
//
// `pin` is applied to both residuals before they are compared: identity
// on the host; the kernels pass a register pin that keeps the compiler
// from pairing the two fmas into one packed fp32 instruction.
template <typename Pin>
TDX_BM_HD float sqrt_fixup(float s, float x, Pin pin) {
  const float sm =
      __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) - 1u);
  const float sp =
      __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, s) + 1u);
  const float em = pin(__builtin_fmaf(-sm, s, x));
  const float ep = pin(__builtin_fmaf(-sp, s, x));
  s = em <= 0.0f ? sm : s;
  s = ep > 0.0f ? sp : s;
  return s;
}

}  // namespace box_muller
}  // namespace tdx
