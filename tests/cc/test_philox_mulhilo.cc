// Host checks for the identities the normal-fill kernels lean on
// (torchdistx_amd/csrc/hip/init_kernels.hip): the one-product mulhilo32,
// the three-input xor's truth table, and the folded angle constants and
// sqrt fix-up the kernels take from csrc/core/box_muller.h. IEEE f32
// multiplies and fmas are the same on the CPU, so the float identities
// are checked here for EVERY input the kernels can see. Built and run by
// tests/test_philox_mulhilo_cc.py with a plain g++.

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../torchdistx_amd/csrc/core/box_muller.h"
#include "../../torchdistx_amd/csrc/core/philox.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (failures < 20) {                                              \
        std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      }                                                                 \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  return u;
}

static float float_of(uint32_t u) {
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

// The kernels' fused form: both halves from one 64-bit product.
static void mulhilo32_fused(uint32_t a, uint32_t b, uint32_t* lo,
                            uint32_t* hi) {
  const uint64_t p = static_cast<uint64_t>(a) * b;
  *lo = static_cast<uint32_t>(p);
  *hi = static_cast<uint32_t>(p >> 32);
}

// Independent high half: schoolbook on 16-bit limbs, 32-bit products only.
static uint32_t mulhi32_limbs(uint32_t a, uint32_t b) {
  const uint32_t a0 = a & 0xffffu, a1 = a >> 16;
  const uint32_t b0 = b & 0xffffu, b1 = b >> 16;
  const uint32_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint32_t mid = (p00 >> 16) + (p01 & 0xffffu) + (p10 & 0xffffu);
  return p11 + (p01 >> 16) + (p10 >> 16) + (mid >> 16);
}

static void check_pair(uint32_t a, uint32_t b) {
  uint32_t lo, hi;
  mulhilo32_fused(a, b, &lo, &hi);
  CHECK(lo == a * b);
  CHECK(hi == tdx::philox::mulhi32(a, b));
  CHECK(hi == mulhi32_limbs(a, b));
}

// v_bitop3_b32's definition: result bit = bit (a<<2 | b<<1 | c) of the
// 8-bit truth table.
static uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c, uint32_t table) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) {
    const uint32_t idx =
        (((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u);
    r |= ((table >> idx) & 1u) << i;
  }
  return r;
}

using tdx::box_muller::kAngleScale16;
using tdx::box_muller::kAngleScale24;
using tdx::box_muller::kNeg2Ln2;
using tdx::box_muller::kTwoPi;
using tdx::box_muller::sqrt_fixup;

// The literal the two-multiply form multiplied by.
constexpr float kTwoPiF = 6.2831853071795865f;

int main() {
  // --- mulhilo32: fused form == a*b / mulhi32 form -----------------------
  const uint32_t edges[] = {0u,          1u,          0xFFFFFFFFu,
                            0x80000000u, 0xD2511F53u, 0xCD9E8D57u};
  for (uint32_t a : edges) {
    for (uint32_t b : edges) {
      check_pair(a, b);
    }
  }
  uint64_t state = 0x9E3779B97F4A7C15ull;  // splitmix64
  auto next = [&state]() {
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  for (int i = 0; i < (1 << 20); ++i) {
    const uint64_t r = next();
    const uint32_t a = static_cast<uint32_t>(r);
    const uint32_t b = static_cast<uint32_t>(r >> 32);
    check_pair(a, b);
    // The products Philox actually forms: multiplier * counter word.
    check_pair(0xD2511F53u, a);
    check_pair(0xCD9E8D57u, b);
  }

  // --- three-input xor: truth table 0x96 is odd parity --------------------
  for (uint32_t idx = 0; idx < 8; ++idx) {
    const uint32_t a = (idx >> 2) & 1u, b = (idx >> 1) & 1u, c = idx & 1u;
    CHECK(((0x96u >> idx) & 1u) == (a ^ b ^ c));
  }
  for (int i = 0; i < 4096; ++i) {
    const uint64_t r = next(), q = next();
    const uint32_t a = static_cast<uint32_t>(r);
    const uint32_t b = static_cast<uint32_t>(r >> 32);
    const uint32_t c = static_cast<uint32_t>(q);
    CHECK(bitop3(a, b, c, 0x96u) == (a ^ b ^ c));
  }

  // --- folded angle constants ---------------------------------------------
  // Rounded once from double == the f32 2*pi scaled by the power of two,
  // which is the value the two-multiply form multiplies by in effect.
  CHECK(bits_of(kAngleScale16) == bits_of(kTwoPiF * (1.0f / 65536.0f)));
  CHECK(bits_of(kAngleScale24) == bits_of(kTwoPiF * (1.0f / 16777216.0f)));
  CHECK(bits_of(kAngleScale16) == bits_of(std::ldexp(kTwoPiF, -16)));
  CHECK(bits_of(kAngleScale24) == bits_of(std::ldexp(kTwoPiF, -24)));
  CHECK(bits_of(static_cast<float>(kTwoPi)) == bits_of(kTwoPiF));
  CHECK(bits_of(tdx::box_muller::kTwoPiF) == bits_of(kTwoPiF));

  // fl(fl(k * 2^-s) * 2pi) == fl(k * fl(2pi * 2^-s)) for EVERY input: all
  // 2^16 draws of the bf16/f16 path, all 2^24 of the f32 path.
  for (uint32_t k = 0; k < (1u << 16); ++k) {
    volatile float u = static_cast<float>(k) * (1.0f / 65536.0f);
    CHECK(bits_of(u) == bits_of(tdx::philox::u16_to_uniform(k)));
    const float two_step = kTwoPiF * u;
    const float folded = static_cast<float>(k) * kAngleScale16;
    CHECK(bits_of(two_step) == bits_of(folded));
  }
  for (uint32_t k = 0; k < (1u << 24); ++k) {
    volatile float u = static_cast<float>(k) * (1.0f / 16777216.0f);
    const float two_step = kTwoPiF * u;
    const float folded = static_cast<float>(k) * kAngleScale24;
    CHECK(bits_of(two_step) == bits_of(folded));
  }
  CHECK(bits_of(tdx::philox::u32_to_uniform(0xFFFFFFFFu)) ==
        bits_of(16777215.0f * (1.0f / 16777216.0f)));

  // --- sqrt fix-up ----------------------------------------------------------
  // From any first estimate within 1 ulp (v_sqrt_f32's accuracy) the fix-up
  // lands on the correctly rounded sqrtf, over Box-Muller's whole argument
  // range [1.1e-7, 175] — so dropping the range scaling and the 0/inf
  // select around it loses nothing there.
  const float kLo = 1.1e-7f, kHi = 175.0f;
  CHECK(kLo > std::ldexp(1.0f, -96));
  const uint32_t lo_bits = bits_of(kLo), hi_bits = bits_of(kHi);
  for (uint32_t xb = lo_bits; xb <= hi_bits; xb += 97u) {
    const float x = float_of(xb);
    const float exact = std::sqrt(x);
    for (int d = -1; d <= 1; ++d) {
      const float s0 = float_of(bits_of(exact) + static_cast<uint32_t>(d));
      CHECK(bits_of(sqrt_fixup(s0, x, [](float v) { return v; })) ==
            bits_of(exact));
    }
  }
  // Both ends of the argument range for both paths, and the zero draw.
  CHECK(bits_of(kNeg2Ln2) == bits_of(-1.3862943611198906f));
  const float args[] = {
      kNeg2Ln2 * std::log2(1.0f - 1.0f / 65536.0f),     // ~2.2e-5
      kNeg2Ln2 * std::log2(1.0f - 1.0f / 16777216.0f),  // ~1.19e-7
      kNeg2Ln2 * -16.0f, kNeg2Ln2 * -24.0f,
      kNeg2Ln2 * -126.0f,                               // u1 = FLT_MIN
  };
  for (float x : args) {
    CHECK(x >= kLo && x <= kHi);
    CHECK(std::isfinite(x) && x > std::ldexp(1.0f, -96));
  }

  if (failures != 0) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all passed\n");
  return 0;
}
