// Standalone tuning probe for the Philox uniform kernel: sweeps
// elements-per-thread and grid size on a 4 GiB bf16 buffer.
// Build/run on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/rng_tune.hip -o /tmp/rng_tune && /tmp/rng_tune
// `rng_tune valu` runs the VALU-trim comparison of the normal kernel
// instead (profiles/normal_fill_valu.md).
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../torchdistx_amd/csrc/core/box_muller.h"

#define CHECK(x)                                            \
  do {                                                      \
    hipError_t e = (x);                                     \
    if (e != hipSuccess) {                                  \
      printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
      return 1;                                             \
    }                                                       \
  } while (0)

__device__ __forceinline__ uint2 mulhilo32(uint32_t a, uint32_t b) {
  uint2 r;
  r.x = a * b;
  r.y = __umulhi(a, b);
  return r;
}

__device__ __forceinline__ uint4 philox10(uint64_t seed, uint64_t subseq,
                                          uint64_t offset) {
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint4 c = make_uint4((uint32_t)offset, (uint32_t)(offset >> 32),
                       (uint32_t)subseq, (uint32_t)(subseq >> 32));
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint2 r0 = mulhilo32(kM0, c.x);
    uint2 r1 = mulhilo32(kM1, c.z);
    c = make_uint4(r1.y ^ c.y ^ k0, r1.x, r0.y ^ c.w ^ k1, r0.x);
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

// Round-count-parametrized Philox (7 rounds passes BigCrush per Salmon
// et al. 2011, Table 2; 10 is PyTorch's margin choice). Measures how much
// of the normal-kernel plateau is Philox VALU work.
template <int R>
__device__ __forceinline__ uint4 philoxR(uint64_t seed, uint64_t subseq,
                                         uint64_t offset) {
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint4 c = make_uint4((uint32_t)offset, (uint32_t)(offset >> 32),
                       (uint32_t)subseq, (uint32_t)(subseq >> 32));
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint2 r0 = mulhilo32(kM0, c.x);
    uint2 r1 = mulhilo32(kM1, c.z);
    c = make_uint4(r1.y ^ c.y ^ k0, r1.x, r0.y ^ c.w ^ k1, r0.x);
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

__device__ __forceinline__ float u2f(uint32_t x) {
  return (float)(x >> 8) * (1.0f / 16777216.0f);
}

struct alignas(16) V8 {
  __hip_bfloat16 v[8];
};

// EPT = elements per thread per grid-stride iteration (multiple of 8).
template <int EPT>
__global__ void rng_bf16(__hip_bfloat16* __restrict__ out, uint32_t n8,
                         float a, float b, uint64_t seed, uint64_t offset) {
  // n8 = number of 8-element groups; 32-bit indexing (n < 2^31 groups).
  constexpr int G = EPT / 8;  // 16B stores per iteration
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g0 = blockIdx.x * blockDim.x + threadIdx.x; g0 * G < n8;
       g0 += stride) {
#pragma unroll
    for (int s = 0; s < G; ++s) {
      uint32_t g = g0 * G + s;
      if (g >= n8) break;
      float vals[8];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        uint4 bits = philox10(seed, (uint64_t)g * 2 + c, offset);
        vals[c * 4 + 0] = fmaf(u2f(bits.x), b, a);
        vals[c * 4 + 1] = fmaf(u2f(bits.y), b, a);
        vals[c * 4 + 2] = fmaf(u2f(bits.z), b, a);
        vals[c * 4 + 3] = fmaf(u2f(bits.w), b, a);
      }
      V8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v.v[j] = __float2bfloat16(vals[j]);
      *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
    }
  }
}

// Contiguous-per-thread variant: thread handles G consecutive groups.
template <int G>
__global__ void rng_bf16_wide(__hip_bfloat16* __restrict__ out, uint32_t n8,
                              float a, float b, uint64_t seed,
                              uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t * G < n8;
       t += stride) {
    uint4 bits[2 * G];
#pragma unroll
    for (int c = 0; c < 2 * G; ++c) {
      uint32_t g = t * G + c / 2;
      bits[c] = philox10(seed, (uint64_t)g * 2 + (c & 1), offset);
    }
#pragma unroll
    for (int s = 0; s < G; ++s) {
      uint32_t g = t * G + s;
      if (g >= n8) break;
      V8 v;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        uint4 bb = bits[s * 2 + c];
        v.v[c * 4 + 0] = __float2bfloat16(fmaf(u2f(bb.x), b, a));
        v.v[c * 4 + 1] = __float2bfloat16(fmaf(u2f(bb.y), b, a));
        v.v[c * 4 + 2] = __float2bfloat16(fmaf(u2f(bb.z), b, a));
        v.v[c * 4 + 3] = __float2bfloat16(fmaf(u2f(bb.w), b, a));
      }
      *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
    }
  }
}

__device__ __forceinline__ float2 bm(float u1, float u2) {
  u1 = fmaxf(u1, 1.1754944e-38f);
  float r = sqrtf(-2.0f * __logf(u1));
  float sn, cs;
  __sincosf(6.2831853071795865f * u2, &sn, &cs);
  return make_float2(r * cs, r * sn);
}

// normal bf16: ONE philox -> 8 samples via 16-bit uniforms (kernel v2).
__global__ void normal_bf16_u16(__hip_bfloat16* __restrict__ out, uint32_t n8,
                                float a, float b, uint64_t seed,
                                uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philox10(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float2 nj = bm((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                     (float)(w[j] >> 16) * (1.0f / 65536.0f));
      v.v[j * 2 + 0] = __float2bfloat16(fmaf(nj.x, b, a));
      v.v[j * 2 + 1] = __float2bfloat16(fmaf(nj.y, b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

// Philox-round sweep of the shipped v2-log2 shape.
template <int R>
__global__ void normal_bf16_rounds(__hip_bfloat16* __restrict__ out,
                                   uint32_t n8, float a, float b,
                                   uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philoxR<R>(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float2 nj = bm((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                     (float)(w[j] >> 16) * (1.0f / 65536.0f));
      v.v[j * 2 + 0] = __float2bfloat16(fmaf(nj.x, b, a));
      v.v[j * 2 + 1] = __float2bfloat16(fmaf(nj.y, b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

template <int R>
__global__ void uniform_bf16_rounds(__hip_bfloat16* __restrict__ out,
                                    uint32_t n8, float a, float b,
                                    uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philoxR<R>(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v.v[j * 2 + 0] = __float2bfloat16(
          fmaf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f), b, a));
      v.v[j * 2 + 1] = __float2bfloat16(
          fmaf((float)(w[j] >> 16) * (1.0f / 65536.0f), b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

// normal bf16 with TWO philox and 24-bit uniforms (kernel v1 style).
__global__ void normal_bf16_u32(__hip_bfloat16* __restrict__ out, uint32_t n8,
                                float a, float b, uint64_t seed,
                                uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    V8 v;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint4 bits = philox10(seed, (uint64_t)g * 2 + c, offset);
      float2 n01 = bm(u2f(bits.x), u2f(bits.y));
      float2 n23 = bm(u2f(bits.z), u2f(bits.w));
      v.v[c * 4 + 0] = __float2bfloat16(fmaf(n01.x, b, a));
      v.v[c * 4 + 1] = __float2bfloat16(fmaf(n01.y, b, a));
      v.v[c * 4 + 2] = __float2bfloat16(fmaf(n23.x, b, a));
      v.v[c * 4 + 3] = __float2bfloat16(fmaf(n23.y, b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

// uniform bf16 v2: ONE philox -> 8 samples via 16-bit uniforms.
__global__ void uniform_bf16_u16(__hip_bfloat16* __restrict__ out,
                                 uint32_t n8, float a, float b, uint64_t seed,
                                 uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philox10(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v.v[j * 2 + 0] =
          __float2bfloat16(fmaf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f), b, a));
      v.v[j * 2 + 1] =
          __float2bfloat16(fmaf((float)(w[j] >> 16) * (1.0f / 65536.0f), b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

// ILP variant: two independent groups per iteration so the transcendental
// chains of two Box-Muller batches interleave.
__global__ void normal_bf16_u16x2(__hip_bfloat16* __restrict__ out,
                                  uint32_t n8, float a, float b,
                                  uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t half = (n8 + 1) / 2;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < half;
       t += stride) {
    uint32_t g0 = t;
    uint32_t g1 = t + half;
    uint4 b0 = philox10(seed, g0, offset);
    uint4 b1 = philox10(seed, g1, offset);
    uint32_t w0[4] = {b0.x, b0.y, b0.z, b0.w};
    uint32_t w1[4] = {b1.x, b1.y, b1.z, b1.w};
    V8 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float2 n0 = bm((float)(w0[j] & 0xffffu) * (1.0f / 65536.0f),
                     (float)(w0[j] >> 16) * (1.0f / 65536.0f));
      float2 n1 = bm((float)(w1[j] & 0xffffu) * (1.0f / 65536.0f),
                     (float)(w1[j] >> 16) * (1.0f / 65536.0f));
      v0.v[j * 2 + 0] = __float2bfloat16(fmaf(n0.x, b, a));
      v0.v[j * 2 + 1] = __float2bfloat16(fmaf(n0.y, b, a));
      v1.v[j * 2 + 0] = __float2bfloat16(fmaf(n1.x, b, a));
      v1.v[j * 2 + 1] = __float2bfloat16(fmaf(n1.y, b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g0 * 8) = v0;
    if (g1 < n8) {
      *reinterpret_cast<V8*>(out + (uint64_t)g1 * 8) = v1;
    }
  }
}

// Cheap-log variant: ln(u) for u = m * 2^-16 with integer m>=1 can be
// computed from the float bit pattern: ln(u) = (log2(m) - 16) * ln2, and
// log2(m) = exponent + log2(mantissa); v_log_f32 IS that — so instead try
// replacing sincos with a single sin via angle-sum identity? Keep simple:
// variant replacing __logf with __log2f * ln2 (same instr count, sanity).
__global__ void normal_bf16_log2(__hip_bfloat16* __restrict__ out,
                                 uint32_t n8, float a, float b,
                                 uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philox10(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float u1 = fmaxf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                       1.1754944e-38f);
      float r = sqrtf(-1.3862943611f * __log2f(u1));
      float sn, cs;
      __sincosf(6.2831853071795865f * ((float)(w[j] >> 16) * (1.0f / 65536.0f)),
                &sn, &cs);
      v.v[j * 2 + 0] = __float2bfloat16(fmaf(r * cs, b, a));
      v.v[j * 2 + 1] = __float2bfloat16(fmaf(r * sn, b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

// Split-phase x2: both philox results first, then all transcendental
// chains back-to-back so the scheduler can interleave them.
__global__ void normal_bf16_split2(__hip_bfloat16* __restrict__ out,
                                   uint32_t n8, float a, float b,
                                   uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t half = (n8 + 1) / 2;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < half;
       t += stride) {
    uint32_t g0 = t, g1 = t + half;
    uint4 b0 = philox10(seed, g0, offset);
    uint4 b1 = philox10(seed, g1, offset);
    uint32_t w[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    float r[8], sn[8], cs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float u1 = fmaxf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                       1.1754944e-38f);
      r[j] = sqrtf(-1.3862943611f * __log2f(u1));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __sincosf(6.2831853071795865f * ((float)(w[j] >> 16) * (1.0f / 65536.0f)),
                &sn[j], &cs[j]);
    }
    V8 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v0.v[j * 2 + 0] = __float2bfloat16(fmaf(r[j] * cs[j], b, a));
      v0.v[j * 2 + 1] = __float2bfloat16(fmaf(r[j] * sn[j], b, a));
      v1.v[j * 2 + 0] = __float2bfloat16(fmaf(r[4 + j] * cs[4 + j], b, a));
      v1.v[j * 2 + 1] = __float2bfloat16(fmaf(r[4 + j] * sn[4 + j], b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g0 * 8) = v0;
    if (g1 < n8) {
      *reinterpret_cast<V8*>(out + (uint64_t)g1 * 8) = v1;
    }
  }
}

// Combined candidate: rounds=7 Philox + log2 Box-Muller (the two wins
// measured separately in round 1, never together).
template <int R>
__global__ void normal_bf16_rlog2(__hip_bfloat16* __restrict__ out,
                                  uint32_t n8, float a, float b,
                                  uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philoxR<R>(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float u1 = fmaxf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                       1.1754944e-38f);
      float r = sqrtf(-1.3862943611f * __log2f(u1));
      float sn, cs;
      __sincosf(
          6.2831853071795865f * ((float)(w[j] >> 16) * (1.0f / 65536.0f)),
          &sn, &cs);
      v.v[j * 2 + 0] = __float2bfloat16(fmaf(r * cs, b, a));
      v.v[j * 2 + 1] = __float2bfloat16(fmaf(r * sn, b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

// r7 + log2 + split-phase x2 (transcendental chains of two groups
// back-to-back for ILP).
template <int R>
__global__ void normal_bf16_rsplit2(__hip_bfloat16* __restrict__ out,
                                    uint32_t n8, float a, float b,
                                    uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t half = (n8 + 1) / 2;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < half;
       t += stride) {
    uint32_t g0 = t, g1 = t + half;
    uint4 b0 = philoxR<R>(seed, g0, offset);
    uint4 b1 = philoxR<R>(seed, g1, offset);
    uint32_t w[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    float r[8], sn[8], cs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float u1 = fmaxf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                       1.1754944e-38f);
      r[j] = sqrtf(-1.3862943611f * __log2f(u1));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __sincosf(
          6.2831853071795865f * ((float)(w[j] >> 16) * (1.0f / 65536.0f)),
          &sn[j], &cs[j]);
    }
    V8 v0, v1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v0.v[j * 2 + 0] = __float2bfloat16(fmaf(r[j] * cs[j], b, a));
      v0.v[j * 2 + 1] = __float2bfloat16(fmaf(r[j] * sn[j], b, a));
      v1.v[j * 2 + 0] = __float2bfloat16(fmaf(r[4 + j] * cs[4 + j], b, a));
      v1.v[j * 2 + 1] = __float2bfloat16(fmaf(r[4 + j] * sn[4 + j], b, a));
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g0 * 8) = v0;
    if (g1 < n8) {
      *reinterpret_cast<V8*>(out + (uint64_t)g1 * 8) = v1;
    }
  }
}

// ---------------------------------------------------------------------------
// VALU-trim candidates for the shipped normal kernel (Philox-7 + log2
// Box-Muller), one flag per step so each is measured alone and all
// together (`rng_tune valu`, results in profiles/normal_fill_valu.md).
// Every step is meant to leave the output bits unchanged; the probe
// checks that with a checksum against the flag-free baseline.
// ---------------------------------------------------------------------------
constexpr int kMul64 = 1;  // one 64-bit product per Philox multiply
constexpr int kXor3 = 2;   // hi ^ c ^ k through the three-input bit-op
constexpr int kSqrt = 4;   // sqrt refinement without range scaling / class
constexpr int kFold = 8;   // cvt * 2^-16 * 2pi as one multiply

template <int F>
__device__ __forceinline__ uint2 mulhilo32_v(uint32_t a, uint32_t b) {
  if constexpr ((F & kMul64) != 0) {
    const uint64_t p = static_cast<uint64_t>(a) * b;
    return make_uint2(static_cast<uint32_t>(p),
                      static_cast<uint32_t>(p >> 32));
  } else {
    return mulhilo32(a, b);
  }
}

template <int F>
__device__ __forceinline__ uint32_t xor3_v(uint32_t a, uint32_t b,
                                           uint32_t c) {
  if constexpr ((F & kXor3) != 0) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
  } else {
    return a ^ b ^ c;
  }
}

template <int R, int F>
__device__ __forceinline__ uint4 philox_v(uint64_t seed, uint64_t subseq,
                                          uint64_t offset) {
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint4 c = make_uint4((uint32_t)offset, (uint32_t)(offset >> 32),
                       (uint32_t)subseq, (uint32_t)(subseq >> 32));
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint2 r0 = mulhilo32_v<F>(kM0, c.x);
    uint2 r1 = mulhilo32_v<F>(kM1, c.z);
    c = make_uint4(xor3_v<F>(r1.y, c.y, k0), r1.x, xor3_v<F>(r0.y, c.w, k1),
                   r0.x);
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

// The product's sqrt_box_muller: v_sqrt_f32 plus the shared +-1 ulp
// fix-up, x and the two residuals pinned in registers so the multiplies
// and fmas are not paired into packed fp32 instructions.
__device__ __forceinline__ float pin_vgpr(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ float sqrt_refined(float x) {
  x = pin_vgpr(x);
  return tdx::box_muller::sqrt_fixup(__builtin_amdgcn_sqrtf(x), x,
                                     [](float v) { return pin_vgpr(v); });
}

template <int F>
__global__ void normal_bf16_valu(__hip_bfloat16* __restrict__ out,
                                 uint32_t n8, float a, float b,
                                 uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philox_v<7, F>(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float u1 = fmaxf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f),
                       1.1754944e-38f);
      const float x = tdx::box_muller::kNeg2Ln2 * __log2f(u1);
      float r;
      if constexpr ((F & kSqrt) != 0) {
        r = sqrt_refined(x);
      } else {
        r = sqrtf(x);
      }
      float angle;
      if constexpr ((F & kFold) != 0) {
        angle = (float)(w[j] >> 16) * tdx::box_muller::kAngleScale16;
      } else {
        angle = 6.2831853071795865f * ((float)(w[j] >> 16) * (1.0f / 65536.0f));
      }
      float sn, cs;
      __sincosf(angle, &sn, &cs);
      float v0 = fmaf(r * cs, b, a);
      float v1 = fmaf(r * sn, b, a);
      // Same rounding pin as from_float() in init_kernels.hip.
      asm volatile("" : "+v"(v0));
      asm volatile("" : "+v"(v1));
      v.v[j * 2 + 0] = __float2bfloat16(v0);
      v.v[j * 2 + 1] = __float2bfloat16(v1);
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

template <int F>
__global__ void uniform_bf16_valu(__hip_bfloat16* __restrict__ out,
                                  uint32_t n8, float a, float b,
                                  uint64_t seed, uint64_t offset) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n8;
       g += stride) {
    uint4 bits = philox_v<10, F>(seed, g, offset);
    uint32_t w[4] = {bits.x, bits.y, bits.z, bits.w};
    V8 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v0 = fmaf((float)(w[j] & 0xffffu) * (1.0f / 65536.0f), b, a);
      float v1 = fmaf((float)(w[j] >> 16) * (1.0f / 65536.0f), b, a);
      asm volatile("" : "+v"(v0));
      asm volatile("" : "+v"(v1));
      v.v[j * 2 + 0] = __float2bfloat16(v0);
      v.v[j * 2 + 1] = __float2bfloat16(v1);
    }
    *reinterpret_cast<V8*>(out + (uint64_t)g * 8) = v;
  }
}

__global__ void zero_u64(unsigned long long* p) { *p = 0; }

// Order-sensitive 64-bit checksum of the buffer's 32-bit words.
__global__ void checksum_words(const uint32_t* __restrict__ in, uint64_t n,
                               unsigned long long* __restrict__ acc) {
  unsigned long long s = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    s += (unsigned long long)in[i] * (2ull * i + 1ull);
  }
  atomicAdd(acc, s);
}

template <typename K>
double benchB(K kernel, __hip_bfloat16* buf, uint32_t n8, int blocks,
              int iters, int threads) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  kernel<<<blocks, threads>>>(buf, n8, -1.f, 2.f, 42, 4);  // warm
  hipDeviceSynchronize();
  hipEventRecord(e0);
  for (int i = 0; i < iters; ++i) {
    kernel<<<blocks, threads>>>(buf, n8, -1.f, 2.f, 42, 4);
  }
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  double bytes = (double)n8 * 16.0 * iters;
  return bytes / (ms / 1e3) / 1e12;  // TB/s
}

template <typename K>
double bench(K kernel, __hip_bfloat16* buf, uint32_t n8, int blocks,
             int iters) {
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  kernel<<<blocks, 256>>>(buf, n8, -1.f, 2.f, 42, 4);  // warm
  hipDeviceSynchronize();
  hipEventRecord(e0);
  for (int i = 0; i < iters; ++i) {
    kernel<<<blocks, 256>>>(buf, n8, -1.f, 2.f, 42, 4);
  }
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  double bytes = (double)n8 * 16.0 * iters;
  return bytes / (ms / 1e3) / 1e12;  // TB/s
}

using TuneKernel = void (*)(__hip_bfloat16*, uint32_t, float, float, uint64_t,
                            uint64_t);
struct Variant {
  const char* name;
  TuneKernel kernel;
  int base;  // index of the variant whose bits this one must reproduce
};

// `rng_tune valu`: every candidate against the baseline, alternating
// inside one process at the product's launch shape (16384 x 256).
int run_valu(__hip_bfloat16* buf, uint32_t n8) {
  constexpr int kAll = kMul64 | kXor3 | kSqrt | kFold;
  const Variant variants[] = {
      {"normal  baseline (r7+log2)", normal_bf16_valu<0>, 0},
      {"normal  +mul64", normal_bf16_valu<kMul64>, 0},
      {"normal  +xor3", normal_bf16_valu<kXor3>, 0},
      {"normal  +sqrt", normal_bf16_valu<kSqrt>, 0},
      {"normal  +fold", normal_bf16_valu<kFold>, 0},
      {"normal  +sqrt+fold", normal_bf16_valu<kSqrt | kFold>, 0},
      {"normal  +sqrt+fold+mul64", normal_bf16_valu<kSqrt | kFold | kMul64>,
       0},
      {"normal  +sqrt+fold+xor3", normal_bf16_valu<kSqrt | kFold | kXor3>, 0},
      {"normal  all four", normal_bf16_valu<kAll>, 0},
      {"uniform baseline (r10)", uniform_bf16_valu<0>, 9},
      {"uniform +mul64", uniform_bf16_valu<kMul64>, 9},
      {"uniform +xor3", uniform_bf16_valu<kXor3>, 9},
      {"uniform +mul64+xor3", uniform_bf16_valu<kMul64 | kXor3>, 9},
  };
  constexpr int kN = sizeof(variants) / sizeof(variants[0]);
  constexpr int kReps = 9, kIters = 10, kBlocks = 16384;

  unsigned long long* acc;
  CHECK(hipMalloc(&acc, sizeof(*acc) * kN));
  unsigned long long sums[kN];
  for (int i = 0; i < kN; ++i) {
    zero_u64<<<1, 1>>>(acc + i);
    // mean 0, std 1: the transform's bits reach the bf16 output unscaled.
    variants[i].kernel<<<kBlocks, 256>>>(buf, n8, 0.0f, 1.0f, 42, 4);
    checksum_words<<<4096, 256>>>(reinterpret_cast<const uint32_t*>(buf),
                                  (uint64_t)n8 * 4, acc + i);
  }
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(sums, acc, sizeof(sums), hipMemcpyDeviceToHost));

  // Warm the clocks (profiles/dvfs_ramp_note.md) before the first timing.
  for (int i = 0; i < 200; ++i) {
    variants[0].kernel<<<kBlocks, 256>>>(buf, n8, 0.25f, 0.02f, 42, 4);
  }
  CHECK(hipDeviceSynchronize());

  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  static double tbps[kN][kReps];
  for (int rep = 0; rep < kReps; ++rep) {
    for (int i = 0; i < kN; ++i) {
      CHECK(hipEventRecord(e0));
      for (int it = 0; it < kIters; ++it) {
        variants[i].kernel<<<kBlocks, 256>>>(buf, n8, 0.25f, 0.02f, 42, 4);
      }
      CHECK(hipEventRecord(e1));
      CHECK(hipEventSynchronize(e1));
      float ms;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      tbps[i][rep] = (double)n8 * 16.0 * kIters / (ms / 1e3) / 1e12;
    }
  }
  printf("%-30s %8s %8s %8s  %s\n", "variant", "median", "min", "max",
         "bits vs baseline");
  for (int i = 0; i < kN; ++i) {
    double* t = tbps[i];
    for (int x = 1; x < kReps; ++x) {
      for (int y = x; y > 0 && t[y - 1] > t[y]; --y) {
        double tmp = t[y];
        t[y] = t[y - 1];
        t[y - 1] = tmp;
      }
    }
    printf("%-30s %8.3f %8.3f %8.3f  %s (%016llx)\n", variants[i].name,
           t[kReps / 2], t[0], t[kReps - 1],
           sums[i] == sums[variants[i].base] ? "same" : "DIFFERENT", sums[i]);
  }
  CHECK(hipFree(acc));
  return 0;
}

int main(int argc, char** argv) {
  const uint64_t bytes = 4ull << 30;
  const uint32_t n8 = (uint32_t)(bytes / 16);
  __hip_bfloat16* buf;
  CHECK(hipMalloc(&buf, bytes));

  if (argc > 1 && strcmp(argv[1], "valu") == 0) {
    int rc = run_valu(buf, n8);
    hipFree(buf);
    return rc;
  }

  for (int blocks : {4096, 8192, 16384}) {
    printf("blocks=%d\n", blocks);
    printf("  uniform 2xphilox (v1): %.2f TB/s\n", bench(rng_bf16<8>, buf, n8, blocks, 5));
    printf("  uniform 1xphilox (v2): %.2f TB/s\n", bench(uniform_bf16_u16, buf, n8, blocks, 5));
    printf("  normal  2xphilox (v1): %.2f TB/s\n", bench(normal_bf16_u32, buf, n8, blocks, 5));
    printf("  normal  1xphilox (v2): %.2f TB/s\n", bench(normal_bf16_u16, buf, n8, blocks, 5));
    printf("  normal  v2 ILPx2     : %.2f TB/s\n", bench(normal_bf16_u16x2, buf, n8, blocks, 5));
    printf("  normal  v2 log2      : %.2f TB/s\n", bench(normal_bf16_log2, buf, n8, blocks, 5));
    printf("  normal  split2 t256  : %.2f TB/s\n", benchB(normal_bf16_split2, buf, n8, blocks, 5, 256));
    printf("  normal  split2 t512  : %.2f TB/s\n", benchB(normal_bf16_split2, buf, n8, blocks/2, 5, 512));
    printf("  normal  log2 t512    : %.2f TB/s\n", benchB(normal_bf16_log2, buf, n8, blocks/2, 5, 512));
    printf("  normal  log2 t128    : %.2f TB/s\n", benchB(normal_bf16_log2, buf, n8, blocks*2, 5, 128));
    printf("  normal  rounds=10    : %.2f TB/s\n", bench(normal_bf16_rounds<10>, buf, n8, blocks, 5));
    printf("  normal  rounds=7     : %.2f TB/s\n", bench(normal_bf16_rounds<7>, buf, n8, blocks, 5));
    printf("  uniform rounds=10    : %.2f TB/s\n", bench(uniform_bf16_rounds<10>, buf, n8, blocks, 5));
    printf("  uniform rounds=7     : %.2f TB/s\n", bench(uniform_bf16_rounds<7>, buf, n8, blocks, 5));
    printf("  normal  r7+log2      : %.2f TB/s\n", bench(normal_bf16_rlog2<7>, buf, n8, blocks, 5));
    printf("  normal  r7+log2 t512 : %.2f TB/s\n", benchB(normal_bf16_rlog2<7>, buf, n8, blocks/2, 5, 512));
    printf("  normal  r7+split2    : %.2f TB/s\n", bench(normal_bf16_rsplit2<7>, buf, n8, blocks, 5));
    printf("  normal  r7+split2 512: %.2f TB/s\n", benchB(normal_bf16_rsplit2<7>, buf, n8, blocks/2, 5, 512));
  }
  // memset reference ceiling
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  hipEventRecord(e0);
  for (int i = 0; i < 5; ++i) hipMemsetAsync(buf, 0, bytes);
  hipEventRecord(e1);
  hipEventSynchronize(e1);
  float ms;
  hipEventElapsedTime(&ms, e0, e1);
  printf("hipMemset      : %.2f TB/s\n", (double)bytes * 5 / (ms / 1e3) / 1e12);
  hipFree(buf);
  return 0;
}
