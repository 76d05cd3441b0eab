// CDNA4 (gfx950) parameter-init kernels for tape replay into HBM3E.
//
// These are the hand-written HIP kernels behind the ops the deferred-init
// tape records for standard module construction:
// uniform_ / normal_ (counter-based Philox4x32: 10 rounds for uniforms,
// 7 for the VALU-bound normals — see philoxN below), fill_ and zero_.
// They register as the `tdx::` op namespace; the deferred-init replay
// engine redirects the recorded aten:: init ops to them when the target
// tensor lives on the GPU (csrc/core/native_redirect.cc).
//
// Design (per the CDNA4 kernel playbook for memory-bound elementwise ops):
//  * 256-thread blocks (4 wave64s), grid-stride loops capped at 16384
//    blocks (measured sweet spot for this ALU-heavy streaming shape;
//    see kMaxBlocks below);
//  * every store is 16 bytes per lane (float4 / 8 x bf16) — 1 KiB per wave
//    per instruction, the HBM coalescing sweet spot; scalar tail only for
//    the last partial group;
//  * counter-based Philox keyed on (seed, element-group) so any slice of a
//    tensor can be generated independently and reproducibly — this is what
//    makes sharded materialization embarrassingly parallel across ranks;
//  * no LDS: the kernels are pure streaming writes, so tiles would add
//    nothing (LDS is for reuse, of which there is none).

#include <hip/hip_runtime.h>

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/HIPGeneratorImpl.h>
#include <torch/library.h>

#include <cstdlib>
#include <limits>
#include <type_traits>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "../core/box_geometry.h"

namespace tdx {
namespace {

constexpr int kBlock = 256;
// Measured on gfx950 (scripts/rng_tune.hip): this ALU-heavy streaming
// kernel keeps improving past the usual ~2048-block guideline — at 16384
// blocks the one-philox-per-store uniform kernel reaches ~5.5 TB/s on a
// 4 GiB bf16 fill (pure-store ceiling: 6.4 TB/s via hipMemset; the
// Philox-7 + log2-Box-Muller normals are VALU-bound at ~3.5 TB/s once
// clocks are warm — profiles/dvfs_ramp_note.md).
constexpr int kMaxBlocks = 16384;

// ---------------------------------------------------------------------------
// Philox4x32-10 (standard constants), producing 4 x uint32 per invocation.
// Kept in sync with the CPU reference in csrc/core/philox.h (identical
// constants and integer pipeline).
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint2 mulhilo32(uint32_t a, uint32_t b) {
  uint2 r;
  r.x = a * b;
  r.y = __umulhi(a, b);
  return r;
}

// Round-count-templated Philox4x32, kept in sync with the CPU reference
// in csrc/core/philox.h. Uniforms use the standard 10 rounds (the kernel
// is store-bound, extra rounds are free); normals use 7 — Philox4x32-7
// passes the full BigCrush battery (Salmon et al., SC'11, Table 2) and
// the transcendental-heavy normal kernel is VALU-bound, where the saved
// rounds are a measured ~13% fill-rate win (profiles/rng_tune_r7.log).
template <int kRounds>
__device__ __forceinline__ uint4 philoxN(uint64_t seed,
                                         uint64_t subsequence,
                                         uint64_t offset) {
  constexpr uint32_t kW0 = 0x9E3779B9u;
  constexpr uint32_t kW1 = 0xBB67AE85u;
  constexpr uint32_t kM0 = 0xD2511F53u;
  constexpr uint32_t kM1 = 0xCD9E8D57u;

  uint32_t k0 = static_cast<uint32_t>(seed);
  uint32_t k1 = static_cast<uint32_t>(seed >> 32);
  uint4 c = make_uint4(static_cast<uint32_t>(offset),
                       static_cast<uint32_t>(offset >> 32),
                       static_cast<uint32_t>(subsequence),
                       static_cast<uint32_t>(subsequence >> 32));
#pragma unroll
  for (int round = 0; round < kRounds; ++round) {
    uint2 r0 = mulhilo32(kM0, c.x);
    uint2 r1 = mulhilo32(kM1, c.z);
    c = make_uint4(r1.y ^ c.y ^ k0, r1.x, r0.y ^ c.w ^ k1, r0.x);
    k0 += kW0;
    k1 += kW1;
  }
  return c;
}

// uint32 -> [0, 1) float with a 24-bit mantissa (matches the resolution of
// PyTorch's uniform transformation).
__device__ __forceinline__ float u32_to_uniform(uint32_t x) {
  return static_cast<float>(x >> 8) * (1.0f / 16777216.0f);
}

// uint16 -> [0, 1) float. For 16-bit output dtypes (8-bit bf16 / 11-bit
// fp16 mantissas) 16 random bits per sample are ample, and they halve the
// Philox work per byte: one philox10 call yields a full 16-byte store.
__device__ __forceinline__ float u16_to_uniform(uint32_t x) {
  return static_cast<float>(x & 0xffffu) * (1.0f / 65536.0f);
}

// Two uniforms -> two standard normals (Box-Muller). -2*ln(u) is computed
// as -2*ln2*log2(u): __log2f maps straight to v_log_f32, measurably
// faster than __logf's wrapper (2.69 -> 3.15 TB/s on the bf16 normal
// kernel, scripts/rng_tune.hip).
__device__ __forceinline__ float2 box_muller(float u1, float u2) {
  // Guard u1 away from 0 so log stays finite.
  u1 = fmaxf(u1, 1.1754944e-38f);
  float r = sqrtf(-1.3862943611198906f * __log2f(u1));
  float s, c;
  __sincosf(6.2831853071795865f * u2, &s, &c);
  return make_float2(r * c, r * s);
}

template <typename T>
__device__ __forceinline__ T from_float(float v) {
  // Pin the f32 rounding step: without this barrier the compiler fuses
  // fma+convert into v_fma_mixlo_f16 (ONE rounding, straight to fp16)
  // in some loop shapes but not others, so the same element's bits
  // depended on which code path (vectorized main loop vs elementwise
  // boundary) stored it — a 1-ulp fp16 divergence that broke the
  // slice/full bitwise invariant (caught by the 40k-seed GPU slice
  // fuzz). bf16/f32 paths never fused; the barrier costs one cvt that
  // was already in the unfused schedule.
  asm volatile("" : "+v"(v));
  if constexpr (std::is_same_v<T, __hip_bfloat16>) {
    return __float2bfloat16(v);
  } else if constexpr (std::is_same_v<T, __half>) {
    return __float2half(v);
  } else {
    return v;
  }
}

// Elements per thread-group-iteration: 16-bit types pack 8 elements into
// one 16-byte store; 32-bit types pack 4 — one philox10 per store either
// way (16-bit dtypes draw 16 random bits per sample).
template <typename T>
struct VecTraits;
template <>
struct VecTraits<float> {
  static constexpr int kElems = 4;
  using Vec = float4;
};
template <>
struct VecTraits<__hip_bfloat16> {
  static constexpr int kElems = 8;
  struct alignas(16) Vec {
    __hip_bfloat16 v[8];
  };
};
template <>
struct VecTraits<__half> {
  static constexpr int kElems = 8;
  struct alignas(16) Vec {
    __half v[8];
  };
};

enum class Dist { kUniform, kNormal, kBernoulli };

// Computes the VecTraits<T>::kElems values of element group `g` — ONE
// philox10 with counter = the 16-byte group index turned into 4 fp32
// samples (24-bit uniforms) or 8 bf16/fp16 samples (16-bit uniforms,
// matched to the output mantissa). Shared by the full-tensor and the
// shard kernels so a shard is bitwise a slice of the full tensor.
template <typename T, Dist kDist>
__device__ __forceinline__ void rngGroupValues(uint64_t g,
                                               float a,
                                               float b,
                                               uint64_t seed,
                                               uint64_t offset,
                                               float* vals) {
  uint4 bits = kDist == Dist::kNormal ? philoxN<7>(seed, g, offset)
                                      : philoxN<10>(seed, g, offset);
  if constexpr (VecTraits<T>::kElems == 4) {
    float u[4] = {u32_to_uniform(bits.x), u32_to_uniform(bits.y),
                  u32_to_uniform(bits.z), u32_to_uniform(bits.w)};
    if constexpr (kDist == Dist::kUniform) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vals[j] = fmaf(u[j], b, a);
      }
    } else if constexpr (kDist == Dist::kBernoulli) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vals[j] = u[j] < a ? 1.0f : 0.0f;
      }
    } else {
      float2 n01 = box_muller(u[0], u[1]);
      float2 n23 = box_muller(u[2], u[3]);
      vals[0] = fmaf(n01.x, b, a);
      vals[1] = fmaf(n01.y, b, a);
      vals[2] = fmaf(n23.x, b, a);
      vals[3] = fmaf(n23.y, b, a);
    }
  } else {
    uint32_t words[4] = {bits.x, bits.y, bits.z, bits.w};
    if constexpr (kDist == Dist::kUniform) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vals[j * 2 + 0] = fmaf(u16_to_uniform(words[j]), b, a);
        vals[j * 2 + 1] = fmaf(u16_to_uniform(words[j] >> 16), b, a);
      }
    } else if constexpr (kDist == Dist::kBernoulli) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vals[j * 2 + 0] = u16_to_uniform(words[j]) < a ? 1.0f : 0.0f;
        vals[j * 2 + 1] = u16_to_uniform(words[j] >> 16) < a ? 1.0f : 0.0f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float2 nj = box_muller(u16_to_uniform(words[j]),
                               u16_to_uniform(words[j] >> 16));
        vals[j * 2 + 0] = fmaf(nj.x, b, a);
        vals[j * 2 + 1] = fmaf(nj.y, b, a);
      }
    }
  }
}

// Indexed by GROUP, not element: full 16-byte groups take the branchless
// main loop (no per-iteration tail compare — worth ~10% on the
// VALU-bound normal kernel), the single partial tail group is handled by
// one thread. Group counts stay 32-bit up to 2^31 groups (= 32 GiB of
// bf16), so real tensors never pay 64-bit loop arithmetic.
template <typename T, Dist kDist, typename IdxT>
__global__ void rng_kernel(T* __restrict__ out,
                           IdxT n_full_groups,
                           uint32_t tail_elems,
                           float a,
                           float b,
                           uint64_t seed,
                           uint64_t offset) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;

  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  for (IdxT g = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
       g < n_full_groups; g += stride) {
    float vals[kElems];
    rngGroupValues<T, kDist>(static_cast<uint64_t>(g), a, b, seed, offset,
                             vals);
    Vec v;
    T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
    for (int j = 0; j < kElems; ++j) {
      vp[j] = from_float<T>(vals[j]);
    }
    *reinterpret_cast<Vec*>(out + static_cast<uint64_t>(g) * kElems) = v;
  }
  if (tail_elems != 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t g = n_full_groups;
    float vals[kElems];
    rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
    for (uint32_t j = 0; j < tail_elems; ++j) {
      out[g * kElems + j] = from_float<T>(vals[j]);
    }
  }
}

template <typename T>
__global__ void fill_kernel(T* __restrict__ out, int64_t n, float value_f) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;

  const int64_t n_groups = (n + kElems - 1) / kElems;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;

  const T value = from_float<T>(value_f);
  Vec v;
  T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
  for (int j = 0; j < kElems; ++j) {
    vp[j] = value;
  }

  for (int64_t g = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
       g < n_groups; g += stride) {
    const int64_t base = g * kElems;
    if (base + kElems <= n) {
      *reinterpret_cast<Vec*>(out + base) = v;
    } else {
      for (int64_t j = 0; base + j < n; ++j) {
        out[base + j] = value;
      }
    }
  }
}

int numBlocks(int64_t n_groups) {
  int64_t blocks = (n_groups + kBlock - 1) / kBlock;
  return static_cast<int>(std::min<int64_t>(blocks, kMaxBlocks));
}

// Reserves a Philox offset window on the generator; 4 counters per launch
// is enough because the per-element-group subsequence already separates
// streams within a launch.
uint64_t acquireSeedOffset(const std::optional<at::Generator>& generator,
                           uint64_t* seed) {
  auto gen = at::get_generator_or_default<at::CUDAGeneratorImpl>(
      generator, at::cuda::detail::getDefaultCUDAGenerator());
  std::lock_guard<std::mutex> lock(gen->mutex_);
  auto state = gen->philox_engine_inputs(4);
  *seed = state.first;
  return state.second;
}

template <Dist kDist>
void launchRng(at::Tensor& self,
               double p0,
               double p1,
               const std::optional<at::Generator>& generator,
               std::optional<int64_t> pinned_seed,
               std::optional<int64_t> pinned_offset) {
  TORCH_CHECK(self.is_contiguous(),
              "tdx init kernels require contiguous tensors");
  const int64_t n = self.numel();
  if (n == 0) {
    return;
  }
  uint64_t seed = 0;
  uint64_t offset = 0;
  if (pinned_seed.has_value() && pinned_offset.has_value()) {
    // Replay with record-time-pinned Philox state: the result is the same
    // no matter which rank replays this op, or in what order.
    seed = static_cast<uint64_t>(*pinned_seed);
    offset = static_cast<uint64_t>(*pinned_offset);
  } else {
    offset = acquireSeedOffset(generator, &seed);
  }
  auto stream = at::cuda::getCurrentCUDAStream();

  // p0/p1 are (from, to) for uniform, (mean, std) for normal, and
  // (p, unused) for bernoulli; uniform/normal apply a + b * sample,
  // bernoulli thresholds the raw uniform against a.
  float a = static_cast<float>(p0);
  float b = kDist == Dist::kUniform ? static_cast<float>(p1 - p0)
                                    : static_cast<float>(p1);

  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    constexpr int kElems = VecTraits<T>::kElems;
    const int64_t n_full = n / kElems;
    const uint32_t tail = static_cast<uint32_t>(n % kElems);
    const int64_t n_groups = n_full + (tail != 0 ? 1 : 0);
    if (n_full <= std::numeric_limits<uint32_t>::max() / 2) {
      hipLaunchKernelGGL((rng_kernel<T, kDist, uint32_t>),
                         dim3(numBlocks(n_groups)), dim3(kBlock), 0,
                         stream.stream(),
                         reinterpret_cast<T*>(self.data_ptr()),
                         static_cast<uint32_t>(n_full), tail, a, b, seed,
                         offset);
    } else {
      hipLaunchKernelGGL((rng_kernel<T, kDist, uint64_t>),
                         dim3(numBlocks(n_groups)), dim3(kBlock), 0,
                         stream.stream(),
                         reinterpret_cast<T*>(self.data_ptr()),
                         static_cast<uint64_t>(n_full), tail, a, b, seed,
                         offset);
    }
    C10_HIP_KERNEL_LAUNCH_CHECK();
  };
  switch (self.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    case at::kHalf:
      launch(__half{});
      break;
    default:
      TORCH_CHECK(false, "tdx RNG init kernels support float32/bf16/fp16, ",
                  "got ", self.scalar_type());
  }
}

at::Tensor& tdx_uniform_(at::Tensor& self,
                         double from,
                         double to,
                         std::optional<at::Generator> generator,
                         std::optional<int64_t> seed,
                         std::optional<int64_t> offset) {
  // double (and other unsupported dtypes) never reach here: the redirect
  // layer filters, and direct callers get a clear dispatch error.
  launchRng<Dist::kUniform>(self, from, to, generator, seed, offset);
  return self;
}

at::Tensor& tdx_normal_(at::Tensor& self,
                        double mean,
                        double std,
                        std::optional<at::Generator> generator,
                        std::optional<int64_t> seed,
                        std::optional<int64_t> offset) {
  TORCH_CHECK(std >= 0.0, "normal_ expects std >= 0.0, but found std=", std);
  launchRng<Dist::kNormal>(self, mean, std, generator, seed, offset);
  return self;
}

// Shard kernel: writes elements [start, end) of the virtual full tensor
// into out[0 .. end-start). Interior groups use full 16-byte stores;
// boundary groups store elementwise.
template <typename T, Dist kDist>
__global__ void rng_shard_kernel(T* __restrict__ out,
                                 int64_t start,
                                 int64_t end,
                                 float a,
                                 float b,
                                 uint64_t seed,
                                 uint64_t offset) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;

  const int64_t g_first = start / kElems;
  const int64_t g_last = (end + kElems - 1) / kElems;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  // The vector path stores Vec packs at out + (base - start); base is a
  // multiple of kElems, so the destination is 16-byte aligned only when
  // `start` is too. Unaligned shards (odd row sizes) store elementwise.
  const bool vec_aligned = (start % kElems) == 0;

  if (vec_aligned) {
    // Branchless main loop over the full interior groups (aligned start
    // means there is no partial head group); the single partial tail
    // group is handled by one thread below.
    const int64_t g_int_hi = end / kElems;
    for (int64_t g = g_first +
             blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
         g < g_int_hi; g += stride) {
      float vals[kElems];
      rngGroupValues<T, kDist>(static_cast<uint64_t>(g), a, b, seed,
                               offset, vals);
      Vec v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int j = 0; j < kElems; ++j) {
        vp[j] = from_float<T>(vals[j]);
      }
      *reinterpret_cast<Vec*>(out + (g * kElems - start)) = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && end % kElems != 0 &&
        g_int_hi >= g_first) {
      float vals[kElems];
      rngGroupValues<T, kDist>(static_cast<uint64_t>(g_int_hi), a, b, seed,
                               offset, vals);
      const int64_t base = g_int_hi * kElems;
      for (int64_t e = base > start ? base : start; e < end; ++e) {
        out[e - start] = from_float<T>(vals[e - base]);
      }
    }
    return;
  }

  for (int64_t g = g_first +
           blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x;
       g < g_last; g += stride) {
    float vals[kElems];
    rngGroupValues<T, kDist>(static_cast<uint64_t>(g), a, b, seed, offset,
                             vals);
    const int64_t base = g * kElems;
    const int64_t lo = base > start ? base : start;
    const int64_t hi = base + kElems < end ? base + kElems : end;
    for (int64_t e = lo; e < hi; ++e) {
      out[e - start] = from_float<T>(vals[e - base]);
    }
  }
}

template <Dist kDist>
void launchRngShard(at::Tensor& shard,
                    int64_t start,
                    int64_t end,
                    double p0,
                    double p1,
                    int64_t seed,
                    int64_t offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx shard kernels require contiguous tensors");
  TORCH_CHECK(shard.numel() == end - start,
              "shard numel must equal end - start");
  if (shard.numel() == 0) {
    return;
  }
  float a = static_cast<float>(p0);
  float b = kDist == Dist::kUniform ? static_cast<float>(p1 - p0)
                                    : static_cast<float>(p1);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    const int64_t n_groups =
        (end + VecTraits<T>::kElems - 1) / VecTraits<T>::kElems -
        start / VecTraits<T>::kElems;
    hipLaunchKernelGGL((rng_shard_kernel<T, kDist>),
                       dim3(numBlocks(n_groups)), dim3(kBlock), 0,
                       stream.stream(),
                       reinterpret_cast<T*>(shard.data_ptr()), start, end, a,
                       b, static_cast<uint64_t>(seed),
                       static_cast<uint64_t>(offset));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    case at::kHalf:
      launch(__half{});
      break;
    default:
      TORCH_CHECK(false, "tdx shard kernels support float32/bf16/fp16, got ",
                  shard.scalar_type());
  }
}

at::Tensor& tdx_uniform_shard_(at::Tensor& shard, int64_t start, int64_t end,
                               double from, double to, int64_t seed,
                               int64_t offset) {
  launchRngShard<Dist::kUniform>(shard, start, end, from, to, seed, offset);
  return shard;
}

at::Tensor& tdx_normal_shard_(at::Tensor& shard, int64_t start, int64_t end,
                              double mean, double std, int64_t seed,
                              int64_t offset) {
  TORCH_CHECK(std >= 0.0, "normal_ expects std >= 0.0, but found std=", std);
  launchRngShard<Dist::kNormal>(shard, start, end, mean, std, seed, offset);
  return shard;
}

at::Tensor& tdx_bernoulli_(at::Tensor& self,
                           double p,
                           std::optional<at::Generator> generator,
                           std::optional<int64_t> seed,
                           std::optional<int64_t> offset) {
  TORCH_CHECK(0.0 <= p && p <= 1.0,
              "bernoulli_ expects 0 <= p <= 1, but found p=", p);
  launchRng<Dist::kBernoulli>(self, p, 0.0, generator, seed, offset);
  return self;
}

at::Tensor& tdx_bernoulli_shard_(at::Tensor& shard, int64_t start,
                                 int64_t end, double p, int64_t seed,
                                 int64_t offset) {
  TORCH_CHECK(0.0 <= p && p <= 1.0,
              "bernoulli_ expects 0 <= p <= 1, but found p=", p);
  launchRngShard<Dist::kBernoulli>(shard, start, end, p, 0.0, seed, offset);
  return shard;
}

// Windowed shard kernel: materializes `full.narrow(dim, s, len)` of a
// contiguous virtual full tensor for any dim — the slice is n_blocks
// contiguous global ranges of block_len elements, block r starting at
// global element g_off + r * g_stride (dim 0 is the n_blocks == 1
// special case, served by rng_shard_kernel above). Shard flat index i
// maps to global element
//   g(i) = g_off + (i / block_len) * g_stride + (i % block_len),
// and the value of global element g is lane g % kElems of Philox group
// g / kElems — identical to the full-tensor kernel, so any-dim slices
// are bitwise sub-tensors of the full materialization. When g_off,
// block_len and g_stride are all group-multiples (the common case:
// trailing dims of transformer weights are multiples of 8) every group
// of the window is whole and the destination is 16-byte aligned, so the
// fast path is group-indexed with vector stores like the flat kernel;
// odd geometries store elementwise.
// IdxT is the SHARD-side loop index type: 32-bit up to 2^31 shard
// groups/elements (the flat-kernel design rule — real shards never pay
// 64-bit divides, the one VALU-expensive op here); only the GLOBAL
// group id widens to 64-bit, with a multiply, not a divide.
template <typename T, Dist kDist, typename IdxT>
__global__ void rng_shard_window_kernel(T* __restrict__ out,
                                        IdxT n_blocks,
                                        IdxT block_len,
                                        int64_t g_stride,
                                        int64_t g_off,
                                        float a,
                                        float b,
                                        uint64_t seed,
                                        uint64_t offset) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;
  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  const bool vec_aligned = (g_off % kElems) == 0 &&
                           (block_len % kElems) == 0 &&
                           (g_stride % kElems) == 0;
  if (vec_aligned) {
    const IdxT gpb = block_len / kElems;  // groups per window block
    const IdxT n_groups = n_blocks * gpb;
    const uint64_t g0 = static_cast<uint64_t>(g_off) / kElems;
    const uint64_t gs = static_cast<uint64_t>(g_stride) / kElems;
    for (IdxT j = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
         j < n_groups; j += stride) {
      const IdxT blk = j / gpb;
      const IdxT within = j - blk * gpb;
      const uint64_t g = g0 + static_cast<uint64_t>(blk) * gs + within;
      float vals[kElems];
      rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
      Vec v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        vp[e] = from_float<T>(vals[e]);
      }
      *reinterpret_cast<Vec*>(out + static_cast<uint64_t>(j) * kElems) = v;
    }
    return;
  }
  const IdxT n = n_blocks * block_len;
  for (IdxT i = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
       i < n; i += stride) {
    const IdxT blk = i / block_len;
    const IdxT rem = i - blk * block_len;
    const uint64_t ge = static_cast<uint64_t>(g_off) +
                        static_cast<uint64_t>(blk) * g_stride + rem;
    const uint64_t g = ge / kElems;
    float vals[kElems];
    rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
    out[i] = from_float<T>(vals[ge - g * kElems]);
  }
}

template <Dist kDist>
void launchRngShardWindow(at::Tensor& shard, int64_t n_blocks,
                          int64_t block_len, int64_t g_stride, int64_t g_off,
                          double p0, double p1, int64_t seed,
                          int64_t offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx shard kernels require contiguous tensors");
  TORCH_CHECK(n_blocks >= 0 && block_len >= 0 && g_stride >= block_len &&
                  g_off >= 0,
              "invalid shard window");
  TORCH_CHECK(shard.numel() == n_blocks * block_len,
              "shard numel must equal n_blocks * block_len");
  if (shard.numel() == 0) {
    return;
  }
  float a = static_cast<float>(p0);
  float b = kDist == Dist::kUniform ? static_cast<float>(p1 - p0)
                                    : static_cast<float>(p1);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    const int64_t n_work =
        (shard.numel() + VecTraits<T>::kElems - 1) / VecTraits<T>::kElems;
    auto launch_idx = [&](auto idx_tag) {
      using IdxT = decltype(idx_tag);
      hipLaunchKernelGGL((rng_shard_window_kernel<T, kDist, IdxT>),
                         dim3(numBlocks(n_work)), dim3(kBlock), 0,
                         stream.stream(),
                         reinterpret_cast<T*>(shard.data_ptr()),
                         static_cast<IdxT>(n_blocks),
                         static_cast<IdxT>(block_len), g_stride, g_off, a,
                         b, static_cast<uint64_t>(seed),
                         static_cast<uint64_t>(offset));
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (shard.numel() <= std::numeric_limits<int32_t>::max()) {
      launch_idx(uint32_t{});
    } else {
      launch_idx(int64_t{});
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    case at::kHalf:
      launch(__half{});
      break;
    default:
      TORCH_CHECK(false, "tdx shard kernels support float32/bf16/fp16, got ",
                  shard.scalar_type());
  }
}

at::Tensor& tdx_uniform_shard_win_(at::Tensor& shard, int64_t n_blocks,
                                   int64_t block_len, int64_t g_stride,
                                   int64_t g_off, double from, double to,
                                   int64_t seed, int64_t offset) {
  launchRngShardWindow<Dist::kUniform>(shard, n_blocks, block_len, g_stride,
                                       g_off, from, to, seed, offset);
  return shard;
}

at::Tensor& tdx_normal_shard_win_(at::Tensor& shard, int64_t n_blocks,
                                  int64_t block_len, int64_t g_stride,
                                  int64_t g_off, double mean, double std,
                                  int64_t seed, int64_t offset) {
  TORCH_CHECK(std >= 0.0, "normal_ expects std >= 0.0, but found std=", std);
  launchRngShardWindow<Dist::kNormal>(shard, n_blocks, block_len, g_stride,
                                      g_off, mean, std, seed, offset);
  return shard;
}

at::Tensor& tdx_bernoulli_shard_win_(at::Tensor& shard, int64_t n_blocks,
                                     int64_t block_len, int64_t g_stride,
                                     int64_t g_off, double p, int64_t seed,
                                     int64_t offset) {
  TORCH_CHECK(0.0 <= p && p <= 1.0,
              "bernoulli_ expects 0 <= p <= 1, but found p=", p);
  launchRngShardWindow<Dist::kBernoulli>(shard, n_blocks, block_len, g_stride,
                                         g_off, p, 0.0, seed, offset);
  return shard;
}

// ---------------------------------------------------------------------------
// Fused init chains: an RNG value step followed by a recorded tail of
// pointwise-scalar ops (trunc_normal_ is uniform_ -> erfinv_ -> mul_ ->
// add_ -> clamp_) in ONE kernel. Unfused, every tail op is an ATen kernel
// that reads and writes the whole tensor; here the tail runs on the
// values in registers before the single store. The result is bitwise
// what the separate kernels give (applyTail below spells out why).
// ---------------------------------------------------------------------------

constexpr int kMaxTail = 8;

// Opcodes: TailOp::Code in csrc/core/deferred_init.h.
enum TailCode : int32_t {
  kTailErfinv = 0,
  kTailMul = 1,
  kTailAdd = 2,
  kTailSub = 3,
  kTailClamp = 4,
  kTailClampMin = 5,
  kTailClampMax = 6,
  kTailNeg = 7,
  kTailAbs = 8,
};

struct TailStep {
  int32_t op;
  float s0;
  float s1;
};

// Passed by value as a kernel argument (or read from the batched blob):
// uniform across the grid, so the opcode switch is a scalar branch.
struct TailProgram {
  // f16 tensors only: elements of the full tensor from this index on get
  // their mul results rounded once (tailMul below).
  uint64_t once_from;
  int32_t n;
  TailStep steps[kMaxTail];
};

// ATen's vectorized elementwise kernel works in blocks of this many
// elements for 2-byte dtypes on ROCm (256 threads x 8); the block that
// holds the last numel % kAtenBlock16 elements takes another code path.
constexpr int64_t kAtenBlock16 = 2048;

// What ATen leaves in memory between two kernels: the value rounded to T.
template <typename T>
__device__ __forceinline__ float roundThrough(float v) {
  if constexpr (std::is_same_v<T, __hip_bfloat16>) {
    return __bfloat162float(from_float<T>(v));
  } else if constexpr (std::is_same_v<T, __half>) {
    return __half2float(from_float<T>(v));
  } else {
    return from_float<T>(v);
  }
}

// A tensor element times a float immediate, rounded the way ATen's kernel
// rounds it. That is the float product followed by the store's rounding
// to T — except on f16 tensors in ATen's last, partial block, whose
// multiply-and-narrow compiles to a mixed-precision FMA that rounds the
// exact product to f16 ONCE (measured on gfx950: every element of the
// last numel % 2048, and no other, equals the once-rounded product;
// add/sub round twice everywhere, and bf16 has no such instruction).
// The f16 x f32 product is exact in double, and double -> f16 rounds
// once.
template <typename T>
__device__ __forceinline__ float tailMul(float v, float s, bool once) {
  if constexpr (std::is_same_v<T, __half>) {
    if (once) {
      const double r = static_cast<double>(v) * static_cast<double>(s);
      return static_cast<float>(static_cast<_Float16>(r));
    }
  }
  return __fmul_rn(v, s);
}

// Applies the tail to one group's values, reproducing the bits of the
// separate ATen kernels:
//  * the value is rounded to T after the RNG step and after every tail
//    step (ATen stores T between kernels), and each step computes in
//    float on the widened value (ATen's opmath_t);
//  * contraction is off in this function: hipcc would otherwise turn
//    mul -> add on an f32 tensor into one FMA, which ATen cannot do
//    across kernels;
//  * clamp keeps NaN and otherwise takes min(max(v, lo), hi), ATen's
//    scalar clamp order;
//  * erfinv is the device library's erfinvf on the widened value.
//  * mul on f16 tensors follows ATen's position-dependent rounding
//    (tailMul); `elem0` is the index of vals[0] in the full tensor.
// Measured on gfx950 this matches ATen on every element except for
// erfinv on f32 tensors, which the planner therefore admits only on
// explicit request (tailOpAdmitted in csrc/core/deferred_init.cc):
// ATen's f32 kernel is 1-2 ulp away on about half of all inputs, and an
// f64 erfinv would cost scratch and half the occupancy.
template <typename T, int kElems>
__device__ __forceinline__ void applyTail(float (&vals)[kElems],
                                          const TailProgram& prog,
                                          uint64_t elem0) {
#pragma clang fp contract(off)
  const uint64_t once_from = prog.once_from;
#pragma unroll
  for (int j = 0; j < kElems; ++j) {
    vals[j] = roundThrough<T>(vals[j]);
  }
  for (int s = 0; s < prog.n; ++s) {
    const int32_t op = prog.steps[s].op;
    const float s0 = prog.steps[s].s0;
    const float s1 = prog.steps[s].s1;
    switch (op) {
      case kTailErfinv:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          vals[j] = roundThrough<T>(erfinvf(vals[j]));
        }
        break;
      case kTailMul:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          vals[j] = roundThrough<T>(
              tailMul<T>(vals[j], s0, elem0 + j >= once_from));
        }
        break;
      case kTailAdd:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          vals[j] = roundThrough<T>(__fadd_rn(vals[j], s0));
        }
        break;
      case kTailSub:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          vals[j] = roundThrough<T>(__fsub_rn(vals[j], s0));
        }
        break;
      case kTailClamp:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          const float v = vals[j];
          vals[j] = roundThrough<T>(v != v ? v : fminf(fmaxf(v, s0), s1));
        }
        break;
      case kTailClampMin:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          const float v = vals[j];
          vals[j] = roundThrough<T>(v != v ? v : fmaxf(v, s0));
        }
        break;
      case kTailClampMax:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          const float v = vals[j];
          vals[j] = roundThrough<T>(v != v ? v : fminf(v, s0));
        }
        break;
      case kTailNeg:
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          vals[j] = roundThrough<T>(-vals[j]);
        }
        break;
      default:  // kTailAbs; the host validates opcodes
#pragma unroll
        for (int j = 0; j < kElems; ++j) {
          vals[j] = roundThrough<T>(fabsf(vals[j]));
        }
        break;
    }
  }
}

// rng_shard_window_kernel with the tail applied before the store. Same
// window geometry and index-width rule. The group-indexed vector path
// additionally serves a single block (n_blocks == 1, the whole-tensor and
// flat dim-0 case) whose length is not a group multiple: its one partial
// last group is stored elementwise by one thread. `vec_ok` is the host's
// check that `out` is 16-byte aligned.
template <typename T, Dist kDist, typename IdxT>
__global__ void rng_chain_window_kernel(T* __restrict__ out,
                                        IdxT n_blocks,
                                        IdxT block_len,
                                        int64_t g_stride,
                                        int64_t g_off,
                                        bool vec_ok,
                                        float a,
                                        float b,
                                        uint64_t seed,
                                        uint64_t offset,
                                        TailProgram prog) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;
  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  const bool vec_aligned =
      vec_ok && (g_off % kElems) == 0 &&
      (n_blocks == 1 ||
       ((block_len % kElems) == 0 && (g_stride % kElems) == 0));
  if (vec_aligned) {
    const IdxT gpb = block_len / kElems;  // full groups per window block
    const IdxT n_groups = n_blocks * gpb;
    const uint64_t g0 = static_cast<uint64_t>(g_off) / kElems;
    const uint64_t gs = static_cast<uint64_t>(g_stride) / kElems;
    for (IdxT j = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
         j < n_groups; j += stride) {
      const IdxT blk = j / gpb;
      const IdxT within = j - blk * gpb;
      const uint64_t g = g0 + static_cast<uint64_t>(blk) * gs + within;
      float vals[kElems];
      rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
      applyTail<T, kElems>(vals, prog, g * kElems);
      Vec v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        vp[e] = from_float<T>(vals[e]);
      }
      *reinterpret_cast<Vec*>(out + static_cast<uint64_t>(j) * kElems) = v;
    }
    // Only a single block can have a partial last group here.
    const uint32_t tail_elems =
        static_cast<uint32_t>(block_len - gpb * kElems);
    if (tail_elems != 0 && blockIdx.x == 0 && threadIdx.x == 0) {
      float vals[kElems];
      rngGroupValues<T, kDist>(g0 + gpb, a, b, seed, offset, vals);
      applyTail<T, kElems>(vals, prog, (g0 + gpb) * kElems);
      for (uint32_t e = 0; e < tail_elems; ++e) {
        out[static_cast<uint64_t>(gpb) * kElems + e] = from_float<T>(vals[e]);
      }
    }
    return;
  }
  const IdxT n = n_blocks * block_len;
  for (IdxT i = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
       i < n; i += stride) {
    const IdxT blk = i / block_len;
    const IdxT rem = i - blk * block_len;
    const uint64_t ge = static_cast<uint64_t>(g_off) +
                        static_cast<uint64_t>(blk) * g_stride + rem;
    const uint64_t g = ge / kElems;
    float vals[kElems];
    rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
    applyTail<T, kElems>(vals, prog, g * kElems);
    out[i] = from_float<T>(vals[ge - g * kElems]);
  }
}

// `full_numel` is the element count of the FULL tensor the values belong
// to (a shard passes its parent's): it places ATen's last, partial block.
TailProgram makeTailProgram(at::IntArrayRef tail_ops,
                            at::ArrayRef<double> tail_s0,
                            at::ArrayRef<double> tail_s1,
                            int64_t full_numel) {
  TORCH_CHECK(tail_ops.size() <= static_cast<size_t>(kMaxTail) &&
                  tail_s0.size() == tail_ops.size() &&
                  tail_s1.size() == tail_ops.size(),
              "rng_chain: at most ", kMaxTail,
              " tail ops, with one s0 and one s1 each");
  TORCH_CHECK(full_numel >= 0, "rng_chain: full_numel must be >= 0");
  TailProgram prog{};
  prog.once_from =
      static_cast<uint64_t>(full_numel / kAtenBlock16 * kAtenBlock16);
  prog.n = static_cast<int32_t>(tail_ops.size());
  for (size_t i = 0; i < tail_ops.size(); ++i) {
    TORCH_CHECK(kTailErfinv <= tail_ops[i] && tail_ops[i] <= kTailAbs,
                "rng_chain: bad tail opcode ", tail_ops[i]);
    prog.steps[i].op = static_cast<int32_t>(tail_ops[i]);
    // double -> float, the way ATen narrows a scalar operand to opmath_t.
    prog.steps[i].s0 = static_cast<float>(tail_s0[i]);
    prog.steps[i].s1 = static_cast<float>(tail_s1[i]);
  }
  return prog;
}

template <Dist kDist>
void launchRngChainWindow(at::Tensor& shard, int64_t n_blocks,
                          int64_t block_len, int64_t g_stride, int64_t g_off,
                          double p0, double p1, const TailProgram& prog,
                          int64_t seed, int64_t offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx shard kernels require contiguous tensors");
  TORCH_CHECK(n_blocks >= 0 && block_len >= 0 && g_stride >= block_len &&
                  g_off >= 0,
              "invalid shard window");
  TORCH_CHECK(shard.numel() == n_blocks * block_len,
              "shard numel must equal n_blocks * block_len");
  if (shard.numel() == 0) {
    return;
  }
  float a = static_cast<float>(p0);
  float b = kDist == Dist::kUniform ? static_cast<float>(p1 - p0)
                                    : static_cast<float>(p1);
  const bool vec_ok =
      reinterpret_cast<uintptr_t>(shard.data_ptr()) % 16 == 0;
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    const int64_t n_work =
        (shard.numel() + VecTraits<T>::kElems - 1) / VecTraits<T>::kElems;
    auto launch_idx = [&](auto idx_tag) {
      using IdxT = decltype(idx_tag);
      hipLaunchKernelGGL((rng_chain_window_kernel<T, kDist, IdxT>),
                         dim3(numBlocks(n_work)), dim3(kBlock), 0,
                         stream.stream(),
                         reinterpret_cast<T*>(shard.data_ptr()),
                         static_cast<IdxT>(n_blocks),
                         static_cast<IdxT>(block_len), g_stride, g_off,
                         vec_ok, a, b, static_cast<uint64_t>(seed),
                         static_cast<uint64_t>(offset), prog);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (shard.numel() <= std::numeric_limits<int32_t>::max()) {
      launch_idx(uint32_t{});
    } else {
      launch_idx(int64_t{});
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    case at::kHalf:
      launch(__half{});
      break;
    default:
      TORCH_CHECK(false, "tdx chain kernels support float32/bf16/fp16, got ",
                  shard.scalar_type());
  }
}

at::Tensor& tdx_rng_chain_shard_win_(
    at::Tensor& shard, int64_t n_blocks, int64_t block_len, int64_t g_stride,
    int64_t g_off, int64_t dist, double p0, double p1,
    at::IntArrayRef tail_ops, at::ArrayRef<double> tail_s0,
    at::ArrayRef<double> tail_s1, int64_t full_numel, int64_t seed,
    int64_t offset) {
  TORCH_CHECK(full_numel >= g_off + (n_blocks > 0 ? (n_blocks - 1) * g_stride
                                                  + block_len : 0),
              "rng_chain: the window does not fit in full_numel");
  const TailProgram prog =
      makeTailProgram(tail_ops, tail_s0, tail_s1, full_numel);
  switch (dist) {
    case 0:
      launchRngChainWindow<Dist::kUniform>(shard, n_blocks, block_len,
                                           g_stride, g_off, p0, p1, prog,
                                           seed, offset);
      break;
    case 1:
      TORCH_CHECK(p1 >= 0.0, "normal_ expects std >= 0.0, but found std=",
                  p1);
      launchRngChainWindow<Dist::kNormal>(shard, n_blocks, block_len,
                                          g_stride, g_off, p0, p1, prog,
                                          seed, offset);
      break;
    case 2:
      TORCH_CHECK(0.0 <= p0 && p0 <= 1.0,
                  "bernoulli_ expects 0 <= p <= 1, but found p=", p0);
      launchRngChainWindow<Dist::kBernoulli>(shard, n_blocks, block_len,
                                             g_stride, g_off, p0, 0.0, prog,
                                             seed, offset);
      break;
    default:
      TORCH_CHECK(false, "rng_chain: dist must be 0 (uniform), 1 (normal) "
                         "or 2 (bernoulli), got ", dist);
  }
  return shard;
}

at::Tensor& tdx_rng_chain_(at::Tensor& self, int64_t dist, double p0,
                           double p1, at::IntArrayRef tail_ops,
                           at::ArrayRef<double> tail_s0,
                           at::ArrayRef<double> tail_s1, int64_t seed,
                           int64_t offset) {
  return tdx_rng_chain_shard_win_(self, 1, self.numel(), self.numel(), 0,
                                  dist, p0, p1, tail_ops, tail_s0, tail_s1,
                                  self.numel(), seed, offset);
}

// ---------------------------------------------------------------------------
// Chains that end in a dtype conversion (`empty(..).normal_().to(bf16)`,
// `Module.to(dtype)` inside the builder): the values are drawn, rounded and
// run through the tail at the SOURCE dtype TSrc, exactly as
// rng_chain_window_kernel<TSrc> computes them, and stored as TDst — one
// launch and one store per element, instead of a TSrc tensor written, read
// back and converted.
//
// The two dtypes differ, so at least one is 16-bit and the work unit is 8
// elements whichever side that is:
//   * f32 source: TWO consecutive Philox groups (2u, 2u + 1) of 4 values
//     each make one 16-byte store;
//   * 16-bit source, f32 destination: one group, 32 bytes, two 16-byte
//     stores;
//   * bf16 <-> f16: one group, one 16-byte store.
// ---------------------------------------------------------------------------

constexpr int kCastUnit = 8;

// The 8 final (float) values of global unit `u`: elements [8u, 8u + 8) of
// the full tensor, after the tail, as TSrc holds them.
template <typename TSrc, Dist kDist>
__device__ __forceinline__ void castUnitValues(uint64_t u, float a, float b,
                                               uint64_t seed, uint64_t offset,
                                               const TailProgram& prog,
                                               float (&vals)[kCastUnit]) {
  constexpr int kSrcElems = VecTraits<TSrc>::kElems;
  if constexpr (kSrcElems == kCastUnit) {
    rngGroupValues<TSrc, kDist>(u, a, b, seed, offset, vals);
    applyTail<TSrc, kCastUnit>(vals, prog, u * kCastUnit);
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float half_vals[kSrcElems];
      const uint64_t g = 2 * u + h;
      rngGroupValues<TSrc, kDist>(g, a, b, seed, offset, half_vals);
      applyTail<TSrc, kSrcElems>(half_vals, prog, g * kSrcElems);
#pragma unroll
      for (int e = 0; e < kSrcElems; ++e) {
        vals[h * kSrcElems + e] = half_vals[e];
      }
    }
  }
}

// One element by its global index, for the paths that store elementwise.
// It draws the element's whole source group and runs the whole tail to
// keep one value, as rng_chain_window_kernel's elementwise path does: 4x
// (f32 source) or 8x the RNG and tail work of the vector path per stored
// element. That is the price of every window with an odd geometry, a
// misaligned destination or g_off % 8 == 4; it has not been measured.
template <typename TSrc, typename TDst, Dist kDist>
__device__ __forceinline__ TDst castElementValue(uint64_t ge, float a,
                                                 float b, uint64_t seed,
                                                 uint64_t offset,
                                                 const TailProgram& prog) {
  constexpr int kSrcElems = VecTraits<TSrc>::kElems;
  const uint64_t g = ge / kSrcElems;
  float vals[kSrcElems];
  rngGroupValues<TSrc, kDist>(g, a, b, seed, offset, vals);
  applyTail<TSrc, kSrcElems>(vals, prog, g * kSrcElems);
  // A select chain, not vals[lane]: a run-time index would put the array
  // in scratch.
  const uint32_t lane = static_cast<uint32_t>(ge - g * kSrcElems);
  float v = vals[0];
#pragma unroll
  for (int e = 1; e < kSrcElems; ++e) {
    v = lane == static_cast<uint32_t>(e) ? vals[e] : v;
  }
  return from_float<TDst>(v);
}

// The first `n` (1..7) elements of global unit `u`, stored elementwise at
// `p`: the one partial last unit of a single block or of a tensor.
template <typename TSrc, typename TDst, Dist kDist>
__device__ __forceinline__ void storePartialCastUnit(
    TDst* __restrict__ p, uint32_t n, uint64_t u, float a, float b,
    uint64_t seed, uint64_t offset, const TailProgram& prog) {
  float vals[kCastUnit];
  castUnitValues<TSrc, kDist>(u, a, b, seed, offset, prog, vals);
#pragma unroll
  for (int e = 0; e < kCastUnit - 1; ++e) {
    if (static_cast<uint32_t>(e) < n) {
      p[e] = from_float<TDst>(vals[e]);
    }
  }
}

// Stores the finished unit at `p` (16-byte aligned): one 16-byte store for
// a 16-bit destination, two for f32.
template <typename TDst>
__device__ __forceinline__ void storeCastUnit(TDst* __restrict__ p,
                                              const float (&vals)[kCastUnit]) {
  if constexpr (std::is_same_v<TDst, float>) {
    float4 lo, hi;
    lo.x = from_float<float>(vals[0]);
    lo.y = from_float<float>(vals[1]);
    lo.z = from_float<float>(vals[2]);
    lo.w = from_float<float>(vals[3]);
    hi.x = from_float<float>(vals[4]);
    hi.y = from_float<float>(vals[5]);
    hi.z = from_float<float>(vals[6]);
    hi.w = from_float<float>(vals[7]);
    reinterpret_cast<float4*>(p)[0] = lo;
    reinterpret_cast<float4*>(p)[1] = hi;
  } else {
    typename VecTraits<TDst>::Vec v;
    TDst* vp = reinterpret_cast<TDst*>(&v);
#pragma unroll
    for (int e = 0; e < kCastUnit; ++e) {
      vp[e] = from_float<TDst>(vals[e]);
    }
    *reinterpret_cast<typename VecTraits<TDst>::Vec*>(p) = v;
  }
}

// The vector loop shared by the window and the batched kernel: this thread
// takes shard units j0, j0 + stride, ... below n_units; unit j is stored at
// out + 8 j and holds global unit gunit(j). The block is 1-d with a
// multiple of 64 threads and j0 - lane is a multiple of 64, so the 64
// lanes of a wave always hold 64 consecutive shard units (a "chunk").
//
// f32 destination: a lane's unit is 32 bytes, and two plain 16-byte stores
// per lane would each touch every other 16 bytes of 2 KiB. While a whole
// chunk lies below n_units (a wave-uniform test, so all 64 lanes are
// active) the lanes pair up instead: lane 2k takes unit k of the chunk,
// lane 2k + 1 unit 32 + k, the pair swaps one half each (even lane: its
// upper half for the odd lane's lower half), and then the first store of
// the wave writes units 0..31 of the chunk and the second units 32..63 —
// lane l at byte 16 l of a contiguous 1 KiB both times. The values do not
// depend on which lane computes them.
template <typename TSrc, typename TDst, Dist kDist, typename IdxT,
          typename GlobalUnitFn>
__device__ __forceinline__ void castUnitLoop(TDst* __restrict__ out, IdxT j0,
                                             IdxT n_units, IdxT stride,
                                             GlobalUnitFn gunit, float a,
                                             float b, uint64_t seed,
                                             uint64_t offset,
                                             const TailProgram& prog) {
  const uint32_t lane = threadIdx.x & 63u;
  for (IdxT j = j0; j < n_units; j += stride) {
    float vals[kCastUnit];
    if constexpr (std::is_same_v<TDst, float>) {
      const IdxT chunk = j - static_cast<IdxT>(lane);
      if (chunk + 64 <= n_units) {
        const uint32_t odd = lane & 1u;
        const IdxT mine = chunk + static_cast<IdxT>((lane >> 1) + (odd << 5));
        castUnitValues<TSrc, kDist>(gunit(mine), a, b, seed, offset, prog,
                                    vals);
        float4 first, second;
        float give[4], got[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // Two values, then the choice: `odd ? vals[e] : vals[4 + e]` is
          // an lvalue, i.e. a run-time address into vals, i.e. scratch.
          const float lower = vals[e];
          const float upper = vals[4 + e];
          give[e] = from_float<float>(odd ? lower : upper);
          got[e] = __shfl_xor(give[e], 1);
        }
        // Even lane: its unit's lower half, then the odd lane's unit's
        // lower half. Odd lane: the even lane's unit's upper half, then
        // its own unit's upper half.
        first.x = odd ? got[0] : from_float<float>(vals[0]);
        first.y = odd ? got[1] : from_float<float>(vals[1]);
        first.z = odd ? got[2] : from_float<float>(vals[2]);
        first.w = odd ? got[3] : from_float<float>(vals[3]);
        second.x = odd ? from_float<float>(vals[4]) : got[0];
        second.y = odd ? from_float<float>(vals[5]) : got[1];
        second.z = odd ? from_float<float>(vals[6]) : got[2];
        second.w = odd ? from_float<float>(vals[7]) : got[3];
        float* p = out +
                   (static_cast<uint64_t>(chunk) + (lane >> 1)) * kCastUnit +
                   odd * 4;
        *reinterpret_cast<float4*>(p) = first;
        *reinterpret_cast<float4*>(p + 32 * kCastUnit) = second;
        continue;
      }
    }
    castUnitValues<TSrc, kDist>(gunit(j), a, b, seed, offset, prog, vals);
    storeCastUnit<TDst>(out + static_cast<uint64_t>(j) * kCastUnit, vals);
  }
}

// rng_chain_window_kernel's geometry and index-width rule with the unit in
// place of the source group. The vector path needs the UNIT whole and
// aligned: `vec_ok` (the host's check that `out` is 16-byte aligned),
// g_off % 8 == 0, and a single block or block_len and g_stride both
// multiples of 8.
// NB g_off % 8 == 4 with an f32 source: the window starts on a source
// GROUP boundary (4 elements), so rng_chain_window_kernel<float> would
// vectorize it — but a unit would then straddle global units (the second
// group of one and the first of the next) and its 16-byte destination
// store pairs up differently. It takes the elementwise path here, like
// every other g_off that is not a unit multiple.
// A single block whose length is no unit multiple stores its one partial
// last unit elementwise from one thread; with an f32 source that unit may
// span a full group and a partial one, so storePartialCastUnit draws the
// whole unit (both groups) and stores its first elements.
template <typename TSrc, typename TDst, Dist kDist, typename IdxT>
__global__ void rng_chain_cast_window_kernel(TDst* __restrict__ out,
                                             IdxT n_blocks,
                                             IdxT block_len,
                                             int64_t g_stride,
                                             int64_t g_off,
                                             bool vec_ok,
                                             float a,
                                             float b,
                                             uint64_t seed,
                                             uint64_t offset,
                                             TailProgram prog) {
  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  const IdxT tid = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
  const bool vec_aligned =
      vec_ok && (g_off % kCastUnit) == 0 &&
      (n_blocks == 1 ||
       ((block_len % kCastUnit) == 0 && (g_stride % kCastUnit) == 0));
  if (vec_aligned) {
    const IdxT upb = block_len / kCastUnit;  // full units per window block
    const IdxT n_units = n_blocks * upb;
    const uint64_t u0 = static_cast<uint64_t>(g_off) / kCastUnit;
    const uint64_t us = static_cast<uint64_t>(g_stride) / kCastUnit;
    castUnitLoop<TSrc, TDst, kDist, IdxT>(
        out, tid, n_units, stride,
        [=](IdxT j) -> uint64_t {
          const IdxT blk = j / upb;
          const IdxT within = j - blk * upb;
          return u0 + static_cast<uint64_t>(blk) * us + within;
        },
        a, b, seed, offset, prog);
    // Only a single block can have a partial last unit here.
    const uint32_t tail_elems =
        static_cast<uint32_t>(block_len - upb * kCastUnit);
    if (tail_elems != 0 && blockIdx.x == 0 && threadIdx.x == 0) {
      storePartialCastUnit<TSrc, TDst, kDist>(
          out + static_cast<uint64_t>(upb) * kCastUnit, tail_elems, u0 + upb,
          a, b, seed, offset, prog);
    }
    return;
  }
  const IdxT n = n_blocks * block_len;
  for (IdxT i = tid; i < n; i += stride) {
    const IdxT blk = i / block_len;
    const IdxT rem = i - blk * block_len;
    const uint64_t ge = static_cast<uint64_t>(g_off) +
                        static_cast<uint64_t>(blk) * g_stride + rem;
    out[i] = castElementValue<TSrc, TDst, kDist>(ge, a, b, seed, offset,
                                                 prog);
  }
}

int castDtypeCode(c10::ScalarType t) {
  switch (t) {
    case at::kFloat:
      return 0;
    case at::kBFloat16:
      return 1;
    case at::kHalf:
      return 2;
    default:
      return -1;
  }
}

// Calls f(TSrc{}, TDst{}) for the pair of two DIFFERENT dtype codes.
template <typename F>
void dispatchCastPair(int src, int dst, F&& f) {
  switch (src * 3 + dst) {
    case 0 * 3 + 1:
      f(float{}, __hip_bfloat16{});
      break;
    case 0 * 3 + 2:
      f(float{}, __half{});
      break;
    case 1 * 3 + 0:
      f(__hip_bfloat16{}, float{});
      break;
    case 1 * 3 + 2:
      f(__hip_bfloat16{}, __half{});
      break;
    case 2 * 3 + 0:
      f(__half{}, float{});
      break;
    case 2 * 3 + 1:
      f(__half{}, __hip_bfloat16{});
      break;
    default:
      TORCH_CHECK(false, "rng_chain_cast: two different dtypes of "
                         "float32/bf16/fp16 are required");
  }
}

template <Dist kDist>
void launchRngChainCastWindow(at::Tensor& shard, c10::ScalarType src_dtype,
                              int64_t n_blocks, int64_t block_len,
                              int64_t g_stride, int64_t g_off, double p0,
                              double p1, const TailProgram& prog,
                              int64_t seed, int64_t offset) {
  float a = static_cast<float>(p0);
  float b = kDist == Dist::kUniform ? static_cast<float>(p1 - p0)
                                    : static_cast<float>(p1);
  const bool vec_ok =
      reinterpret_cast<uintptr_t>(shard.data_ptr()) % 16 == 0;
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t n_work = (shard.numel() + kCastUnit - 1) / kCastUnit;
  dispatchCastPair(
      castDtypeCode(src_dtype), castDtypeCode(shard.scalar_type()),
      [&](auto src_tag, auto dst_tag) {
        using TSrc = decltype(src_tag);
        using TDst = decltype(dst_tag);
        auto launch_idx = [&](auto idx_tag) {
          using IdxT = decltype(idx_tag);
          hipLaunchKernelGGL(
              (rng_chain_cast_window_kernel<TSrc, TDst, kDist, IdxT>),
              dim3(numBlocks(n_work)), dim3(kBlock), 0, stream.stream(),
              reinterpret_cast<TDst*>(shard.data_ptr()),
              static_cast<IdxT>(n_blocks), static_cast<IdxT>(block_len),
              g_stride, g_off, vec_ok, a, b, static_cast<uint64_t>(seed),
              static_cast<uint64_t>(offset), prog);
          C10_HIP_KERNEL_LAUNCH_CHECK();
        };
        if (shard.numel() <= std::numeric_limits<int32_t>::max()) {
          launch_idx(uint32_t{});
        } else {
          launch_idx(int64_t{});
        }
      });
}

at::Tensor& tdx_rng_chain_cast_shard_win_(
    at::Tensor& shard, at::ScalarType src_dtype, int64_t n_blocks,
    int64_t block_len, int64_t g_stride, int64_t g_off, int64_t dist,
    double p0, double p1, at::IntArrayRef tail_ops,
    at::ArrayRef<double> tail_s0, at::ArrayRef<double> tail_s1,
    int64_t full_numel, int64_t seed, int64_t offset) {
  TORCH_CHECK(castDtypeCode(src_dtype) >= 0 &&
                  castDtypeCode(shard.scalar_type()) >= 0 &&
                  src_dtype != shard.scalar_type(),
              "rng_chain_cast: two different dtypes of float32/bf16/fp16, "
              "got ", src_dtype, " -> ", shard.scalar_type());
  TORCH_CHECK(shard.is_contiguous(),
              "tdx shard kernels require contiguous tensors");
  TORCH_CHECK(n_blocks >= 0 && block_len >= 0 && g_stride >= block_len &&
                  g_off >= 0,
              "invalid shard window");
  TORCH_CHECK(shard.numel() == n_blocks * block_len,
              "shard numel must equal n_blocks * block_len");
  TORCH_CHECK(full_numel >= g_off + (n_blocks > 0 ? (n_blocks - 1) * g_stride
                                                  + block_len : 0),
              "rng_chain: the window does not fit in full_numel");
  const TailProgram prog =
      makeTailProgram(tail_ops, tail_s0, tail_s1, full_numel);
  TORCH_CHECK(0 <= dist && dist <= 2,
              "rng_chain: dist must be 0 (uniform), 1 (normal) or 2 "
              "(bernoulli), got ", dist);
  TORCH_CHECK(dist != 1 || p1 >= 0.0,
              "normal_ expects std >= 0.0, but found std=", p1);
  TORCH_CHECK(dist != 2 || (0.0 <= p0 && p0 <= 1.0),
              "bernoulli_ expects 0 <= p <= 1, but found p=", p0);
  if (shard.numel() == 0) {
    return shard;
  }
  switch (dist) {
    case 0:
      launchRngChainCastWindow<Dist::kUniform>(shard, src_dtype, n_blocks,
                                               block_len, g_stride, g_off,
                                               p0, p1, prog, seed, offset);
      break;
    case 1:
      launchRngChainCastWindow<Dist::kNormal>(shard, src_dtype, n_blocks,
                                              block_len, g_stride, g_off, p0,
                                              p1, prog, seed, offset);
      break;
    default:
      launchRngChainCastWindow<Dist::kBernoulli>(shard, src_dtype, n_blocks,
                                                 block_len, g_stride, g_off,
                                                 p0, 0.0, prog, seed, offset);
      break;
  }
  return shard;
}

at::Tensor& tdx_rng_chain_cast_(at::Tensor& self, at::ScalarType src_dtype,
                                int64_t dist, double p0, double p1,
                                at::IntArrayRef tail_ops,
                                at::ArrayRef<double> tail_s0,
                                at::ArrayRef<double> tail_s1, int64_t seed,
                                int64_t offset) {
  return tdx_rng_chain_cast_shard_win_(self, src_dtype, 1, self.numel(),
                                       self.numel(), 0, dist, p0, p1,
                                       tail_ops, tail_s0, tail_s1,
                                       self.numel(), seed, offset);
}

// ---------------------------------------------------------------------------
// N-d box kernel: materializes full[lo_0:hi_0, ..., lo_{r-1}:hi_{r-1}] of a
// contiguous virtual full tensor. The box arrives normalized (BoxGeometry
// in csrc/core/box_geometry.h): equally long contiguous runs nested under
// up to kMaxBoxLevels strided levels — rng_chain_window_kernel's geometry
// with more than one level. A shard unit (a 16-byte group on the vector
// path, an element otherwise) splits into its run and its place within
// the run; the run index is decomposed innermost level first, and every
// coordinate adds its level's stride to the GLOBAL unit index. From there
// on the value is computed exactly as in the kernels above (same group
// id, lane, from_float barrier and tail), so a box is bitwise a sub-tensor
// of the full materialization.
// The decomposition costs one division per level. On the 32-bit index
// path those are multiply-shift divisions by host-computed magics
// (MagicDiv32); the 64-bit path (shards of 2^31 elements or more) divides
// plainly.
// ---------------------------------------------------------------------------

// Geometry in UNITS (groups on the vector path, elements otherwise).
// Levels are outermost first; only levels 1.. are divided by (the
// outermost coordinate is what remains of the run index).
template <typename IdxT>
struct BoxArgs {
  uint64_t g0;
  uint64_t gs[kMaxBoxLevels];
  IdxT run;
  IdxT ext[kMaxBoxLevels];
  int32_t levels;
  // Magics and shifts (MagicDiv32) of `run` and of ext[1..]; unused on
  // the plain-division paths.
  uint32_t run_magic, run_shift;
  uint32_t ext_magic[kMaxBoxLevels - 1];
  uint32_t ext_shift[kMaxBoxLevels - 1];
};

template <typename IdxT, bool kMagic>
__device__ __forceinline__ IdxT boxDiv(IdxT n, IdxT d, uint32_t magic,
                                       uint32_t shift) {
  if constexpr (kMagic) {
    static_assert(std::is_same_v<IdxT, uint32_t>,
                  "the multiply-shift divisor is exact below 2^31 only");
    return magicDiv(MagicDiv32{d, magic, shift}, n);
  } else {
    return n / d;
  }
}

// Global unit index of shard unit j.
template <typename IdxT, bool kMagic>
__device__ __forceinline__ uint64_t boxGlobalUnit(const BoxArgs<IdxT>& box,
                                                  IdxT j) {
  IdxT row = boxDiv<IdxT, kMagic>(j, box.run, box.run_magic, box.run_shift);
  const IdxT within = j - row * box.run;
  uint64_t u = box.g0 + within;
#pragma unroll
  for (int l = kMaxBoxLevels - 1; l >= 1; --l) {
    if (l < box.levels) {
      const IdxT q = boxDiv<IdxT, kMagic>(
          row, box.ext[l], box.ext_magic[l - 1], box.ext_shift[l - 1]);
      u += static_cast<uint64_t>(row - q * box.ext[l]) * box.gs[l];
      row = q;
    }
  }
  return u + static_cast<uint64_t>(row) * box.gs[0];
}

// `vec`: the host's check that `out` is 16-byte aligned and that g_off,
// run_len and every stride are group multiples — `box` is then in groups
// and every group of the box is whole. `n_units` is the shard's group
// (vec) or element count. kHasTail == false carries no tail code.
template <typename T, Dist kDist, typename IdxT, bool kHasTail, bool kMagic>
__global__ void rng_box_kernel(T* __restrict__ out,
                               BoxArgs<IdxT> box,
                               IdxT n_units,
                               bool vec,
                               float a,
                               float b,
                               uint64_t seed,
                               uint64_t offset,
                               TailProgram prog) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;
  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  if (vec) {
    for (IdxT j = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
         j < n_units; j += stride) {
      const uint64_t g = boxGlobalUnit<IdxT, kMagic>(box, j);
      float vals[kElems];
      rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
      if constexpr (kHasTail) {
        applyTail<T, kElems>(vals, prog, g * kElems);
      }
      Vec v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        vp[e] = from_float<T>(vals[e]);
      }
      *reinterpret_cast<Vec*>(out + static_cast<uint64_t>(j) * kElems) = v;
    }
    return;
  }
  for (IdxT i = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
       i < n_units; i += stride) {
    const uint64_t ge = boxGlobalUnit<IdxT, kMagic>(box, i);
    const uint64_t g = ge / kElems;
    float vals[kElems];
    rngGroupValues<T, kDist>(g, a, b, seed, offset, vals);
    if constexpr (kHasTail) {
      applyTail<T, kElems>(vals, prog, g * kElems);
    }
    out[i] = from_float<T>(vals[ge - g * kElems]);
  }
}

// Benchmark switch (scripts/box_kernel_bench.py): with TDX_BOX_PLAIN_DIV=1
// in the environment the untailed 32-bit normal kernels divide with `/`,
// so one process can time both forms alternately.
bool boxPlainDivRequested() {
  const char* v = std::getenv("TDX_BOX_PLAIN_DIV");
  return v != nullptr && v[0] == '1';
}

template <Dist kDist>
void launchRngBox(at::Tensor& shard, const BoxGeometry& geo, double p0,
                  double p1, const TailProgram& prog, int64_t seed,
                  int64_t offset) {
  float a = static_cast<float>(p0);
  float b = kDist == Dist::kUniform ? static_cast<float>(p1 - p0)
                                    : static_cast<float>(p1);
  const int64_t numel = shard.numel();
  const bool ptr_ok = reinterpret_cast<uintptr_t>(shard.data_ptr()) % 16 == 0;
  const bool has_tail = prog.n > 0;
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    constexpr int64_t kElems = VecTraits<T>::kElems;
    bool vec = ptr_ok && geo.g_off % kElems == 0 && geo.run_len % kElems == 0;
    for (int l = 0; l < geo.levels; ++l) {
      vec = vec && geo.g_stride[l] % kElems == 0;
    }
    const int64_t unit = vec ? kElems : 1;
    const int64_t n_units = numel / unit;  // vec: numel is a group multiple
    const int64_t n_work = (numel + kElems - 1) / kElems;
    auto launch_idx = [&](auto idx_tag, auto tail_tag, auto magic_tag) {
      using IdxT = decltype(idx_tag);
      constexpr bool kHasTail = decltype(tail_tag)::value;
      constexpr bool kMagic = decltype(magic_tag)::value;
      BoxArgs<IdxT> box{};
      box.g0 = static_cast<uint64_t>(geo.g_off / unit);
      box.run = static_cast<IdxT>(geo.run_len / unit);
      box.levels = geo.levels;
      for (int l = 0; l < kMaxBoxLevels; ++l) {
        box.gs[l] = 0;
        box.ext[l] = 1;
      }
      for (int l = 0; l < geo.levels; ++l) {
        box.gs[l] = static_cast<uint64_t>(geo.g_stride[l] / unit);
        box.ext[l] = static_cast<IdxT>(geo.extent[l]);
      }
      if constexpr (kMagic) {
        const MagicDiv32 rd = makeMagicDiv32(static_cast<uint32_t>(box.run));
        box.run_magic = rd.magic;
        box.run_shift = rd.shift;
        for (int l = 1; l < kMaxBoxLevels; ++l) {
          const MagicDiv32 ed =
              makeMagicDiv32(static_cast<uint32_t>(box.ext[l]));
          box.ext_magic[l - 1] = ed.magic;
          box.ext_shift[l - 1] = ed.shift;
        }
      }
      hipLaunchKernelGGL(
          (rng_box_kernel<T, kDist, IdxT, kHasTail, kMagic>),
          dim3(numBlocks(n_work)), dim3(kBlock), 0, stream.stream(),
          reinterpret_cast<T*>(shard.data_ptr()), box,
          static_cast<IdxT>(n_units), vec, a, b,
          static_cast<uint64_t>(seed), static_cast<uint64_t>(offset), prog);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (numel > std::numeric_limits<int32_t>::max()) {
      if (has_tail) {
        launch_idx(int64_t{}, std::true_type{}, std::false_type{});
      } else {
        launch_idx(int64_t{}, std::false_type{}, std::false_type{});
      }
    } else if (has_tail) {
      launch_idx(uint32_t{}, std::true_type{}, std::true_type{});
    } else if (kDist == Dist::kNormal && boxPlainDivRequested()) {
      if constexpr (kDist == Dist::kNormal) {
        launch_idx(uint32_t{}, std::false_type{}, std::false_type{});
      }
    } else {
      launch_idx(uint32_t{}, std::false_type{}, std::true_type{});
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    case at::kHalf:
      launch(__half{});
      break;
    default:
      TORCH_CHECK(false, "tdx box kernel supports float32/bf16/fp16, got ",
                  shard.scalar_type());
  }
}

at::Tensor& tdx_rng_box_(at::Tensor& shard, at::IntArrayRef extents,
                         at::IntArrayRef g_strides, int64_t run_len,
                         int64_t g_off, int64_t dist, double p0, double p1,
                         at::IntArrayRef tail_ops,
                         at::ArrayRef<double> tail_s0,
                         at::ArrayRef<double> tail_s1, int64_t full_numel,
                         int64_t seed, int64_t offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx shard kernels require contiguous tensors");
  const char* err =
      checkBoxArgs(extents.data(), extents.size(), g_strides.data(),
                   g_strides.size(), run_len, g_off, shard.numel(),
                   full_numel);
  TORCH_CHECK(err == nullptr, "rng_box: ", err);
  const TailProgram prog =
      makeTailProgram(tail_ops, tail_s0, tail_s1, full_numel);
  TORCH_CHECK(dist != 1 || p1 >= 0.0,
              "normal_ expects std >= 0.0, but found std=", p1);
  TORCH_CHECK(dist != 2 || (0.0 <= p0 && p0 <= 1.0),
              "bernoulli_ expects 0 <= p <= 1, but found p=", p0);
  TORCH_CHECK(0 <= dist && dist <= 2,
              "rng_box: dist must be 0 (uniform), 1 (normal) or 2 "
              "(bernoulli), got ", dist);
  TORCH_CHECK(shard.scalar_type() == at::kFloat ||
                  shard.scalar_type() == at::kBFloat16 ||
                  shard.scalar_type() == at::kHalf,
              "tdx box kernel supports float32/bf16/fp16, got ",
              shard.scalar_type());
  if (shard.numel() == 0) {
    return shard;
  }
  BoxGeometry geo;
  geo.g_off = g_off;
  geo.run_len = run_len;
  geo.levels = static_cast<int32_t>(extents.size());
  for (int l = 0; l < geo.levels; ++l) {
    geo.extent[l] = extents[l];
    geo.g_stride[l] = g_strides[l];
  }
  switch (dist) {
    case 0:
      launchRngBox<Dist::kUniform>(shard, geo, p0, p1, prog, seed, offset);
      break;
    case 1:
      launchRngBox<Dist::kNormal>(shard, geo, p0, p1, prog, seed, offset);
      break;
    default:
      launchRngBox<Dist::kBernoulli>(shard, geo, p0, 0.0, prog, seed,
                                     offset);
      break;
  }
  return shard;
}

// ---------------------------------------------------------------------------
// Patch kernel (tdx::patch_box_): a value step recorded on a contiguous
// sub-range [lo, hi) of the full tensor (`w[i].zero_()`,
// `w[:k].normal_()`), applied to the part of it a box holds. The rows of
// the box that meet the patch are one contiguous row range, found on the
// host (rowsMeeting); the kernel walks only those, so its work is the
// intersection plus the two edge rows, whatever the shard's or the
// patch's size.
//
// A work item is one (row, view group) pair: `slots` items per row, the
// most 16-byte groups of the patch VIEW a row can meet. Item s of a row
// is group k0 / kElems + s of the view, k0 being the row's first view
// element; items past the row's last group do nothing. The group's values
// come from rngGroupValues keyed by the VIEW group index, so they are the
// full-tensor kernels' values for a contiguous patch_len-element tensor;
// the lanes inside row and patch are stored, as one 16-byte store when the
// group is whole and its destination aligned, element by element
// otherwise. The constant kinds store the scalar narrowed as fill_kernel
// narrows it.
// ---------------------------------------------------------------------------

// Geometry in ELEMENTS. Levels are outermost first; only levels 1.. are
// divided by, as in BoxArgs.
template <typename IdxT>
struct PatchArgs {
  int64_t g_off;
  int64_t gs[kMaxBoxLevels];
  int64_t run_len;
  int64_t lo, hi;     // the patch, in full-tensor elements
  int64_t row_first;  // first row that meets the patch
  IdxT ext[kMaxBoxLevels];
  IdxT slots;
  int32_t levels;
  uint32_t slots_magic, slots_shift;
  uint32_t ext_magic[kMaxBoxLevels - 1];
  uint32_t ext_shift[kMaxBoxLevels - 1];
};

enum class PatchKind { kUniform, kNormal, kBernoulli, kConst };

template <typename T, PatchKind kKind, typename IdxT, bool kMagic>
__global__ void patch_box_kernel(T* __restrict__ out,
                                 PatchArgs<IdxT> p,
                                 IdxT n_work,
                                 float a,
                                 float b,
                                 uint64_t seed,
                                 uint64_t offset) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;
  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  for (IdxT w = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
       w < n_work; w += stride) {
    const IdxT rel =
        boxDiv<IdxT, kMagic>(w, p.slots, p.slots_magic, p.slots_shift);
    const IdxT slot = w - rel * p.slots;
    const int64_t row = p.row_first + static_cast<int64_t>(rel);
    // First full-tensor element of the row (BoxGeometry::rowStart).
    IdxT rem = static_cast<IdxT>(row);
    int64_t rs = p.g_off;
#pragma unroll
    for (int l = kMaxBoxLevels - 1; l >= 1; --l) {
      if (l < p.levels) {
        const IdxT q = boxDiv<IdxT, kMagic>(rem, p.ext[l], p.ext_magic[l - 1],
                                            p.ext_shift[l - 1]);
        rs += static_cast<int64_t>(rem - q * p.ext[l]) * p.gs[l];
        rem = q;
      }
    }
    rs += static_cast<int64_t>(rem) * p.gs[0];
    // Row ∩ patch in view elements [k0, k1); non-empty for these rows.
    const int64_t ga = rs > p.lo ? rs : p.lo;
    const int64_t gb = rs + p.run_len < p.hi ? rs + p.run_len : p.hi;
    const int64_t k0 = ga - p.lo;
    const int64_t k1 = gb - p.lo;
    const int64_t g = k0 / kElems + static_cast<int64_t>(slot);
    const int64_t kb = g * kElems;
    if (kb >= k1) {
      continue;
    }
    // Shard index of the group's lane 0 (before the row's start when the
    // group begins left of it; only in-range lanes are addressed).
    const int64_t i0 = row * p.run_len + (kb + p.lo - rs);
    T vals_t[kElems];
    if constexpr (kKind == PatchKind::kConst) {
      const T value = from_float<T>(a);
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        vals_t[e] = value;
      }
    } else {
      constexpr Dist kDist = kKind == PatchKind::kUniform
                                 ? Dist::kUniform
                                 : (kKind == PatchKind::kNormal
                                        ? Dist::kNormal
                                        : Dist::kBernoulli);
      float vals[kElems];
      rngGroupValues<T, kDist>(static_cast<uint64_t>(g), a, b, seed, offset,
                               vals);
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        vals_t[e] = from_float<T>(vals[e]);
      }
    }
    const bool whole = kb >= k0 && kb + kElems <= k1;
    if (whole && reinterpret_cast<uintptr_t>(out + i0) % 16 == 0) {
      Vec v;
      T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        vp[e] = vals_t[e];
      }
      *reinterpret_cast<Vec*>(out + i0) = v;
    } else {
#pragma unroll
      for (int e = 0; e < kElems; ++e) {
        const int64_t k = kb + e;
        if (k >= k0 && k < k1) {
          out[i0 + e] = vals_t[e];
        }
      }
    }
  }
}

template <PatchKind kKind>
void launchPatchBox(at::Tensor& shard, const BoxGeometry& geo,
                    const RowRange& rows, int64_t patch_lo, int64_t patch_len,
                    float a, float b, uint64_t seed, uint64_t offset) {
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    constexpr int64_t kElems = VecTraits<T>::kElems;
    // The most view groups an interval of run_len elements can touch,
    // and never more than the view has.
    const int64_t slots =
        std::min((geo.run_len + kElems - 2) / kElems + 1,
                 (patch_len + kElems - 1) / kElems);
    const int64_t n_work = rows.count() * slots;
    auto launch_idx = [&](auto idx_tag, auto magic_tag) {
      using IdxT = decltype(idx_tag);
      constexpr bool kMagic = decltype(magic_tag)::value;
      PatchArgs<IdxT> p{};
      p.g_off = geo.g_off;
      p.run_len = geo.run_len;
      p.lo = patch_lo;
      p.hi = patch_lo + patch_len;
      p.row_first = rows.first;
      p.levels = geo.levels;
      p.slots = static_cast<IdxT>(slots);
      for (int l = 0; l < kMaxBoxLevels; ++l) {
        p.gs[l] = 0;
        p.ext[l] = 1;
      }
      for (int l = 0; l < geo.levels; ++l) {
        p.gs[l] = geo.g_stride[l];
        p.ext[l] = static_cast<IdxT>(geo.extent[l]);
      }
      if constexpr (kMagic) {
        const MagicDiv32 sd = makeMagicDiv32(static_cast<uint32_t>(slots));
        p.slots_magic = sd.magic;
        p.slots_shift = sd.shift;
        for (int l = 1; l < kMaxBoxLevels; ++l) {
          const MagicDiv32 ed =
              makeMagicDiv32(static_cast<uint32_t>(p.ext[l]));
          p.ext_magic[l - 1] = ed.magic;
          p.ext_shift[l - 1] = ed.shift;
        }
      }
      hipLaunchKernelGGL((patch_box_kernel<T, kKind, IdxT, kMagic>),
                         dim3(numBlocks(n_work)), dim3(kBlock), 0,
                         stream.stream(),
                         reinterpret_cast<T*>(shard.data_ptr()), p,
                         static_cast<IdxT>(n_work), a, b, seed, offset);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    // The multiply-shift division is exact below 2^31: both the work
    // index and the row index must stay under it.
    if (n_work > std::numeric_limits<int32_t>::max() ||
        geo.rows() > std::numeric_limits<int32_t>::max()) {
      launch_idx(int64_t{}, std::false_type{});
    } else {
      launch_idx(uint32_t{}, std::true_type{});
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    default:
      launch(__half{});
      break;
  }
}

at::Tensor& tdx_patch_box_(at::Tensor& shard, at::IntArrayRef extents,
                           at::IntArrayRef g_strides, int64_t run_len,
                           int64_t g_off, int64_t full_numel,
                           int64_t patch_lo, int64_t patch_len, int64_t dist,
                           double p0, double p1, std::optional<int64_t> seed,
                           std::optional<int64_t> offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx shard kernels require contiguous tensors");
  const char* err =
      checkBoxArgs(extents.data(), extents.size(), g_strides.data(),
                   g_strides.size(), run_len, g_off, shard.numel(),
                   full_numel);
  TORCH_CHECK(err == nullptr, "patch_box: ", err);
  err = checkPatchArgs(patch_lo, patch_len, full_numel, dist,
                       seed.has_value(), offset.has_value());
  TORCH_CHECK(err == nullptr, "patch_box: ", err);
  TORCH_CHECK(dist != 1 || p1 >= 0.0,
              "normal_ expects std >= 0.0, but found std=", p1);
  TORCH_CHECK(dist != 2 || (0.0 <= p0 && p0 <= 1.0),
              "bernoulli_ expects 0 <= p <= 1, but found p=", p0);
  TORCH_CHECK(shard.scalar_type() == at::kFloat ||
                  shard.scalar_type() == at::kBFloat16 ||
                  shard.scalar_type() == at::kHalf,
              "tdx patch kernel supports float32/bf16/fp16, got ",
              shard.scalar_type());
  BoxGeometry geo;
  geo.g_off = g_off;
  geo.run_len = run_len;
  geo.levels = static_cast<int32_t>(extents.size());
  for (int l = 0; l < geo.levels; ++l) {
    geo.extent[l] = extents[l];
    geo.g_stride[l] = g_strides[l];
  }
  const RowRange rows = rowsMeeting(geo, patch_lo, patch_lo + patch_len);
  if (rows.count() == 0) {
    return shard;  // the patch misses the box (or one of them is empty)
  }
  const auto s = static_cast<uint64_t>(seed.value_or(0));
  const auto o = static_cast<uint64_t>(offset.value_or(0));
  const float a = static_cast<float>(p0);
  switch (dist) {
    case 0:
      launchPatchBox<PatchKind::kUniform>(shard, geo, rows, patch_lo,
                                          patch_len, a,
                                          static_cast<float>(p1 - p0), s, o);
      break;
    case 1:
      launchPatchBox<PatchKind::kNormal>(shard, geo, rows, patch_lo,
                                         patch_len, a, static_cast<float>(p1),
                                         s, o);
      break;
    case 2:
      launchPatchBox<PatchKind::kBernoulli>(shard, geo, rows, patch_lo,
                                            patch_len, a, 0.0f, s, o);
      break;
    case 3:
      launchPatchBox<PatchKind::kConst>(shard, geo, rows, patch_lo, patch_len,
                                        a, 0.0f, 0, 0);
      break;
    default:
      launchPatchBox<PatchKind::kConst>(shard, geo, rows, patch_lo, patch_len,
                                        0.0f, 0.0f, 0, 0);
      break;
  }
  return shard;
}

at::Tensor& tdx_fill_(at::Tensor& self, const at::Scalar& value) {
  TORCH_CHECK(self.is_contiguous(),
              "tdx init kernels require contiguous tensors");
  const int64_t n = self.numel();
  if (n == 0) {
    return self;
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  auto launch = [&](auto type_tag) {
    using T = decltype(type_tag);
    const int64_t n_groups =
        (n + VecTraits<T>::kElems - 1) / VecTraits<T>::kElems;
    hipLaunchKernelGGL(fill_kernel<T>, dim3(numBlocks(n_groups)),
                       dim3(kBlock), 0, stream.stream(),
                       reinterpret_cast<T*>(self.data_ptr()), n,
                       value.to<float>());
    C10_HIP_KERNEL_LAUNCH_CHECK();
  };
  switch (self.scalar_type()) {
    case at::kFloat:
      launch(float{});
      break;
    case at::kBFloat16:
      launch(__hip_bfloat16{});
      break;
    case at::kHalf:
      launch(__half{});
      break;
    default:
      TORCH_CHECK(false, "tdx fill kernel supports float32/bf16/fp16, got ",
                  self.scalar_type());
  }
  return self;
}

// Vectorized cast-copy: dst[i] = cast(src[i]) for contiguous same-shape
// GPU tensors across {f32, bf16, f16}. 8 elements per thread per
// iteration; the narrow side uses 16-byte packs, the f32 side 2x16-byte.
template <typename TDst, typename TSrc, typename IdxT>
__global__ void cast_copy_kernel(TDst* __restrict__ dst,
                                 const TSrc* __restrict__ src,
                                 IdxT n) {
  struct alignas(16) PackDst {
    TDst v[8];
  };
  struct alignas(16) PackSrc {
    TSrc v[8];
  };
  const IdxT n_groups = (n + 7) / 8;
  const IdxT stride = static_cast<IdxT>(gridDim.x) * blockDim.x;
  for (IdxT g = blockIdx.x * static_cast<IdxT>(blockDim.x) + threadIdx.x;
       g < n_groups; g += stride) {
    const IdxT base = g * 8;
    if (base + 8 <= n) {
      PackSrc in = *reinterpret_cast<const PackSrc*>(src + base);
      PackDst out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f;
        if constexpr (std::is_same_v<TSrc, float>) {
          f = in.v[j];
        } else if constexpr (std::is_same_v<TSrc, __hip_bfloat16>) {
          f = __bfloat162float(in.v[j]);
        } else {
          f = __half2float(in.v[j]);
        }
        out.v[j] = from_float<TDst>(f);
      }
      *reinterpret_cast<PackDst*>(dst + base) = out;
    } else {
      for (IdxT j = 0; base + j < n; ++j) {
        float f;
        if constexpr (std::is_same_v<TSrc, float>) {
          f = src[base + j];
        } else if constexpr (std::is_same_v<TSrc, __hip_bfloat16>) {
          f = __bfloat162float(src[base + j]);
        } else {
          f = __half2float(src[base + j]);
        }
        dst[base + j] = from_float<TDst>(f);
      }
    }
  }
}

template <typename F>
bool dispatchCopyType(c10::ScalarType st, F&& f) {
  switch (st) {
    case at::kFloat:
      f(float{});
      return true;
    case at::kBFloat16:
      f(__hip_bfloat16{});
      return true;
    case at::kHalf:
      f(__half{});
      return true;
    default:
      return false;
  }
}

at::Tensor& tdx_copy_(at::Tensor& self,
                      const at::Tensor& src,
                      bool non_blocking) {
  (void)non_blocking;  // same-device async copy; stream-ordered anyway
  TORCH_CHECK(self.is_contiguous() && src.is_contiguous() &&
                  self.sizes().equals(src.sizes()) && self.is_cuda() &&
                  src.is_cuda(),
              "tdx::copy_ requires contiguous same-shape GPU tensors");
  const int64_t n = self.numel();
  if (n == 0) {
    return self;
  }
  // Same dtype: a straight device memcpy is the fastest path.
  if (self.scalar_type() == src.scalar_type()) {
    auto stream = at::cuda::getCurrentCUDAStream();
    C10_HIP_CHECK(hipMemcpyAsync(self.data_ptr(), src.data_ptr(),
                                 n * self.element_size(),
                                 hipMemcpyDeviceToDevice, stream.stream()));
    return self;
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  bool ok = dispatchCopyType(self.scalar_type(), [&](auto dt) {
    using TDst = decltype(dt);
    dispatchCopyType(src.scalar_type(), [&](auto st2) {
      using TSrc = decltype(st2);
      const int64_t n_groups = (n + 7) / 8;
      if (n <= std::numeric_limits<uint32_t>::max() / 2) {
        hipLaunchKernelGGL((cast_copy_kernel<TDst, TSrc, uint32_t>),
                           dim3(numBlocks(n_groups)), dim3(kBlock), 0,
                           stream.stream(),
                           reinterpret_cast<TDst*>(self.data_ptr()),
                           reinterpret_cast<const TSrc*>(src.data_ptr()),
                           static_cast<uint32_t>(n));
      } else {
        hipLaunchKernelGGL((cast_copy_kernel<TDst, TSrc, uint64_t>),
                           dim3(numBlocks(n_groups)), dim3(kBlock), 0,
                           stream.stream(),
                           reinterpret_cast<TDst*>(self.data_ptr()),
                           reinterpret_cast<const TSrc*>(src.data_ptr()),
                           static_cast<uint64_t>(n));
      }
      C10_HIP_KERNEL_LAUNCH_CHECK();
    });
  });
  TORCH_CHECK(ok, "tdx::copy_ supports float32/bf16/fp16");
  return self;
}

at::Tensor& tdx_zero_(at::Tensor& self) {
  if (!self.is_contiguous() || self.numel() == 0) {
    return self.zero_();
  }
  // A pure byte clear: hand it to the copy engine via memset.
  auto stream = at::cuda::getCurrentCUDAStream();
  C10_HIP_CHECK(hipMemsetAsync(self.data_ptr(), 0,
                               self.numel() * self.element_size(),
                               stream.stream()));
  return self;
}

// ---------------------------------------------------------------------------
// Batched init: ONE launch fills a whole list of tensors (the reduced
// value steps of simple init chains, see tensorInitPlan). A 70B replica
// is ~560 per-tensor launches; at ~8 us of launch+ramp each, batching
// them recovers ~4.5 ms of a ~53 ms step. Virtual blocks of kInitEPB
// elements map to tensors via a prefix table (same dispatch shape as
// the batched AdamW kernel); each tensor keeps its own Philox
// (seed, offset) and group indexing from 0, so bits are identical to
// the per-tensor kernels.
// ---------------------------------------------------------------------------

constexpr int kInitEPB = 16384;  // elements per virtual block

struct InitTensorMeta {
  void* ptr;
  int64_t n;
  int32_t dist;   // 0 uniform, 1 normal, 2 bernoulli, 3 fill, 4 zero
  int32_t dtype;  // 0 f32, 1 bf16, 2 f16
  float a, b;     // (from, range) / (mean, std) / (p, -) / (value, -)
  uint64_t seed, offset;
};

// kHasTail: apply the tensor's fused pointwise tail (`tail`, in the blob)
// before the stores; the false instantiation is the tail-free code as it
// always was.
template <typename T, Dist kDist, bool kHasTail>
__device__ __forceinline__ void fillRangeVec(T* __restrict__ out,
                                             int64_t begin, int64_t end,
                                             int64_t n, float a, float b,
                                             uint64_t seed,
                                             uint64_t offset,
                                             const TailProgram* tail) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;
  // begin is kInitEPB-aligned (hence kElems-aligned); only the last
  // vblock can carry a partial tail group — handled by one thread after
  // the branchless full-group loop.
  const int64_t full_end = begin + ((end - begin) / kElems) * kElems;
  for (int64_t base = begin + threadIdx.x * kElems; base < full_end;
       base += blockDim.x * kElems) {
    float vals[kElems];
    rngGroupValues<T, kDist>(static_cast<uint64_t>(base / kElems), a, b,
                             seed, offset, vals);
    if constexpr (kHasTail) {
      applyTail<T, kElems>(vals, *tail, static_cast<uint64_t>(base));
    }
    Vec v;
    T* vp = reinterpret_cast<T*>(&v);
#pragma unroll
    for (int j = 0; j < kElems; ++j) {
      vp[j] = from_float<T>(vals[j]);
    }
    *reinterpret_cast<Vec*>(out + base) = v;
  }
  if (threadIdx.x == 0 && full_end < end) {
    float vals[kElems];
    rngGroupValues<T, kDist>(static_cast<uint64_t>(full_end / kElems), a,
                             b, seed, offset, vals);
    if constexpr (kHasTail) {
      applyTail<T, kElems>(vals, *tail, static_cast<uint64_t>(full_end));
    }
    for (int64_t e = full_end; e < end; ++e) {
      out[e] = from_float<T>(vals[e - full_end]);
    }
  }
}

template <typename T>
__device__ __forceinline__ void fillRangeConst(T* __restrict__ out,
                                               int64_t begin, int64_t end,
                                               int64_t n, float value) {
  constexpr int kElems = VecTraits<T>::kElems;
  using Vec = typename VecTraits<T>::Vec;
  const T v = from_float<T>(value);
  Vec pack;
  T* vp = reinterpret_cast<T*>(&pack);
#pragma unroll
  for (int j = 0; j < kElems; ++j) {
    vp[j] = v;
  }
  for (int64_t base = begin + threadIdx.x * kElems; base < end;
       base += blockDim.x * kElems) {
    if (base + kElems <= n) {
      *reinterpret_cast<Vec*>(out + base) = pack;
    } else {
      for (int64_t j = 0; base + j < n; ++j) {
        out[base + j] = v;
      }
    }
  }
}

template <typename T, bool kHasTail>
__device__ __forceinline__ void initDispatchDist(const InitTensorMeta& mt,
                                                 int64_t begin,
                                                 int64_t end,
                                                 const TailProgram* tail) {
  T* out = static_cast<T*>(mt.ptr);
  switch (mt.dist) {
    case 0:
      fillRangeVec<T, Dist::kUniform, kHasTail>(out, begin, end, mt.n, mt.a, mt.b,
                                      mt.seed, mt.offset, tail);
      break;
    case 1:
      fillRangeVec<T, Dist::kNormal, kHasTail>(out, begin, end, mt.n, mt.a, mt.b,
                                     mt.seed, mt.offset, tail);
      break;
    case 2:
      fillRangeVec<T, Dist::kBernoulli, kHasTail>(out, begin, end, mt.n, mt.a, mt.b,
                                        mt.seed, mt.offset, tail);
      break;
    case 3:
      fillRangeConst<T>(out, begin, end, mt.n, mt.a);
      break;
    default:
      fillRangeConst<T>(out, begin, end, mt.n, 0.0f);
      break;
  }
}

// blob layout: int64 prefix[n_tensors], InitTensorMeta[n_tensors] and,
// when kHasTail, TailProgram[n_tensors] (n == 0 for a tensor without a
// tail). The tails sit in a table of their own, not in InitTensorMeta,
// so a batch without tails reads the blob it always read and launches
// the instantiation that compiles to the code that was here before.
template <bool kHasTail>
__global__ void batched_init_kernel(const uint8_t* __restrict__ blob,
                                    int32_t n_tensors,
                                    int64_t total_vblocks) {
  const int64_t* prefix = reinterpret_cast<const int64_t*>(blob);
  const InitTensorMeta* metas = reinterpret_cast<const InitTensorMeta*>(
      blob + sizeof(int64_t) * n_tensors);
  const TailProgram* tails =
      kHasTail ? reinterpret_cast<const TailProgram*>(
                     blob + (sizeof(int64_t) + sizeof(InitTensorMeta)) *
                                n_tensors)
               : nullptr;

  for (int64_t vb = blockIdx.x; vb < total_vblocks; vb += gridDim.x) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= vb) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    const InitTensorMeta mt = metas[lo];
    const int64_t begin = (vb - prefix[lo]) * kInitEPB;
    const int64_t end = begin + kInitEPB < mt.n ? begin + kInitEPB : mt.n;
    const TailProgram* tail = kHasTail ? tails + lo : nullptr;
    switch (mt.dtype) {
      case 0:
        initDispatchDist<float, kHasTail>(mt, begin, end, tail);
        break;
      case 1:
        initDispatchDist<__hip_bfloat16, kHasTail>(mt, begin, end, tail);
        break;
      default:
        initDispatchDist<__half, kHasTail>(mt, begin, end, tail);
        break;
    }
  }
}

// fillRangeVec for a tensor whose chain ends in a dtype conversion: drawn
// and run through the tail at TSrc, stored as TDst, in units of 8 elements
// (castUnitLoop). begin is kInitEPB-aligned and kInitEPB is a unit
// multiple, so virtual blocks start on a unit; only the tensor's last
// vblock can carry a partial unit, stored elementwise by one thread.
static_assert(kInitEPB % kCastUnit == 0 && (kInitEPB / kCastUnit) % 64 == 0,
              "virtual blocks must start on a unit, at lane 0 of a wave");

template <typename TSrc, typename TDst, Dist kDist>
__device__ __forceinline__ void fillRangeCast(TDst* __restrict__ out,
                                              int64_t begin, int64_t end,
                                              float a, float b,
                                              uint64_t seed, uint64_t offset,
                                              const TailProgram& tail) {
  const int64_t full_end =
      begin + ((end - begin) / kCastUnit) * kCastUnit;
  castUnitLoop<TSrc, TDst, kDist, int64_t>(
      out, begin / kCastUnit + threadIdx.x, full_end / kCastUnit,
      static_cast<int64_t>(blockDim.x),
      [](int64_t j) -> uint64_t { return static_cast<uint64_t>(j); }, a, b,
      seed, offset, tail);
  if (threadIdx.x == 0 && full_end < end) {
    storePartialCastUnit<TSrc, TDst, kDist>(
        out + full_end, static_cast<uint32_t>(end - full_end),
        static_cast<uint64_t>(full_end / kCastUnit), a, b, seed, offset,
        tail);
  }
}

template <typename TSrc, typename TDst>
__device__ __forceinline__ void castDispatchDist(void* ptr, int32_t dist,
                                                 float a, float b,
                                                 uint64_t seed,
                                                 uint64_t offset,
                                                 int64_t begin, int64_t end,
                                                 const TailProgram& tail) {
  TDst* out = static_cast<TDst*>(ptr);
  switch (dist) {
    case 0:
      fillRangeCast<TSrc, TDst, Dist::kUniform>(out, begin, end, a, b, seed,
                                                offset, tail);
      break;
    case 1:
      fillRangeCast<TSrc, TDst, Dist::kNormal>(out, begin, end, a, b, seed,
                                               offset, tail);
      break;
    default:  // 2; the host admits RNG plans only
      fillRangeCast<TSrc, TDst, Dist::kBernoulli>(out, begin, end, a, b, seed,
                                                  offset, tail);
      break;
  }
}

// The batched kernel for tensors with a conversion; batches without one
// never launch it, and batched_init_kernel is untouched by it. One
// instantiation: the (source, destination) pair and the distribution are
// uniform per virtual block, so the dispatch is scalar branches. blob
// layout: int64 prefix[n], InitTensorMeta[n] (dtype = the destination's),
// TailProgram[n] (always present, n == 0 for none), int32 src_dtype[n].
__global__ void batched_init_cast_kernel(const uint8_t* __restrict__ blob,
                                         int32_t n_tensors,
                                         int64_t total_vblocks) {
  const int64_t* prefix = reinterpret_cast<const int64_t*>(blob);
  const InitTensorMeta* metas = reinterpret_cast<const InitTensorMeta*>(
      blob + sizeof(int64_t) * n_tensors);
  const TailProgram* tails = reinterpret_cast<const TailProgram*>(
      blob + (sizeof(int64_t) + sizeof(InitTensorMeta)) * n_tensors);
  const int32_t* srcs = reinterpret_cast<const int32_t*>(
      blob + (sizeof(int64_t) + sizeof(InitTensorMeta) +
              sizeof(TailProgram)) * n_tensors);

  for (int64_t vb = blockIdx.x; vb < total_vblocks; vb += gridDim.x) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (prefix[mid] <= vb) {
        lo = mid;
      } else {
        hi = mid - 1;
      }
    }
    const InitTensorMeta mt = metas[lo];
    const int64_t begin = (vb - prefix[lo]) * kInitEPB;
    const int64_t end = begin + kInitEPB < mt.n ? begin + kInitEPB : mt.n;
    const TailProgram& tail = tails[lo];
    switch (srcs[lo] * 3 + mt.dtype) {
      case 0 * 3 + 1:
        castDispatchDist<float, __hip_bfloat16>(
            mt.ptr, mt.dist, mt.a, mt.b, mt.seed, mt.offset, begin, end, tail);
        break;
      case 0 * 3 + 2:
        castDispatchDist<float, __half>(
            mt.ptr, mt.dist, mt.a, mt.b, mt.seed, mt.offset, begin, end, tail);
        break;
      case 1 * 3 + 0:
        castDispatchDist<__hip_bfloat16, float>(
            mt.ptr, mt.dist, mt.a, mt.b, mt.seed, mt.offset, begin, end, tail);
        break;
      case 1 * 3 + 2:
        castDispatchDist<__hip_bfloat16, __half>(
            mt.ptr, mt.dist, mt.a, mt.b, mt.seed, mt.offset, begin, end, tail);
        break;
      case 2 * 3 + 0:
        castDispatchDist<__half, float>(
            mt.ptr, mt.dist, mt.a, mt.b, mt.seed, mt.offset, begin, end, tail);
        break;
      default:  // 2 * 3 + 1; the host admits the six pairs only
        castDispatchDist<__half, __hip_bfloat16>(
            mt.ptr, mt.dist, mt.a, mt.b, mt.seed, mt.offset, begin, end, tail);
        break;
    }
  }
}

void batchedInitPlain(std::vector<at::Tensor> tensors,
                      std::vector<int64_t> dists,
                      std::vector<double> p0s,
                      std::vector<double> p1s,
                      std::vector<int64_t> seeds,
                      std::vector<int64_t> offsets,
                      std::vector<std::vector<int64_t>> tail_ops,
                      std::vector<std::vector<double>> tail_s0,
                      std::vector<std::vector<double>> tail_s1);

// A batch's tensors with a conversion, checked: every tensor's source
// dtype code and tail program. Everything that can be refused is refused
// here, before any launch of the batch — the conversion-free part
// included.
struct CastBatch {
  std::vector<int32_t> srcs;
  std::vector<TailProgram> tails;
};

CastBatch checkBatchedCast(
    const std::vector<at::Tensor>& tensors,
    const std::vector<int64_t>& dists,
    const std::vector<double>& p1s,
    const std::vector<std::vector<int64_t>>& tail_ops,
    const std::vector<std::vector<double>>& tail_s0,
    const std::vector<std::vector<double>>& tail_s1,
    const std::vector<at::ScalarType>& src_dtypes) {
  CastBatch batch;
  for (size_t t = 0; t < tensors.size(); ++t) {
    const at::Tensor& x = tensors[t];
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
                "batched init: contiguous GPU tensors only");
    TORCH_CHECK(x.device() == tensors[0].device(),
                "batched init: one device per batch");
    TORCH_CHECK(0 <= dists[t] && dists[t] <= 2,
                "batched init: only RNG plans carry a src_dtype");
    const int dst = castDtypeCode(x.scalar_type());
    const int src = castDtypeCode(src_dtypes[t]);
    TORCH_CHECK(dst >= 0 && src >= 0 && dst != src,
                "batched init: a conversion is between two different "
                "dtypes of f32/bf16/f16, got ", src_dtypes[t], " -> ",
                x.scalar_type());
    // The allocator's blocks are 512-byte aligned; the vector stores need
    // 16.
    TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
                "batched init: 16-byte aligned tensors only");
    TORCH_CHECK(dists[t] != 1 || p1s[t] >= 0.0,
                "normal_ expects std >= 0.0, but found std=", p1s[t]);
    batch.srcs.push_back(src);
    batch.tails.push_back(
        tail_ops.empty()
            ? makeTailProgram(at::IntArrayRef{}, at::ArrayRef<double>{},
                              at::ArrayRef<double>{}, x.numel())
            : makeTailProgram(tail_ops[t], tail_s0[t], tail_s1[t],
                              x.numel()));
  }
  return batch;
}

// The second launch of a batch: its tensors with a conversion.
void batchedInitCast(const std::vector<at::Tensor>& tensors,
                     const std::vector<int64_t>& dists,
                     const std::vector<double>& p0s,
                     const std::vector<double>& p1s,
                     const std::vector<int64_t>& seeds,
                     const std::vector<int64_t>& offsets,
                     const CastBatch& batch) {
  static_assert(sizeof(InitTensorMeta) % alignof(TailProgram) == 0 &&
                    sizeof(int64_t) % alignof(TailProgram) == 0 &&
                    sizeof(TailProgram) % alignof(int32_t) == 0,
                "the tables must stay aligned behind one another");
  const size_t n_tensors = tensors.size();
  const size_t metas_off = sizeof(int64_t) * n_tensors;
  const size_t tails_off = metas_off + sizeof(InitTensorMeta) * n_tensors;
  const size_t srcs_off = tails_off + sizeof(TailProgram) * n_tensors;
  const size_t blob_bytes = srcs_off + sizeof(int32_t) * n_tensors;
  at::Tensor host_blob = at::empty(
      {static_cast<int64_t>(blob_bytes)},
      at::TensorOptions().dtype(at::kByte).pinned_memory(true));
  auto* base = static_cast<uint8_t*>(host_blob.data_ptr());
  auto* prefix = reinterpret_cast<int64_t*>(base);
  auto* metas = reinterpret_cast<InitTensorMeta*>(base + metas_off);
  auto* tails = reinterpret_cast<TailProgram*>(base + tails_off);
  auto* srcs = reinterpret_cast<int32_t*>(base + srcs_off);
  int64_t total_vblocks = 0;
  for (size_t t = 0; t < n_tensors; ++t) {
    const at::Tensor& x = tensors[t];
    InitTensorMeta& mt = metas[t];
    mt.ptr = x.data_ptr();
    mt.n = x.numel();
    mt.dist = static_cast<int32_t>(dists[t]);
    mt.dtype = castDtypeCode(x.scalar_type());
    // Same (a, b) mapping as launchRng.
    mt.a = static_cast<float>(p0s[t]);
    mt.b = mt.dist == 0 ? static_cast<float>(p1s[t] - p0s[t])
                        : static_cast<float>(p1s[t]);
    mt.seed = static_cast<uint64_t>(seeds[t]);
    mt.offset = static_cast<uint64_t>(offsets[t]);
    tails[t] = batch.tails[t];
    srcs[t] = batch.srcs[t];
    prefix[t] = total_vblocks;
    total_vblocks += (mt.n + kInitEPB - 1) / kInitEPB;
  }
  if (total_vblocks == 0) {
    return;
  }
  at::Tensor dev_blob =
      host_blob.to(tensors[0].device(), /*non_blocking=*/true);
  const int grid =
      static_cast<int>(std::min<int64_t>(total_vblocks, 16384));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(batched_init_cast_kernel, dim3(grid), dim3(kBlock), 0,
                     stream.stream(),
                     static_cast<const uint8_t*>(dev_blob.const_data_ptr()),
                     static_cast<int32_t>(n_tensors), total_vblocks);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace

// `src_dtypes`: nullopt (or all-None) for a batch without conversions,
// which launches exactly what it always launched. Otherwise one entry per
// tensor; the tensors with one go into a second launch of their own
// kernel, the others into the first as before.
void batched_init_launch(
    std::vector<at::Tensor> tensors,
    std::vector<int64_t> dists,
    std::vector<double> p0s,
    std::vector<double> p1s,
    std::vector<int64_t> seeds,
    std::vector<int64_t> offsets,
    std::vector<std::vector<int64_t>> tail_ops,
    std::vector<std::vector<double>> tail_s0,
    std::vector<std::vector<double>> tail_s1,
    std::optional<std::vector<std::optional<at::ScalarType>>> src_dtypes) {
  bool any_cast = false;
  if (src_dtypes.has_value()) {
    TORCH_CHECK(src_dtypes->size() == tensors.size(),
                "batched init: src_dtypes length mismatch");
    for (const auto& s : *src_dtypes) {
      any_cast = any_cast || s.has_value();
    }
  }
  if (!any_cast) {
    batchedInitPlain(std::move(tensors), std::move(dists), std::move(p0s),
                     std::move(p1s), std::move(seeds), std::move(offsets),
                     std::move(tail_ops), std::move(tail_s0),
                     std::move(tail_s1));
    return;
  }
  const size_t n = tensors.size();
  TORCH_CHECK(dists.size() == n && p0s.size() == n && p1s.size() == n &&
                  seeds.size() == n && offsets.size() == n,
              "batched init: list length mismatch");
  TORCH_CHECK((tail_ops.empty() && tail_s0.empty() && tail_s1.empty()) ||
                  (tail_ops.size() == n && tail_s0.size() == n &&
                   tail_s1.size() == n),
              "batched init: tail list length mismatch");
  const bool tails_given = !tail_ops.empty();
  // part[0]: no conversion, part[1]: conversion.
  struct Part {
    std::vector<at::Tensor> tensors;
    std::vector<int64_t> dists, seeds, offsets;
    std::vector<double> p0s, p1s;
    std::vector<std::vector<int64_t>> tail_ops;
    std::vector<std::vector<double>> tail_s0, tail_s1;
    std::vector<at::ScalarType> srcs;
  } part[2];
  for (size_t t = 0; t < n; ++t) {
    const auto& src = (*src_dtypes)[t];
    Part& p = part[src.has_value() ? 1 : 0];
    p.tensors.push_back(tensors[t]);
    p.dists.push_back(dists[t]);
    p.p0s.push_back(p0s[t]);
    p.p1s.push_back(p1s[t]);
    p.seeds.push_back(seeds[t]);
    p.offsets.push_back(offsets[t]);
    if (tails_given) {
      p.tail_ops.push_back(tail_ops[t]);
      p.tail_s0.push_back(tail_s0[t]);
      p.tail_s1.push_back(tail_s1[t]);
    }
    if (src.has_value()) {
      p.srcs.push_back(*src);
    }
  }
  // The conversion part is checked before the plain part launches, so a
  // refused batch has filled nothing.
  const CastBatch cast_batch = checkBatchedCast(
      part[1].tensors, part[1].dists, part[1].p1s, part[1].tail_ops,
      part[1].tail_s0, part[1].tail_s1, part[1].srcs);
  if (!part[0].tensors.empty()) {
    batchedInitPlain(std::move(part[0].tensors), std::move(part[0].dists),
                     std::move(part[0].p0s), std::move(part[0].p1s),
                     std::move(part[0].seeds), std::move(part[0].offsets),
                     std::move(part[0].tail_ops), std::move(part[0].tail_s0),
                     std::move(part[0].tail_s1));
  }
  batchedInitCast(part[1].tensors, part[1].dists, part[1].p0s, part[1].p1s,
                  part[1].seeds, part[1].offsets, cast_batch);
}

namespace {

void batchedInitPlain(std::vector<at::Tensor> tensors,
                      std::vector<int64_t> dists,
                      std::vector<double> p0s,
                      std::vector<double> p1s,
                      std::vector<int64_t> seeds,
                      std::vector<int64_t> offsets,
                      std::vector<std::vector<int64_t>> tail_ops,
                      std::vector<std::vector<double>> tail_s0,
                      std::vector<std::vector<double>> tail_s1) {
  const size_t n_tensors = tensors.size();
  TORCH_CHECK(n_tensors > 0 && dists.size() == n_tensors &&
                  p0s.size() == n_tensors && p1s.size() == n_tensors &&
                  seeds.size() == n_tensors && offsets.size() == n_tensors,
              "batched init: list length mismatch");
  // The tail lists are optional as a whole (old call sites pass none).
  TORCH_CHECK((tail_ops.empty() && tail_s0.empty() && tail_s1.empty()) ||
                  (tail_ops.size() == n_tensors &&
                   tail_s0.size() == n_tensors &&
                   tail_s1.size() == n_tensors),
              "batched init: tail list length mismatch");
  bool has_tail = false;
  for (const auto& ops : tail_ops) {
    has_tail = has_tail || !ops.empty();
  }

  const size_t prefix_bytes = sizeof(int64_t) * n_tensors;
  static_assert(sizeof(InitTensorMeta) % alignof(TailProgram) == 0 &&
                    sizeof(int64_t) % alignof(TailProgram) == 0,
                "the tail table must stay aligned behind the metas");
  const size_t tails_off = prefix_bytes + sizeof(InitTensorMeta) * n_tensors;
  const size_t blob_bytes =
      tails_off + (has_tail ? sizeof(TailProgram) * n_tensors : 0);
  at::Tensor host_blob = at::empty(
      {static_cast<int64_t>(blob_bytes)},
      at::TensorOptions().dtype(at::kByte).pinned_memory(true));
  auto* prefix = reinterpret_cast<int64_t*>(host_blob.data_ptr());
  auto* metas = reinterpret_cast<InitTensorMeta*>(
      static_cast<uint8_t*>(host_blob.data_ptr()) + prefix_bytes);

  int64_t total_vblocks = 0;
  for (size_t t = 0; t < n_tensors; ++t) {
    const at::Tensor& x = tensors[t];
    TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
                "batched init: contiguous GPU tensors only");
    InitTensorMeta& mt = metas[t];
    mt.ptr = x.data_ptr();
    mt.n = x.numel();
    mt.dist = static_cast<int32_t>(dists[t]);
    TORCH_CHECK(0 <= mt.dist && mt.dist <= 4, "batched init: bad dist");
    switch (x.scalar_type()) {
      case at::kFloat:
        mt.dtype = 0;
        break;
      case at::kBFloat16:
        mt.dtype = 1;
        break;
      case at::kHalf:
        mt.dtype = 2;
        break;
      default:
        TORCH_CHECK(false, "batched init supports f32/bf16/f16, got ",
                    x.scalar_type());
    }
    const double p0 = p0s[t];
    const double p1 = p1s[t];
    // Same (a, b) mapping as launchRng.
    mt.a = static_cast<float>(p0);
    mt.b = mt.dist == 0 ? static_cast<float>(p1 - p0)
                        : static_cast<float>(p1);
    mt.seed = static_cast<uint64_t>(seeds[t]);
    mt.offset = static_cast<uint64_t>(offsets[t]);
    if (has_tail) {
      TORCH_CHECK(tail_ops[t].empty() || mt.dist <= 2,
                  "batched init: only RNG plans carry a tail");
      reinterpret_cast<TailProgram*>(
          static_cast<uint8_t*>(host_blob.data_ptr()) + tails_off)[t] =
          makeTailProgram(tail_ops[t], tail_s0[t], tail_s1[t], mt.n);
    }
    prefix[t] = total_vblocks;
    total_vblocks += (mt.n + kInitEPB - 1) / kInitEPB;
  }

  at::Tensor dev_blob =
      host_blob.to(tensors[0].device(), /*non_blocking=*/true);
  const int grid =
      static_cast<int>(std::min<int64_t>(total_vblocks, 16384));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (has_tail) {
    hipLaunchKernelGGL(batched_init_kernel<true>, dim3(grid), dim3(kBlock), 0,
                       stream.stream(),
                       static_cast<const uint8_t*>(dev_blob.const_data_ptr()),
                       static_cast<int32_t>(n_tensors), total_vblocks);
  } else {
    hipLaunchKernelGGL(batched_init_kernel<false>, dim3(grid), dim3(kBlock),
                       0, stream.stream(),
                       static_cast<const uint8_t*>(dev_blob.const_data_ptr()),
                       static_cast<int32_t>(n_tensors), total_vblocks);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Schemas are defined by the core extension (csrc/core/tdx_ops.cc); this
// extension contributes the CUDA implementations.
TORCH_LIBRARY_IMPL(tdx, CUDA, m) {
  m.impl("uniform_", tdx_uniform_);
  m.impl("normal_", tdx_normal_);
  m.impl("fill_", tdx_fill_);
  m.impl("zero_", tdx_zero_);
  m.impl("copy_", tdx_copy_);
  m.impl("uniform_shard_", tdx_uniform_shard_);
  m.impl("normal_shard_", tdx_normal_shard_);
  m.impl("bernoulli_", tdx_bernoulli_);
  m.impl("bernoulli_shard_", tdx_bernoulli_shard_);
  m.impl("uniform_shard_win_", tdx_uniform_shard_win_);
  m.impl("normal_shard_win_", tdx_normal_shard_win_);
  m.impl("bernoulli_shard_win_", tdx_bernoulli_shard_win_);
  m.impl("rng_chain_", tdx_rng_chain_);
  m.impl("rng_chain_shard_win_", tdx_rng_chain_shard_win_);
  m.impl("rng_box_", tdx_rng_box_);
  m.impl("patch_box_", tdx_patch_box_);
  m.impl("rng_chain_cast_", tdx_rng_chain_cast_);
  m.impl("rng_chain_cast_shard_win_", tdx_rng_chain_cast_shard_win_);
}

}  // namespace
}  // namespace tdx
