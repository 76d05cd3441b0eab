// tdx:: op schemas and their CPU reference implementations.
//
// The schemas live here (in the always-loaded core extension) so the CUDA
// implementations in the _K kernel extension can register against them,
// and so the CPU reference paths below are available everywhere — they
// implement the same counter-based value layout as the CDNA4 kernels
// (one Philox4x32-10 call per 16-byte element group, keyed by the group
// index), which is what makes slice materialization testable on GPU-less
// CI. Bitwise determinism is per device type: CPU results match CPU
// results; GPU results match GPU results. (The uniform transform is pure
// integer+fma math and matches across devices in practice; the normal
// transform uses each device's fastest transcendentals.)

#include <cmath>
#include <optional>
#include <type_traits>

#include <ATen/ATen.h>
#include <ATen/ScalarOps.h>
#include <torch/library.h>

#include "box_geometry.h"
#include "deferred_init.h"
#include "philox.h"

namespace tdx {
namespace {

template <typename T>
struct GroupTraits;
template <>
struct GroupTraits<float> {
  static constexpr int kElems = 4;
};
template <>
struct GroupTraits<at::BFloat16> {
  static constexpr int kElems = 8;
};
template <>
struct GroupTraits<at::Half> {
  static constexpr int kElems = 8;
};

// RNG kinds shared with the CDNA4 kernels.
enum class RngKind { kUniform, kNormal, kBernoulli };

// Fills vals[kElems] for element group `g` — the same mapping the CDNA4
// kernels use (csrc/hip/init_kernels.hip rng_kernel). Normals draw from
// Philox4x32-7, uniforms and bernoulli from Philox4x32-10 (see philox.h).
template <typename T, RngKind kKind>
void groupValues(uint64_t g, float a, float b, uint64_t seed,
                 uint64_t offset, float* vals) {
  constexpr bool kNormal = kKind == RngKind::kNormal;
  philox::U4 bits = kNormal ? philox::philox7(seed, g, offset)
                            : philox::philox10(seed, g, offset);
  if constexpr (GroupTraits<T>::kElems == 4) {
    float u[4] = {philox::u32_to_uniform(bits.x),
                  philox::u32_to_uniform(bits.y),
                  philox::u32_to_uniform(bits.z),
                  philox::u32_to_uniform(bits.w)};
    if constexpr (kKind == RngKind::kUniform) {
      for (int j = 0; j < 4; ++j) {
        vals[j] = std::fmaf(u[j], b, a);
      }
    } else if constexpr (kKind == RngKind::kBernoulli) {
      for (int j = 0; j < 4; ++j) {
        vals[j] = u[j] < a ? 1.0f : 0.0f;
      }
    } else {
      for (int p = 0; p < 2; ++p) {
        float u1 = std::max(u[p * 2], 1.1754944e-38f);
        float r = std::sqrt(-2.0f * std::log(u1));
        float ang = 6.2831853071795865f * u[p * 2 + 1];
        vals[p * 2 + 0] = std::fmaf(r * std::cos(ang), b, a);
        vals[p * 2 + 1] = std::fmaf(r * std::sin(ang), b, a);
      }
    }
  } else {
    uint32_t words[4] = {bits.x, bits.y, bits.z, bits.w};
    for (int j = 0; j < 4; ++j) {
      float lo = philox::u16_to_uniform(words[j]);
      float hi = philox::u16_to_uniform(words[j] >> 16);
      if constexpr (kKind == RngKind::kUniform) {
        vals[j * 2 + 0] = std::fmaf(lo, b, a);
        vals[j * 2 + 1] = std::fmaf(hi, b, a);
      } else if constexpr (kKind == RngKind::kBernoulli) {
        vals[j * 2 + 0] = lo < a ? 1.0f : 0.0f;
        vals[j * 2 + 1] = hi < a ? 1.0f : 0.0f;
      } else {
        float u1 = std::max(lo, 1.1754944e-38f);
        float r = std::sqrt(-2.0f * std::log(u1));
        float ang = 6.2831853071795865f * hi;
        vals[j * 2 + 0] = std::fmaf(r * std::cos(ang), b, a);
        vals[j * 2 + 1] = std::fmaf(r * std::sin(ang), b, a);
      }
    }
  }
}

// Writes elements [start, end) of the virtual full tensor into
// out[0 .. end-start), reproducing the group-indexed counter layout.
template <typename T, RngKind kKind>
void cpuPhiloxRange(T* out, int64_t start, int64_t end, float a, float b,
                    uint64_t seed, uint64_t offset) {
  constexpr int kElems = GroupTraits<T>::kElems;
  const int64_t g_first = start / kElems;
  const int64_t g_last = (end + kElems - 1) / kElems;
  float vals[kElems];
  for (int64_t g = g_first; g < g_last; ++g) {
    groupValues<T, kKind>(static_cast<uint64_t>(g), a, b, seed, offset,
                          vals);
    const int64_t base = g * kElems;
    const int64_t lo = std::max(base, start);
    const int64_t hi = std::min(base + kElems, end);
    for (int64_t e = lo; e < hi; ++e) {
      out[e - start] = static_cast<T>(vals[e - base]);
    }
  }
}

template <RngKind kKind>
void cpuPhiloxDispatch(at::Tensor& self, int64_t start, int64_t end,
                       float a, float b, uint64_t seed, uint64_t offset) {
  TORCH_CHECK(self.is_contiguous(),
              "tdx CPU init requires contiguous tensors");
  TORCH_CHECK(self.numel() == end - start,
              "shard numel must equal end - start");
  switch (self.scalar_type()) {
    case at::kFloat:
      cpuPhiloxRange<float, kKind>(self.data_ptr<float>(), start, end, a,
                                     b, seed, offset);
      break;
    case at::kBFloat16:
      cpuPhiloxRange<at::BFloat16, kKind>(self.data_ptr<at::BFloat16>(),
                                            start, end, a, b, seed, offset);
      break;
    case at::kHalf:
      cpuPhiloxRange<at::Half, kKind>(self.data_ptr<at::Half>(), start,
                                        end, a, b, seed, offset);
      break;
    default:
      TORCH_CHECK(false, "tdx init supports float32/bf16/fp16, got ",
                  self.scalar_type());
  }
}

// ---- CPU impls of the full-tensor ops -------------------------------------

at::Tensor& cpu_uniform_(at::Tensor& self, double from, double to,
                         std::optional<at::Generator> generator,
                         std::optional<int64_t> seed,
                         std::optional<int64_t> offset) {
  if (seed.has_value() && offset.has_value()) {
    cpuPhiloxDispatch<RngKind::kUniform>(self, 0, self.numel(),
                             static_cast<float>(from),
                             static_cast<float>(to - from),
                             static_cast<uint64_t>(*seed),
                             static_cast<uint64_t>(*offset));
    return self;
  }
  return self.uniform_(from, to, std::move(generator));
}

at::Tensor& cpu_normal_(at::Tensor& self, double mean, double std,
                        std::optional<at::Generator> generator,
                        std::optional<int64_t> seed,
                        std::optional<int64_t> offset) {
  TORCH_CHECK(std >= 0.0, "normal_ expects std >= 0.0, but found std=", std);
  if (seed.has_value() && offset.has_value()) {
    cpuPhiloxDispatch<RngKind::kNormal>(self, 0, self.numel(), static_cast<float>(mean),
                            static_cast<float>(std),
                            static_cast<uint64_t>(*seed),
                            static_cast<uint64_t>(*offset));
    return self;
  }
  return self.normal_(mean, std, std::move(generator));
}

at::Tensor& cpu_bernoulli_(at::Tensor& self, double p,
                           std::optional<at::Generator> generator,
                           std::optional<int64_t> seed,
                           std::optional<int64_t> offset) {
  TORCH_CHECK(0.0 <= p && p <= 1.0,
              "bernoulli_ expects 0 <= p <= 1, but found p=", p);
  if (seed.has_value() && offset.has_value()) {
    cpuPhiloxDispatch<RngKind::kBernoulli>(
        self, 0, self.numel(), static_cast<float>(p), 0.0f,
        static_cast<uint64_t>(*seed), static_cast<uint64_t>(*offset));
    return self;
  }
  return self.bernoulli_(p, std::move(generator));
}

at::Tensor& cpu_fill_(at::Tensor& self, const at::Scalar& value) {
  return self.fill_(value);
}

at::Tensor& cpu_zero_(at::Tensor& self) {
  return self.zero_();
}

at::Tensor& cpu_copy_(at::Tensor& self, const at::Tensor& src,
                      bool non_blocking) {
  return self.copy_(src, non_blocking);
}

// ---- shard ops (CPU impls; CUDA impls in csrc/hip/init_kernels.hip) -------

at::Tensor& cpu_uniform_shard_(at::Tensor& shard, int64_t start, int64_t end,
                               double from, double to, int64_t seed,
                               int64_t offset) {
  cpuPhiloxDispatch<RngKind::kUniform>(shard, start, end, static_cast<float>(from),
                           static_cast<float>(to - from),
                           static_cast<uint64_t>(seed),
                           static_cast<uint64_t>(offset));
  return shard;
}

at::Tensor& cpu_normal_shard_(at::Tensor& shard, int64_t start, int64_t end,
                              double mean, double std, int64_t seed,
                              int64_t offset) {
  cpuPhiloxDispatch<RngKind::kNormal>(shard, start, end, static_cast<float>(mean),
                          static_cast<float>(std),
                          static_cast<uint64_t>(seed),
                          static_cast<uint64_t>(offset));
  return shard;
}

at::Tensor& cpu_bernoulli_shard_(at::Tensor& shard, int64_t start,
                                 int64_t end, double p, int64_t seed,
                                 int64_t offset) {
  cpuPhiloxDispatch<RngKind::kBernoulli>(
      shard, start, end, static_cast<float>(p), 0.0f,
      static_cast<uint64_t>(seed), static_cast<uint64_t>(offset));
  return shard;
}

// Windowed shard (any-dim slices): the shard is n_blocks contiguous
// global ranges of block_len elements, block r starting at global
// element g_off + r * g_stride — `full.narrow(dim, s, len)` flattened.
// Same counter layout as the flat range, so each block is bitwise the
// matching stretch of the full tensor (CUDA twin:
// csrc/hip/init_kernels.hip rng_shard_window_kernel).
template <RngKind kKind>
void cpuPhiloxWindow(at::Tensor& shard, int64_t n_blocks, int64_t block_len,
                     int64_t g_stride, int64_t g_off, float a, float b,
                     uint64_t seed, uint64_t offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx CPU init requires contiguous tensors");
  TORCH_CHECK(n_blocks >= 0 && block_len >= 0 && g_stride >= block_len &&
                  g_off >= 0,
              "invalid shard window");
  TORCH_CHECK(shard.numel() == n_blocks * block_len,
              "shard numel must equal n_blocks * block_len");
  auto run = [&](auto* out) {
    using T = std::remove_pointer_t<decltype(out)>;
    for (int64_t r = 0; r < n_blocks; ++r) {
      const int64_t lo = g_off + r * g_stride;
      cpuPhiloxRange<T, kKind>(out + r * block_len, lo, lo + block_len, a,
                               b, seed, offset);
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      run(shard.data_ptr<float>());
      break;
    case at::kBFloat16:
      run(shard.data_ptr<at::BFloat16>());
      break;
    case at::kHalf:
      run(shard.data_ptr<at::Half>());
      break;
    default:
      TORCH_CHECK(false, "tdx CPU init supports float32/bf16/fp16, got ",
                  shard.scalar_type());
  }
}

at::Tensor& cpu_uniform_shard_win_(at::Tensor& shard, int64_t n_blocks,
                                   int64_t block_len, int64_t g_stride,
                                   int64_t g_off, double from, double to,
                                   int64_t seed, int64_t offset) {
  cpuPhiloxWindow<RngKind::kUniform>(
      shard, n_blocks, block_len, g_stride, g_off, static_cast<float>(from),
      static_cast<float>(to - from), static_cast<uint64_t>(seed),
      static_cast<uint64_t>(offset));
  return shard;
}

at::Tensor& cpu_normal_shard_win_(at::Tensor& shard, int64_t n_blocks,
                                  int64_t block_len, int64_t g_stride,
                                  int64_t g_off, double mean, double std,
                                  int64_t seed, int64_t offset) {
  cpuPhiloxWindow<RngKind::kNormal>(
      shard, n_blocks, block_len, g_stride, g_off, static_cast<float>(mean),
      static_cast<float>(std), static_cast<uint64_t>(seed),
      static_cast<uint64_t>(offset));
  return shard;
}

at::Tensor& cpu_bernoulli_shard_win_(at::Tensor& shard, int64_t n_blocks,
                                     int64_t block_len, int64_t g_stride,
                                     int64_t g_off, double p, int64_t seed,
                                     int64_t offset) {
  cpuPhiloxWindow<RngKind::kBernoulli>(
      shard, n_blocks, block_len, g_stride, g_off, static_cast<float>(p),
      0.0f, static_cast<uint64_t>(seed), static_cast<uint64_t>(offset));
  return shard;
}

// ---- fused RNG + pointwise-tail ops ---------------------------------------
// CPU form: the Philox fill above, then the same ATen in-place ops the
// unfused replay would run, in order — bitwise equal to it by
// construction. It exists so the planner and slice plumbing are testable
// without a GPU; the CDNA4 kernels apply the tail in registers instead.

void cpuCheckTail(at::IntArrayRef tail_ops, at::ArrayRef<double> tail_s0,
                  at::ArrayRef<double> tail_s1) {
  TORCH_CHECK(tail_ops.size() <= kMaxTailOps &&
                  tail_s0.size() == tail_ops.size() &&
                  tail_s1.size() == tail_ops.size(),
              "rng_chain: at most ", kMaxTailOps,
              " tail ops, with one s0 and one s1 each");
}

void cpuApplyTail(at::Tensor& self, at::IntArrayRef tail_ops,
                  at::ArrayRef<double> tail_s0,
                  at::ArrayRef<double> tail_s1) {
  for (size_t i = 0; i < tail_ops.size(); ++i) {
    const double s0 = tail_s0[i];
    const double s1 = tail_s1[i];
    switch (tail_ops[i]) {
      case TailOp::kErfinv:
        self.erfinv_();
        break;
      case TailOp::kMul:
        // The mul_.Tensor overload with a wrapped number, which is what
        // `t.mul_(2.0)` records: mul_.Scalar rounds the scalar to a
        // 16-bit dtype first on CPU, so it is not in the fusable set.
        self.mul_(at::native::wrapped_scalar_tensor(s0));
        break;
      case TailOp::kAdd:
        self.add_(s0);
        break;
      case TailOp::kSub:
        self.sub_(s0);
        break;
      case TailOp::kClamp:
        self.clamp_(s0, s1);
        break;
      case TailOp::kClampMin:
        self.clamp_min_(s0);
        break;
      case TailOp::kClampMax:
        self.clamp_max_(s0);
        break;
      case TailOp::kNeg:
        self.neg_();
        break;
      case TailOp::kAbs:
        self.abs_();
        break;
      default:
        TORCH_CHECK(false, "rng_chain: bad tail opcode ", tail_ops[i]);
    }
  }
}

at::Tensor& cpu_rng_chain_shard_win_(
    at::Tensor& shard, int64_t n_blocks, int64_t block_len, int64_t g_stride,
    int64_t g_off, int64_t dist, double p0, double p1,
    at::IntArrayRef tail_ops, at::ArrayRef<double> tail_s0,
    at::ArrayRef<double> tail_s1, int64_t full_numel, int64_t seed,
    int64_t offset) {
  // full_numel places ATen's position-dependent f16 mul rounding in the
  // GPU kernels; ATen's CPU kernels have none.
  (void)full_numel;
  cpuCheckTail(tail_ops, tail_s0, tail_s1);
  switch (dist) {
    case 0:
      cpu_uniform_shard_win_(shard, n_blocks, block_len, g_stride, g_off, p0,
                             p1, seed, offset);
      break;
    case 1:
      cpu_normal_shard_win_(shard, n_blocks, block_len, g_stride, g_off, p0,
                            p1, seed, offset);
      break;
    case 2:
      cpu_bernoulli_shard_win_(shard, n_blocks, block_len, g_stride, g_off,
                               p0, seed, offset);
      break;
    default:
      TORCH_CHECK(false, "rng_chain: dist must be 0 (uniform), 1 (normal) "
                         "or 2 (bernoulli), got ", dist);
  }
  cpuApplyTail(shard, tail_ops, tail_s0, tail_s1);
  return shard;
}

// N-d box (csrc/core/box_geometry.h): the shard is prod(extents) runs of
// run_len contiguous global elements each, so the CPU form is the flat
// range fill once per run, then the tail ops on the shard. CUDA twin:
// csrc/hip/init_kernels.hip rng_box_kernel.
template <RngKind kKind>
void cpuPhiloxBox(at::Tensor& shard, const BoxGeometry& geo, float a,
                  float b, uint64_t seed, uint64_t offset) {
  auto run = [&](auto* out) {
    using T = std::remove_pointer_t<decltype(out)>;
    const int64_t rows = geo.rows();
    for (int64_t r = 0; r < rows; ++r) {
      const int64_t lo = geo.rowStart(r);
      cpuPhiloxRange<T, kKind>(out + r * geo.run_len, lo, lo + geo.run_len,
                               a, b, seed, offset);
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      run(shard.data_ptr<float>());
      break;
    case at::kBFloat16:
      run(shard.data_ptr<at::BFloat16>());
      break;
    default:
      run(shard.data_ptr<at::Half>());
      break;
  }
}

at::Tensor& cpu_rng_box_(at::Tensor& shard, at::IntArrayRef extents,
                         at::IntArrayRef g_strides, int64_t run_len,
                         int64_t g_off, int64_t dist, double p0, double p1,
                         at::IntArrayRef tail_ops,
                         at::ArrayRef<double> tail_s0,
                         at::ArrayRef<double> tail_s1, int64_t full_numel,
                         int64_t seed, int64_t offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx CPU init requires contiguous tensors");
  const char* err =
      checkBoxArgs(extents.data(), extents.size(), g_strides.data(),
                   g_strides.size(), run_len, g_off, shard.numel(),
                   full_numel);
  TORCH_CHECK(err == nullptr, "rng_box: ", err);
  cpuCheckTail(tail_ops, tail_s0, tail_s1);
  for (int64_t op : tail_ops) {
    TORCH_CHECK(TailOp::kErfinv <= op && op <= TailOp::kAbs,
                "rng_chain: bad tail opcode ", op);
  }
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
  const auto s = static_cast<uint64_t>(seed);
  const auto o = static_cast<uint64_t>(offset);
  switch (dist) {
    case 0:
      cpuPhiloxBox<RngKind::kUniform>(shard, geo, static_cast<float>(p0),
                                      static_cast<float>(p1 - p0), s, o);
      break;
    case 1:
      cpuPhiloxBox<RngKind::kNormal>(shard, geo, static_cast<float>(p0),
                                     static_cast<float>(p1), s, o);
      break;
    default:
      cpuPhiloxBox<RngKind::kBernoulli>(shard, geo, static_cast<float>(p0),
                                        0.0f, s, o);
      break;
  }
  cpuApplyTail(shard, tail_ops, tail_s0, tail_s1);
  return shard;
}

at::Tensor& cpu_rng_chain_(at::Tensor& self, int64_t dist, double p0,
                           double p1, at::IntArrayRef tail_ops,
                           at::ArrayRef<double> tail_s0,
                           at::ArrayRef<double> tail_s1, int64_t seed,
                           int64_t offset) {
  return cpu_rng_chain_shard_win_(self, 1, self.numel(), self.numel(), 0,
                                  dist, p0, p1, tail_ops, tail_s0, tail_s1,
                                  self.numel(), seed, offset);
}

// ---- RNG + tail + dtype conversion ----------------------------------------
// The element is what rng_chain_ gives at src_dtype (source-dtype Philox
// group, value rounded through src_dtype, tail at src_dtype), converted
// to the shard's dtype. CPU form: exactly that, through a shard-sized
// temporary at src_dtype; the CDNA4 kernels keep the value in registers
// (csrc/hip/init_kernels.hip rng_chain_cast_window_kernel).

bool isCastChainDtype(c10::ScalarType t) {
  return t == at::kFloat || t == at::kBFloat16 || t == at::kHalf;
}

at::Tensor& cpu_rng_chain_cast_shard_win_(
    at::Tensor& shard, at::ScalarType src_dtype, int64_t n_blocks,
    int64_t block_len, int64_t g_stride, int64_t g_off, int64_t dist,
    double p0, double p1, at::IntArrayRef tail_ops,
    at::ArrayRef<double> tail_s0, at::ArrayRef<double> tail_s1,
    int64_t full_numel, int64_t seed, int64_t offset) {
  TORCH_CHECK(isCastChainDtype(src_dtype) &&
                  isCastChainDtype(shard.scalar_type()) &&
                  src_dtype != shard.scalar_type(),
              "rng_chain_cast: two different dtypes of float32/bf16/fp16, "
              "got ", src_dtype, " -> ", shard.scalar_type());
  TORCH_CHECK(shard.is_contiguous(),
              "tdx CPU init requires contiguous tensors");
  at::Tensor src = at::empty(shard.sizes(), shard.options().dtype(src_dtype));
  cpu_rng_chain_shard_win_(src, n_blocks, block_len, g_stride, g_off, dist,
                           p0, p1, tail_ops, tail_s0, tail_s1, full_numel,
                           seed, offset);
  shard.copy_(src);
  return shard;
}

at::Tensor& cpu_rng_chain_cast_(at::Tensor& self, at::ScalarType src_dtype,
                                int64_t dist, double p0, double p1,
                                at::IntArrayRef tail_ops,
                                at::ArrayRef<double> tail_s0,
                                at::ArrayRef<double> tail_s1, int64_t seed,
                                int64_t offset) {
  return cpu_rng_chain_cast_shard_win_(self, src_dtype, 1, self.numel(),
                                       self.numel(), 0, dist, p0, p1,
                                       tail_ops, tail_s0, tail_s1,
                                       self.numel(), seed, offset);
}

// ---- patch: a value step on a contiguous sub-range of the full tensor -----
// The shard elements whose full-tensor index lies in
// [patch_lo, patch_lo + patch_len) take the value that element
// k = g - patch_lo of a contiguous patch_len-element tensor gets from the
// full-tensor op; every other element is left alone. Only the rows of the
// box that meet the patch are visited (rowsMeeting). CUDA twin:
// csrc/hip/init_kernels.hip patch_box_kernel.
at::Tensor& cpu_patch_box_(at::Tensor& shard, at::IntArrayRef extents,
                           at::IntArrayRef g_strides, int64_t run_len,
                           int64_t g_off, int64_t full_numel,
                           int64_t patch_lo, int64_t patch_len, int64_t dist,
                           double p0, double p1, std::optional<int64_t> seed,
                           std::optional<int64_t> offset) {
  TORCH_CHECK(shard.is_contiguous(),
              "tdx CPU init requires contiguous tensors");
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
  const int64_t patch_hi = patch_lo + patch_len;
  const RowRange rows = rowsMeeting(geo, patch_lo, patch_hi);
  if (rows.count() == 0) {
    return shard;
  }
  const auto s = static_cast<uint64_t>(seed.value_or(0));
  const auto o = static_cast<uint64_t>(offset.value_or(0));
  const float a = static_cast<float>(p0);
  const float b = dist == 0 ? static_cast<float>(p1 - p0)
                            : (dist == 1 ? static_cast<float>(p1) : 0.0f);
  at::Tensor flat = shard.view({-1});
  auto run = [&](auto* out) {
    using T = std::remove_pointer_t<decltype(out)>;
    for (int64_t r = rows.first; r < rows.last; ++r) {
      const int64_t rs = geo.rowStart(r);
      const int64_t ga = std::max(rs, patch_lo);
      const int64_t gb = std::min(rs + run_len, patch_hi);
      const int64_t at_shard = r * run_len + (ga - rs);
      switch (dist) {
        case 0:
          cpuPhiloxRange<T, RngKind::kUniform>(out + at_shard, ga - patch_lo,
                                               gb - patch_lo, a, b, s, o);
          break;
        case 1:
          cpuPhiloxRange<T, RngKind::kNormal>(out + at_shard, ga - patch_lo,
                                              gb - patch_lo, a, b, s, o);
          break;
        case 2:
          cpuPhiloxRange<T, RngKind::kBernoulli>(out + at_shard,
                                                 ga - patch_lo, gb - patch_lo,
                                                 a, b, s, o);
          break;
        case 3:
          flat.narrow(0, at_shard, gb - ga).fill_(p0);
          break;
        default:
          flat.narrow(0, at_shard, gb - ga).zero_();
          break;
      }
    }
  };
  switch (shard.scalar_type()) {
    case at::kFloat:
      run(shard.data_ptr<float>());
      break;
    case at::kBFloat16:
      run(shard.data_ptr<at::BFloat16>());
      break;
    default:
      run(shard.data_ptr<at::Half>());
      break;
  }
  return shard;
}

TORCH_LIBRARY(tdx, m) {
  m.def(
      "uniform_(Tensor(a!) self, float from=0., float to=1., *, "
      "Generator? generator=None, int? seed=None, int? offset=None) "
      "-> Tensor(a!)");
  m.def(
      "normal_(Tensor(a!) self, float mean=0., float std=1., *, "
      "Generator? generator=None, int? seed=None, int? offset=None) "
      "-> Tensor(a!)");
  m.def(
      "bernoulli_(Tensor(a!) self, float p=0.5, *, "
      "Generator? generator=None, int? seed=None, int? offset=None) "
      "-> Tensor(a!)");
  m.def("fill_(Tensor(a!) self, Scalar value) -> Tensor(a!)");
  m.def("zero_(Tensor(a!) self) -> Tensor(a!)");
  m.def(
      "copy_(Tensor(a!) self, Tensor src, bool non_blocking=False) "
      "-> Tensor(a!)");
  m.def(
      "uniform_shard_(Tensor(a!) shard, int start, int end, float from=0., "
      "float to=1., *, int seed, int offset) -> Tensor(a!)");
  m.def(
      "normal_shard_(Tensor(a!) shard, int start, int end, float mean=0., "
      "float std=1., *, int seed, int offset) -> Tensor(a!)");
  m.def(
      "bernoulli_shard_(Tensor(a!) shard, int start, int end, float p=0.5, "
      "*, int seed, int offset) -> Tensor(a!)");
  m.def(
      "uniform_shard_win_(Tensor(a!) shard, int n_blocks, int block_len, "
      "int g_stride, int g_off, float from=0., float to=1., *, int seed, "
      "int offset) -> Tensor(a!)");
  m.def(
      "normal_shard_win_(Tensor(a!) shard, int n_blocks, int block_len, "
      "int g_stride, int g_off, float mean=0., float std=1., *, int seed, "
      "int offset) -> Tensor(a!)");
  m.def(
      "bernoulli_shard_win_(Tensor(a!) shard, int n_blocks, int block_len, "
      "int g_stride, int g_off, float p=0.5, *, int seed, int offset) "
      "-> Tensor(a!)");
  // dist: 0 uniform (p0, p1 = from, to), 1 normal (mean, std),
  // 2 bernoulli (p, unused); tail_ops are TailOp codes (deferred_init.h);
  // full_numel is the element count of the full tensor the window is
  // cut from.
  m.def(
      "rng_chain_(Tensor(a!) self, int dist, float p0, float p1, "
      "int[] tail_ops, float[] tail_s0, float[] tail_s1, *, int seed, "
      "int offset) -> Tensor(a!)");
  m.def(
      "rng_chain_shard_win_(Tensor(a!) shard, int n_blocks, int block_len, "
      "int g_stride, int g_off, int dist, float p0, float p1, "
      "int[] tail_ops, float[] tail_s0, float[] tail_s1, int full_numel, "
      "*, int seed, int offset) -> Tensor(a!)");
  // rng_chain_ / rng_chain_shard_win_ drawn (and the tail applied) at
  // src_dtype, stored in the tensor's own, different dtype; both are one
  // of float32/bf16/fp16. Bitwise the src_dtype op followed by `.to()`.
  m.def(
      "rng_chain_cast_(Tensor(a!) self, ScalarType src_dtype, int dist, "
      "float p0, float p1, int[] tail_ops, float[] tail_s0, "
      "float[] tail_s1, *, int seed, int offset) -> Tensor(a!)");
  m.def(
      "rng_chain_cast_shard_win_(Tensor(a!) shard, ScalarType src_dtype, "
      "int n_blocks, int block_len, int g_stride, int g_off, int dist, "
      "float p0, float p1, int[] tail_ops, float[] tail_s0, "
      "float[] tail_s1, int full_numel, *, int seed, int offset) "
      "-> Tensor(a!)");
  // An N-d box of the full tensor in normalized form (box_geometry.h):
  // extents/g_strides per level, outermost first. Empty tail lists mean
  // no tail.
  m.def(
      "rng_box_(Tensor(a!) shard, int[] extents, int[] g_strides, "
      "int run_len, int g_off, int dist, float p0, float p1, "
      "int[] tail_ops, float[] tail_s0, float[] tail_s1, int full_numel, "
      "int seed, int offset) -> Tensor(a!)");
  // A value step on the contiguous range [patch_lo, patch_lo + patch_len)
  // of the full tensor, applied to the part of it the box holds. Geometry
  // as for rng_box_ (a flat range or window is the one-level box it is);
  // dist: 0 uniform, 1 normal, 2 bernoulli, 3 fill (p0), 4 zero. The
  // values are those of the full-tensor op run on a contiguous
  // patch_len-element tensor of the shard's dtype with that seed/offset.
  m.def(
      "patch_box_(Tensor(a!) shard, int[] extents, int[] g_strides, "
      "int run_len, int g_off, int full_numel, int patch_lo, int patch_len, "
      "int dist, float p0, float p1, int? seed, int? offset) -> Tensor(a!)");
}

TORCH_LIBRARY_IMPL(tdx, CPU, m) {
  m.impl("uniform_", cpu_uniform_);
  m.impl("normal_", cpu_normal_);
  m.impl("fill_", cpu_fill_);
  m.impl("zero_", cpu_zero_);
  m.impl("copy_", cpu_copy_);
  m.impl("uniform_shard_", cpu_uniform_shard_);
  m.impl("normal_shard_", cpu_normal_shard_);
  m.impl("bernoulli_", cpu_bernoulli_);
  m.impl("bernoulli_shard_", cpu_bernoulli_shard_);
  m.impl("uniform_shard_win_", cpu_uniform_shard_win_);
  m.impl("normal_shard_win_", cpu_normal_shard_win_);
  m.impl("bernoulli_shard_win_", cpu_bernoulli_shard_win_);
  m.impl("rng_chain_", cpu_rng_chain_);
  m.impl("rng_chain_shard_win_", cpu_rng_chain_shard_win_);
  m.impl("rng_box_", cpu_rng_box_);
  m.impl("patch_box_", cpu_patch_box_);
  m.impl("rng_chain_cast_", cpu_rng_chain_cast_);
  m.impl("rng_chain_cast_shard_win_", cpu_rng_chain_cast_shard_win_);
}

}  // namespace
}  // namespace tdx
