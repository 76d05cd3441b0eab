// Multi-tensor kernels for SlowMomentumOptimizer(use_fused=True)
// (docs/slowmo.md): the pack that feeds the parameter all-reduce and the
// slow-momentum outer step that follows it, each one launch for all
// parameters of all param groups on one device.
//
// slowmo_pack_kernel writes every parameter, multiplied by 1 / world_size,
// into its slot of one flat buffer; after the all-reduce of that buffer
// slowmo_outer_step_kernel reads each slot back as the averaged parameter
// and applies
//     d  = prev - a
//     m' = fma(d, 1/lr, factor * m)
//     q  = fma(-slowmo_lr * lr, m', prev)
//     prev' = p' = round_P(q)
// in fp32, once per element: three tensors read (flat, prev, m), three
// written (m, prev, p). The difference is taken before it is scaled, so the
// cancellation of prev against a costs no precision.
//
// Work split: the prefix-sum table of 2048-element virtual blocks of
// grad_norm.hip, 256-thread workgroups, 8 consecutive elements per lane.
// Nothing is accumulated across blocks, so the grid is one workgroup per
// virtual block: no grid-stride loop, no LDS, no barrier, no atomics. The
// scalars that depend on the param group (1/lr, slowmo_lr * lr) live in the
// per-tensor meta, so one launch serves groups of different learning rates.
// A lane takes 16-byte accesses (one for a 16-bit dtype, two for fp32) on
// every operand whose base pointer allows it and goes element by element on
// a misaligned view and on the lane that straddles the end of a tensor.
//
// Flat buffer: each tensor's slot starts at an element offset that is a
// multiple of 8 (slowmo_flat_layout), so with a 16-byte-aligned buffer every
// slot is vector-aligned for 16-bit and fp32 elements alike. The kernels
// never write the padding between slots: zero-filled at allocation, it
// stays zero under all-reduce.

#include <hip/hip_runtime.h>

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>

#include <climits>
#include <cstring>
#include <tuple>
#include <vector>

// Compiled without the packed fp32 VALU instructions, as grad_norm.hip is.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "adamw_device.h"

namespace tdx {
namespace {

using namespace adamw_device;  // DT, roundBarrier, load8Plain

constexpr int kEPB = 2048;     // elements per virtual block
constexpr int kThreads = 256;  // 8 elements per lane

static_assert(kEPB == kThreads * 8, "8 elements per lane");

struct SlowMoMeta {
  void* param;
  void* prev;       // dtype of param; unused by the pack
  float* momentum;  // unused by the pack
  int64_t flat_off;  // element offset of the slot, a multiple of 8
  int64_t n;
  int32_t dtype;  // a DT, of param and prev
  float inv_lr;   // 1 / lr
  float coef;     // slowmo_lr * lr
};

// The 16-bit code of v rounded to nearest even; tag is kBF16 or kF16.
__device__ __forceinline__ uint32_t narrow16(float v, int tag) {
  v = roundBarrier(v);
  if (tag == static_cast<int>(DT::kBF16)) {
    return __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
  }
  return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
}

__device__ __forceinline__ float widen16(uint32_t code, int tag) {
  if (tag == static_cast<int>(DT::kBF16)) {
    return asFloat(code << 16);
  }
  return static_cast<float>(
      __builtin_bit_cast(_Float16, static_cast<uint16_t>(code)));
}

// v as the dtype `tag` holds it, widened again.
__device__ __forceinline__ float roundTo(float v, int tag) {
  if (tag == static_cast<int>(DT::kF32)) {
    return v;
  }
  return widen16(narrow16(v, tag), tag);
}

// The counterpart of load8Plain: 8 fp32 values of one lane rounded to the
// dtype `tag` and stored at p[e0 ..]. `wide` (all 8 inside the tensor, base
// pointer 16-byte aligned) takes one 16-byte access for a 16-bit dtype and
// two for fp32; otherwise the first `count` elements store one by one and
// nothing past them is touched.
__device__ __forceinline__ void store8Plain(void* p, int tag, int64_t e0,
                                            int count, bool wide,
                                            const float* in) {
  if (tag == static_cast<int>(DT::kF32)) {
    float* q = static_cast<float*>(p) + e0;
    if (wide) {
      f32x4 a, b;
      a.x = in[0]; a.y = in[1]; a.z = in[2]; a.w = in[3];
      b.x = in[4]; b.y = in[5]; b.z = in[6]; b.w = in[7];
      reinterpret_cast<f32x4*>(q)[0] = a;
      reinterpret_cast<f32x4*>(q)[1] = b;
      return;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j < count) {
        q[j] = in[j];
      }
    }
    return;
  }
  uint16_t* q = static_cast<uint16_t*>(p) + e0;
  if (wide) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w[k] = narrow16(in[2 * k], tag) | narrow16(in[2 * k + 1], tag) << 16;
    }
    u32x4 pk;
    pk.x = w[0]; pk.y = w[1]; pk.z = w[2]; pk.w = w[3];
    *reinterpret_cast<u32x4*>(q) = pk;
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < count) {
      q[j] = static_cast<uint16_t>(narrow16(in[j], tag));
    }
  }
}

__device__ __forceinline__ bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 0xf) == 0;
}

// What a lane owns: the tensor and its 8 elements [e0, e0 + count).
struct Lane {
  SlowMoMeta mt;
  int64_t e0;
  int count;  // 0: the lane lies past the end of its tensor
};

// blob layout: int64 prefix[n_tensors] then SlowMoMeta[n_tensors]; no
// listed tensor is empty; gridDim.x is the total number of virtual blocks.
__device__ __forceinline__ Lane findLane(const uint8_t* blob,
                                         int32_t n_tensors) {
  const int64_t* prefix = reinterpret_cast<const int64_t*>(blob);
  const SlowMoMeta* metas =
      reinterpret_cast<const SlowMoMeta*>(blob + sizeof(int64_t) * n_tensors);
  const int64_t vb = blockIdx.x;
  // Largest t with prefix[t] <= vb.
  int lo = 0, hi = n_tensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= vb) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  Lane lane;
  lane.mt = metas[lo];
  lane.e0 = (vb - prefix[lo]) * kEPB + static_cast<int64_t>(threadIdx.x) * 8;
  const int64_t left = lane.mt.n - lane.e0;
  lane.count = left >= 8 ? 8 : (left > 0 ? static_cast<int>(left) : 0);
  return lane;
}

// flat[off + i] = round_flat(widen(p[i]) * inv_world). ATen divides a GPU
// tensor by a host scalar as a product with the scalar's reciprocal formed
// in the compute type (fp32 here), rounded once to fp32 and then to the
// tensor's dtype; the same two roundings here reproduce
// cat(params).div_(world_size) bit for bit. flat is 16-byte aligned.
//
// The dtypes are template arguments of the lane's body, so that each
// combination is straight-line code with all of a lane's loads in flight
// together; the kernel picks the body by the (workgroup-uniform) tags. The
// flat dtype is the parameter's or fp32 (the host checks it).
// kWide: the lane has all 8 elements and the parameter is 16-byte aligned.
template <int kTag, int kFlatTag, bool kWide>
__device__ __forceinline__ void packBody(const Lane& lane, void* flat,
                                         float inv_world) {
  const SlowMoMeta& mt = lane.mt;
  const int count = kWide ? 8 : lane.count;
  float v[8];
  load8Plain(mt.param, kTag, lane.e0, count, kWide, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = v[j] * inv_world;
  }
  store8Plain(flat, kFlatTag, mt.flat_off + lane.e0, count, kWide, v);
}

template <int kTag, int kFlatTag>
__device__ __forceinline__ void packLane(const Lane& lane, void* flat,
                                         float inv_world) {
  // e0 and flat_off are multiples of 8 elements, so the base pointer
  // decides.
  if (lane.count == 8 && aligned16(lane.mt.param)) {
    packBody<kTag, kFlatTag, true>(lane, flat, inv_world);
  } else {
    packBody<kTag, kFlatTag, false>(lane, flat, inv_world);
  }
}

template <int kTag>
__device__ __forceinline__ void packLaneOf(const Lane& lane, void* flat,
                                           int32_t flat_dtype,
                                           float inv_world) {
  if (flat_dtype == kTag) {
    packLane<kTag, kTag>(lane, flat, inv_world);
  } else {
    packLane<kTag, static_cast<int>(DT::kF32)>(lane, flat, inv_world);
  }
}

__global__ __launch_bounds__(kThreads) void slowmo_pack_kernel(
    const uint8_t* __restrict__ blob, int32_t n_tensors,
    void* __restrict__ flat, int32_t flat_dtype, float inv_world) {
  const Lane lane = findLane(blob, n_tensors);
  if (lane.count == 0) {
    return;
  }
  switch (lane.mt.dtype) {
    case static_cast<int>(DT::kF32):
      packLane<static_cast<int>(DT::kF32), static_cast<int>(DT::kF32)>(
          lane, flat, inv_world);
      break;
    case static_cast<int>(DT::kBF16):
      packLaneOf<static_cast<int>(DT::kBF16)>(lane, flat, flat_dtype,
                                              inv_world);
      break;
    default:
      packLaneOf<static_cast<int>(DT::kF16)>(lane, flat, flat_dtype,
                                             inv_world);
      break;
  }
}

// The outer step of the header. flat == nullptr: the parameter itself is
// the averaged value a. Otherwise a is the slot's value rounded to the
// parameter's dtype, which is what copying the flat buffer back into the
// parameter would have stored, and the parameter is only written.
constexpr int kNoFlat = -1;

// kFlatTag: the flat buffer's dtype (the parameter's or fp32), or kNoFlat.
// kWide: the lane has all 8 elements and every pointer is 16-byte aligned.
template <int kTag, int kFlatTag, bool kWide>
__device__ __forceinline__ void outerBody(const Lane& lane, const void* flat,
                                          float factor) {
  constexpr int kF32 = static_cast<int>(DT::kF32);
  const SlowMoMeta& mt = lane.mt;
  const int count = kWide ? 8 : lane.count;

  float a[8], prev[8], m[8];
  if constexpr (kFlatTag == kNoFlat) {
    load8Plain(mt.param, kTag, lane.e0, count, kWide, a);
  } else {
    load8Plain(flat, kFlatTag, mt.flat_off + lane.e0, count, kWide, a);
  }
  load8Plain(mt.prev, kTag, lane.e0, count, kWide, prev);
  load8Plain(mt.momentum, kF32, lane.e0, count, kWide, m);

  float q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float aj = a[j];
    if constexpr (kFlatTag != kNoFlat && kFlatTag != kTag) {
      aj = roundTo(aj, kTag);
    }
    const float d = prev[j] - aj;
    m[j] = __builtin_fmaf(d, mt.inv_lr, factor * m[j]);
    q[j] = __builtin_fmaf(-mt.coef, m[j], prev[j]);
  }
  store8Plain(mt.momentum, kF32, lane.e0, count, kWide, m);
  store8Plain(mt.prev, kTag, lane.e0, count, kWide, q);
  store8Plain(mt.param, kTag, lane.e0, count, kWide, q);
}

template <int kTag, int kFlatTag>
__device__ __forceinline__ void outerLane(const Lane& lane, const void* flat,
                                          float factor) {
  // e0 and flat_off are multiples of 8 elements, so the base pointers
  // decide.
  const SlowMoMeta& mt = lane.mt;
  if (lane.count == 8 && aligned16(mt.param) && aligned16(mt.prev) &&
      aligned16(mt.momentum)) {
    outerBody<kTag, kFlatTag, true>(lane, flat, factor);
  } else {
    outerBody<kTag, kFlatTag, false>(lane, flat, factor);
  }
}

template <int kTag>
__device__ __forceinline__ void outerLaneOf(const Lane& lane,
                                            const void* flat,
                                            int32_t flat_dtype,
                                            float factor) {
  if (flat == nullptr) {
    outerLane<kTag, kNoFlat>(lane, flat, factor);
  } else if (flat_dtype == kTag) {
    outerLane<kTag, kTag>(lane, flat, factor);
  } else {
    outerLane<kTag, static_cast<int>(DT::kF32)>(lane, flat, factor);
  }
}

__global__ __launch_bounds__(kThreads) void slowmo_outer_step_kernel(
    const uint8_t* __restrict__ blob, int32_t n_tensors,
    const void* __restrict__ flat, int32_t flat_dtype, float factor) {
  const Lane lane = findLane(blob, n_tensors);
  if (lane.count == 0) {
    return;
  }
  switch (lane.mt.dtype) {
    case static_cast<int>(DT::kF32):
      outerLaneOf<static_cast<int>(DT::kF32)>(lane, flat, flat_dtype, factor);
      break;
    case static_cast<int>(DT::kBF16):
      outerLaneOf<static_cast<int>(DT::kBF16)>(lane, flat, flat_dtype,
                                               factor);
      break;
    default:
      outerLaneOf<static_cast<int>(DT::kF16)>(lane, flat, flat_dtype, factor);
      break;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

int32_t dtypeTag(at::ScalarType st, const char* what) {
  switch (st) {
    case at::kFloat:
      return static_cast<int32_t>(DT::kF32);
    case at::kBFloat16:
      return static_cast<int32_t>(DT::kBF16);
    case at::kHalf:
      return static_cast<int32_t>(DT::kF16);
    default:
      TORCH_CHECK(false, "slowmo: ", what,
                  " must be float32/bf16/fp16, got ", st);
  }
}

constexpr int64_t roundUp8(int64_t x) { return (x + 7) & ~int64_t{7}; }

void checkPlainGpuTensor(const at::Tensor& t, const at::Device& device,
                         const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.unsafeGetTensorImpl()->has_storage() &&
                  (t.numel() == 0 || t.const_data_ptr() != nullptr),
              "slowmo: ", what,
              " must be a plain dense contiguous GPU tensor");
  TORCH_CHECK(t.device() == device, "slowmo: ", what, " is on ", t.device(),
              ", expected ", device);
}

// The flat buffer as the kernels take it; `needed` elements.
int32_t checkFlat(const at::Tensor& flat, const at::Device& device,
                  int64_t needed) {
  checkPlainGpuTensor(flat, device, "the flat buffer");
  const int32_t tag = dtypeTag(flat.scalar_type(), "the flat buffer");
  TORCH_CHECK(flat.numel() >= needed, "slowmo: the flat buffer holds ",
              flat.numel(), " elements, the layout needs ", needed);
  TORCH_CHECK(flat.numel() == 0 ||
                  (reinterpret_cast<uintptr_t>(flat.const_data_ptr()) & 0xf) ==
                      0,
              "slowmo: the flat buffer must be 16-byte aligned");
  return tag;
}

// The table of one launch, uploaded: prefix then metas, empty tensors left
// out.
struct Table {
  at::Tensor dev_blob;
  int32_t n_tensors = 0;
  int64_t total_vblocks = 0;
};

Table uploadTable(const std::vector<SlowMoMeta>& metas_host,
                  const at::Device& device) {
  Table table;
  const size_t n_tensors = metas_host.size();
  std::vector<int64_t> prefix_host(n_tensors);
  for (size_t t = 0; t < n_tensors; ++t) {
    prefix_host[t] = table.total_vblocks;
    table.total_vblocks += (metas_host[t].n + kEPB - 1) / kEPB;
  }
  // One workgroup per virtual block.
  TORCH_CHECK(table.total_vblocks <= INT_MAX,
              "slowmo: too many elements for one launch");
  table.n_tensors = static_cast<int32_t>(n_tensors);
  if (n_tensors == 0) {
    return table;
  }
  const size_t prefix_bytes = sizeof(int64_t) * n_tensors;
  const size_t blob_bytes = prefix_bytes + sizeof(SlowMoMeta) * n_tensors;
  at::Tensor host_blob = at::empty(
      {static_cast<int64_t>(blob_bytes)},
      at::TensorOptions().dtype(at::kByte).pinned_memory(true));
  auto* blob = static_cast<uint8_t*>(host_blob.data_ptr());
  std::memcpy(blob, prefix_host.data(), prefix_bytes);
  std::memcpy(blob + prefix_bytes, metas_host.data(),
              sizeof(SlowMoMeta) * n_tensors);
  table.dev_blob = host_blob.to(device, /*non_blocking=*/true);
  return table;
}

}  // namespace

std::tuple<std::vector<int64_t>, int64_t> slowmo_flat_layout(
    const std::vector<at::Tensor>& params) {
  std::vector<int64_t> offsets;
  offsets.reserve(params.size());
  int64_t end = 0;
  for (const at::Tensor& p : params) {
    offsets.push_back(roundUp8(end));
    end = offsets.back() + p.numel();
  }
  return {std::move(offsets), roundUp8(end)};
}

void slowmo_pack(std::vector<at::Tensor> params, at::Tensor& flat,
                 int64_t world_size) {
  TORCH_CHECK(world_size >= 1, "slowmo: world_size must be >= 1, got ",
              world_size);
  if (params.empty()) {
    return;
  }
  const at::Device device = params[0].device();
  auto [offsets, total] = slowmo_flat_layout(params);
  const int32_t flat_tag = checkFlat(flat, device, total);

  std::vector<SlowMoMeta> metas_host;
  for (size_t t = 0; t < params.size(); ++t) {
    const at::Tensor& p = params[t];
    checkPlainGpuTensor(p, device, "every parameter");
    SlowMoMeta mt{};
    mt.dtype = dtypeTag(p.scalar_type(), "every parameter");
    if (p.numel() == 0) {
      continue;  // owns no virtual block
    }
    TORCH_CHECK(flat_tag == mt.dtype ||
                    flat_tag == static_cast<int32_t>(DT::kF32),
                "slowmo: the flat buffer must have the promoted dtype of "
                "the parameters; it is ", flat.scalar_type(),
                ", a parameter ", p.scalar_type());
    mt.param = p.data_ptr();
    mt.flat_off = offsets[t];
    mt.n = p.numel();
    metas_host.push_back(mt);
  }
  const Table table = uploadTable(metas_host, device);
  if (table.total_vblocks == 0) {
    return;
  }
  // As ATen forms the reciprocal of a host scalar divisor in fp32.
  const float inv_world = 1.0f / static_cast<float>(world_size);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      slowmo_pack_kernel, dim3(static_cast<uint32_t>(table.total_vblocks)),
      dim3(kThreads), 0, stream.stream(),
      static_cast<const uint8_t*>(table.dev_blob.const_data_ptr()),
      table.n_tensors, flat.data_ptr(), flat_tag, inv_world);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void slowmo_outer_step(std::vector<at::Tensor> params,
                       std::vector<at::Tensor> prevs,
                       std::vector<at::Tensor> momenta,
                       std::optional<at::Tensor> flat,
                       std::vector<double> lrs, double slowmo_factor,
                       double slowmo_lr) {
  const size_t n = params.size();
  TORCH_CHECK(prevs.size() == n && momenta.size() == n && lrs.size() == n,
              "slowmo: list length mismatch");
  if (n == 0) {
    return;
  }
  const at::Device device = params[0].device();
  auto [offsets, total] = slowmo_flat_layout(params);
  const void* flat_ptr = nullptr;
  int32_t flat_tag = static_cast<int32_t>(DT::kF32);
  if (flat.has_value()) {
    flat_tag = checkFlat(*flat, device, total);
    flat_ptr = flat->const_data_ptr();
  }

  std::vector<SlowMoMeta> metas_host;
  for (size_t t = 0; t < n; ++t) {
    const at::Tensor& p = params[t];
    checkPlainGpuTensor(p, device, "every parameter");
    checkPlainGpuTensor(prevs[t], device, "every previous parameter");
    checkPlainGpuTensor(momenta[t], device, "every slow momentum");
    TORCH_CHECK(prevs[t].scalar_type() == p.scalar_type(),
                "slowmo: a previous parameter is ", prevs[t].scalar_type(),
                ", its parameter ", p.scalar_type());
    TORCH_CHECK(momenta[t].scalar_type() == at::kFloat,
                "slowmo: every slow momentum must be float32, got ",
                momenta[t].scalar_type());
    TORCH_CHECK(prevs[t].numel() == p.numel() &&
                    momenta[t].numel() == p.numel(),
                "slowmo: a parameter, its previous value and its momentum "
                "must have equal numel");
    TORCH_CHECK(lrs[t] != 0.0, "slowmo: a learning rate is zero");
    SlowMoMeta mt{};
    mt.dtype = dtypeTag(p.scalar_type(), "every parameter");
    if (p.numel() == 0) {
      continue;  // owns no virtual block
    }
    TORCH_CHECK(!flat.has_value() || flat_tag == mt.dtype ||
                    flat_tag == static_cast<int32_t>(DT::kF32),
                "slowmo: the flat buffer must have the promoted dtype of "
                "the parameters; it is ", flat->scalar_type(),
                ", a parameter ", p.scalar_type());
    mt.param = p.data_ptr();
    mt.prev = prevs[t].data_ptr();
    mt.momentum = static_cast<float*>(momenta[t].data_ptr());
    mt.flat_off = offsets[t];
    mt.n = p.numel();
    mt.inv_lr = static_cast<float>(1.0 / lrs[t]);
    mt.coef = static_cast<float>(slowmo_lr * lrs[t]);
    metas_host.push_back(mt);
  }
  const Table table = uploadTable(metas_host, device);
  if (table.total_vblocks == 0) {
    return;
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      slowmo_outer_step_kernel,
      dim3(static_cast<uint32_t>(table.total_vblocks)), dim3(kThreads), 0,
      stream.stream(),
      static_cast<const uint8_t*>(table.dev_blob.const_data_ptr()),
      table.n_tensors, flat_ptr, flat_tag, static_cast<float>(slowmo_factor));
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace tdx
