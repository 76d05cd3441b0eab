// Global L2 gradient norm and clip coefficient for AnyPrecisionAdamW
// (docs/anyprecision_adamw.md, "Gradient clipping").
//
// grad_sumsq_kernel reads every gradient of every param group once, in one
// launch, and leaves one fp64 partial sum of squares per workgroup;
// grad_norm_finalize_kernel (one workgroup) adds the partials and writes
// [norm, coef] as two fp32 values that stay on the device. The step kernels
// multiply each gradient by coef as they load it, so gradients are never
// rewritten and the host never waits.
//
// Work split: the prefix-sum table of 2048-element virtual blocks that
// adamw_batched_kernel and adamw_q8_kernel walk, here with per-tensor meta
// {ptr, n, dtype}. 256-thread workgroups, grid = min(total_vblocks,
// kGridCap), grid-stride over virtual blocks: which lane adds which element
// in which order is a function of the tensor sizes alone, so the result
// repeats from run to run bit for bit. A lane owns 8 consecutive elements of
// its virtual block (load8Plain: one 16-byte access for a 16-bit dtype, two
// for fp32, element-wise for misaligned views and the lane that straddles
// the end of a tensor).
//
// Arithmetic: each element is widened to fp64 and accumulated with an fp64
// FMA. The square of an fp32 value is exact in fp64 and cannot overflow or
// underflow there, and the sum's error is of order n * 2^-53. The lane
// keeps its accumulator across its grid-stride iterations; at the end the
// wavefront reduces it by lane exchanges on the two dwords (DPP row
// operations, ds_swizzle, readlane), the four wave results meet in 32 bytes
// of LDS behind one barrier, and thread 0 stores the workgroup's partial.
// No atomics, no waiting between workgroups, no completion counters.
//
// Resident forms (docs/anyprecision_adamw.md, "Graph capture"):
// grad_sumsq_resident_kernel is the same pass over the device table of an
// AdamWResidentPlan, one launch per plan into its stretch of a partials
// buffer the optimizer keeps; grad_norm_finalize_resident_kernel adds all
// stretches and writes [norm, coef, grad_mult, found_inf], with the loss
// scale of a GradScaler folded into the multiplier the step kernels load.
// Nothing is allocated, copied or built per call, so the launches can be
// captured, and replay with whatever gradients, scale and flag are there.

#include <hip/hip_runtime.h>

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>

#include <cstring>
#include <vector>

#include "adamw_q8_table.h"

// Compiled without the packed fp32 VALU instructions, as
// anyprecision_adamw_q8.hip is (see there): device code below uses the
// compiler's own types and builtins only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push( \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "adamw_device.h"

namespace tdx {
namespace {

using namespace adamw_device;  // DT, load8Plain

constexpr int kEPB = 2048;     // elements per virtual block
constexpr int kThreads = 256;  // 8 elements per lane
constexpr int kWaves = kThreads / 64;
// 8 workgroups of 4 waves fill a CU; 256 CUs.
constexpr int kGridCap = 2048;

static_assert(kEPB == kThreads * 8, "8 elements per lane");

struct GradMeta {
  const void* ptr;
  int64_t n;
  int32_t dtype;  // a DT
};

template <int kCtrl>
__device__ __forceinline__ double dppAdd(double x) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(
      0, static_cast<int>(static_cast<uint32_t>(b)), kCtrl, 0xf, 0xf, false));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(
      0, static_cast<int>(static_cast<uint32_t>(b >> 32)), kCtrl, 0xf, 0xf,
      false));
  return x + __builtin_bit_cast(double,
                                static_cast<uint64_t>(hi) << 32 | lo);
}

__device__ __forceinline__ double readLane(double x, int lane) {
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(
      static_cast<int>(static_cast<uint32_t>(b)), lane));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(
      static_cast<int>(static_cast<uint32_t>(b >> 32)), lane));
  return __builtin_bit_cast(double, static_cast<uint64_t>(hi) << 32 | lo);
}

// Sum over the 64 lanes of a wave, the same bits in every lane. The
// exchanges are those of the q8 kernel's halfWaveMax (both partners of an
// exchange form the same commutative sum, so the lanes of a group agree
// after each step); the two half-waves then meet through readlane. Every
// lane of the wave must be active.
__device__ __forceinline__ double waveSum(double x) {
  x = dppAdd<0xB1>(x);   // quad_perm [1, 0, 3, 2]
  x = dppAdd<0x4E>(x);   // quad_perm [2, 3, 0, 1]
  x = dppAdd<0x141>(x);  // row_half_mirror
  x = dppAdd<0x140>(x);  // row_mirror
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  // Bit-mask mode: and 0x1f, xor 0x10 (the other row of the half-wave).
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(
      static_cast<int>(static_cast<uint32_t>(b)), 0x401F));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_ds_swizzle(
      static_cast<int>(static_cast<uint32_t>(b >> 32)), 0x401F));
  x += __builtin_bit_cast(double, static_cast<uint64_t>(hi) << 32 | lo);
  return readLane(x, 0) + readLane(x, 32);
}

// Sum over the workgroup, valid in thread 0. `lds` holds kWaves doubles.
__device__ __forceinline__ double blockSum(double x, double* lds) {
  x = waveSum(x);
  if ((threadIdx.x & 63) == 0) {
    lds[threadIdx.x >> 6] = x;
  }
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      total += lds[w];
    }
  }
  return total;
}

// What the sum of squares needs of a table's per-tensor meta.
struct GradRef {
  const void* ptr;
  int64_t n;
  int32_t dtype;
};

__device__ __forceinline__ GradRef gradRef(const GradMeta& mt) {
  return {mt.ptr, mt.n, mt.dtype};
}
__device__ __forceinline__ GradRef gradRef(
    const adamw_q8::ResidentTensorMeta& mt) {
  return {mt.grad, mt.n, mt.dt_grad};
}

// The workgroup's sum of squares over its virtual blocks of a table
// (int64 prefix[n_tensors], then Meta[n_tensors]), valid in thread 0.
template <class Meta>
__device__ __forceinline__ double sumsqOfTable(const uint8_t* table,
                                               int32_t n_tensors,
                                               int64_t total_vblocks,
                                               double* lds) {
  const int64_t* prefix = reinterpret_cast<const int64_t*>(table);
  const Meta* metas =
      reinterpret_cast<const Meta*>(table + sizeof(int64_t) * n_tensors);

  double acc = 0.0;
  for (int64_t vb = blockIdx.x; vb < total_vblocks; vb += gridDim.x) {
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
    const GradRef mt = gradRef(metas[lo]);
    const int64_t e0 =
        (vb - prefix[lo]) * kEPB + static_cast<int64_t>(threadIdx.x) * 8;
    const int64_t left = mt.n - e0;
    const int count = left >= 8 ? 8 : (left > 0 ? static_cast<int>(left) : 0);
    // e0 is a multiple of 8 elements, so the base pointer decides.
    const bool wide =
        count == 8 && (reinterpret_cast<uintptr_t>(mt.ptr) & 0xf) == 0;
    float g[8];
    load8Plain(mt.ptr, mt.dtype, e0, count, wide, g);
    // Elements past the end read as zero and add nothing.
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double d = static_cast<double>(g[j]);
      acc = __builtin_fma(d, d, acc);
    }
  }
  return blockSum(acc, lds);
}

// blob layout: int64 prefix[n_tensors] then GradMeta[n_tensors]. No listed
// tensor is empty. partials has gridDim.x entries; every workgroup owns at
// least one virtual block and writes its own.
__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(
    const uint8_t* __restrict__ blob, int32_t n_tensors,
    int64_t total_vblocks, double* __restrict__ partials) {
  __shared__ double lds[kWaves];
  const double total =
      sumsqOfTable<GradMeta>(blob, n_tensors, total_vblocks, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = total;
  }
}

// The same pass over the resident table of an AdamWResidentPlan
// (adamw_q8_table.h): the virtual blocks, lanes and order of
// grad_sumsq_kernel over the plan's gradients, read through the
// {grad, n, dt_grad} of the metas the step kernel walks. No blob of its
// own: a rebound plan is followed as it is, and a capture records one node
// that needs no host work at replay. An empty tensor shares its prefix with
// its successor and is never found. gridDim.x <= total_vblocks, one
// partial per workgroup.
__global__ __launch_bounds__(kThreads) void grad_sumsq_resident_kernel(
    const uint8_t* __restrict__ table, int32_t n_tensors,
    int64_t total_vblocks, double* __restrict__ partials) {
  __shared__ double lds[kWaves];
  const double total = sumsqOfTable<adamw_q8::ResidentTensorMeta>(
      table, n_tensors, total_vblocks, lds);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = total;
  }
}

// One workgroup. Adds the partials in a fixed order (lane-strided, then the
// tree of blockSum) and writes out[0] = norm, out[1] = the coefficient of
// torch.nn.utils.clip_grad_norm_: min(max_norm / (norm + 1e-6), 1), a NaN
// passing through as it does through clamp(max=1). An infinite norm gives
// 0, a NaN norm NaN. n_partials may be 0 (norm 0).
__global__ __launch_bounds__(kThreads) void grad_norm_finalize_kernel(
    const double* __restrict__ partials, int n_partials, double max_norm,
    float* __restrict__ out) {
  __shared__ double lds[kWaves];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += kThreads) {
    acc += partials[i];
  }
  const double sumsq = blockSum(acc, lds);
  if (threadIdx.x == 0) {
    const double norm = __builtin_sqrt(sumsq);
    const double c = max_norm / (norm + 1e-6);
    const double coef = c < 1.0 ? c : (c != c ? c : 1.0);
    out[0] = static_cast<float>(norm);
    out[1] = static_cast<float>(coef);
  }
}

// The finalize of the resident step, one workgroup: the partials of every
// plan of the optimizer in the order of grad_norm_finalize_kernel, then
// everything a captured step reads, formed in fp64 and narrowed once:
//   out[0] = norm       sqrt(sumsq) / loss_scale, of the unscaled gradients
//   out[1] = coef       the clip formula above on that norm; exactly 1
//                       without clipping (`clip` false; n_partials is 0)
//   out[2] = grad_mult  coef / loss_scale: what the step kernels multiply
//                       each gradient by, one fp32 rounding as under coef
//   out[3] = found_inf  1 if *found_inf_in is not zero, else 0
// loss_scale and found_inf_in may be nullptr (scale 1, nothing found).
__global__ __launch_bounds__(kThreads) void
grad_norm_finalize_resident_kernel(const double* __restrict__ partials,
                                   int n_partials, double max_norm, bool clip,
                                   const float* __restrict__ loss_scale,
                                   const float* __restrict__ found_inf_in,
                                   float* __restrict__ out) {
  __shared__ double lds[kWaves];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += kThreads) {
    acc += partials[i];
  }
  const double sumsq = blockSum(acc, lds);
  if (threadIdx.x == 0) {
    const double inv =
        loss_scale != nullptr ? 1.0 / static_cast<double>(*loss_scale) : 1.0;
    const double norm = __builtin_sqrt(sumsq) * inv;
    double coef = 1.0;
    if (clip) {
      const double c = max_norm / (norm + 1e-6);
      coef = c < 1.0 ? c : (c != c ? c : 1.0);
    }
    out[0] = static_cast<float>(norm);
    out[1] = static_cast<float>(coef);
    out[2] = static_cast<float>(coef * inv);
    out[3] = found_inf_in != nullptr && *found_inf_in != 0.0f ? 1.0f : 0.0f;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// The refusals of the batched step, for one tensor of a list.
void checkPlainGpuTensor(const at::Tensor& t, const at::Device& device,
                         const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.unsafeGetTensorImpl()->has_storage() &&
                  (t.numel() == 0 || t.const_data_ptr() != nullptr),
              "grad norm: ", what,
              " must be a plain dense contiguous GPU tensor");
  TORCH_CHECK(t.device() == device, "grad norm: ", what, " is on ",
              t.device(), ", expected ", device);
}

}  // namespace

// The device address of a step's optional gradient scale: one fp32 element
// on the parameters' device (in practice the coef element of the tensor
// grad_norm_clip_coef fills), or nullptr for none.
const float* deviceScalarPtr(const std::optional<at::Tensor>& scalar,
                             const at::Device& device, const char* what) {
  if (!scalar.has_value()) {
    return nullptr;
  }
  const at::Tensor& s = *scalar;
  TORCH_CHECK(s.is_cuda() && s.unsafeGetTensorImpl()->has_storage() &&
                  s.scalar_type() == at::kFloat && s.numel() == 1 &&
                  s.const_data_ptr() != nullptr,
              what, " must be a 1-element float32 GPU tensor");
  TORCH_CHECK(s.device() == device, what, " is on ", s.device(),
              ", the parameters are on ", device);
  return static_cast<const float*>(s.const_data_ptr());
}

const float* gradScalePtr(const std::optional<at::Tensor>& grad_scale,
                          const at::Tensor& param) {
  return deviceScalarPtr(grad_scale, param.device(), "grad_scale");
}

void grad_norm_clip_coef(std::vector<at::Tensor> grads, double max_norm,
                         at::Tensor& out) {
  TORCH_CHECK(max_norm > 0.0, "grad norm: max_norm must be positive, got ",
              max_norm);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                  out.numel() == 2,
              "grad norm: out must be a 2-element float32 GPU tensor");
  checkPlainGpuTensor(out, out.device(), "out");

  std::vector<int64_t> prefix_host;
  std::vector<GradMeta> metas_host;
  int64_t total_vblocks = 0;
  for (const at::Tensor& g : grads) {
    checkPlainGpuTensor(g, out.device(), "every gradient");
    GradMeta mt{};
    switch (g.scalar_type()) {
      case at::kFloat:
        mt.dtype = static_cast<int32_t>(DT::kF32);
        break;
      case at::kBFloat16:
        mt.dtype = static_cast<int32_t>(DT::kBF16);
        break;
      case at::kHalf:
        mt.dtype = static_cast<int32_t>(DT::kF16);
        break;
      default:
        TORCH_CHECK(false,
                    "grad norm: gradients must be float32/bf16/fp16, got ",
                    g.scalar_type());
    }
    if (g.numel() == 0) {
      continue;  // owns no virtual block
    }
    mt.ptr = g.const_data_ptr();
    mt.n = g.numel();
    prefix_host.push_back(total_vblocks);
    metas_host.push_back(mt);
    total_vblocks += (mt.n + kEPB - 1) / kEPB;
  }

  auto stream = at::cuda::getCurrentCUDAStream();
  const int grid = static_cast<int>(std::min<int64_t>(total_vblocks, kGridCap));
  at::Tensor partials = at::empty(
      {grid}, at::TensorOptions().dtype(at::kDouble).device(out.device()));
  if (grid > 0) {
    const size_t n_tensors = metas_host.size();
    const size_t prefix_bytes = sizeof(int64_t) * n_tensors;
    const size_t blob_bytes = prefix_bytes + sizeof(GradMeta) * n_tensors;
    at::Tensor host_blob = at::empty(
        {static_cast<int64_t>(blob_bytes)},
        at::TensorOptions().dtype(at::kByte).pinned_memory(true));
    auto* blob = static_cast<uint8_t*>(host_blob.data_ptr());
    std::memcpy(blob, prefix_host.data(), prefix_bytes);
    std::memcpy(blob + prefix_bytes, metas_host.data(),
                sizeof(GradMeta) * n_tensors);
    at::Tensor dev_blob = host_blob.to(out.device(), /*non_blocking=*/true);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(kThreads), 0,
                       stream.stream(),
                       static_cast<const uint8_t*>(dev_blob.const_data_ptr()),
                       static_cast<int32_t>(n_tensors), total_vblocks,
                       static_cast<double*>(partials.data_ptr()));
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  // With no element at all the partial list is empty: norm 0, and no
  // zero-block launch above.
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(kThreads), 0,
                     stream.stream(),
                     static_cast<const double*>(partials.const_data_ptr()),
                     grid, max_norm, static_cast<float*>(out.data_ptr()));
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

int64_t grad_norm_grid_cap() { return kGridCap; }

static_assert(kEPB == adamw_q8::kQ8EPB,
              "the resident table counts the norm pass's virtual blocks");

int64_t gradSumsqResidentGrid(int64_t total_vblocks) {
  return std::min<int64_t>(total_vblocks, kGridCap);
}

void launchGradSumsqResident(const uint8_t* table, int32_t n_tensors,
                             int64_t total_vblocks, double* partials,
                             hipStream_t stream) {
  const int grid = static_cast<int>(gradSumsqResidentGrid(total_vblocks));
  if (grid == 0) {
    return;  // every tensor is empty: no partial, and no zero-block launch
  }
  hipLaunchKernelGGL(grad_sumsq_resident_kernel, dim3(grid), dim3(kThreads),
                     0, stream, table, n_tensors, total_vblocks, partials);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

void grad_norm_finalize_resident(const std::optional<at::Tensor>& partials,
                                 int64_t n_partials,
                                 std::optional<double> max_norm,
                                 const std::optional<at::Tensor>& loss_scale,
                                 const std::optional<at::Tensor>& found_inf,
                                 at::Tensor& out) {
  TORCH_CHECK(!max_norm.has_value() || *max_norm > 0.0,
              "grad norm: max_norm must be positive, got ", *max_norm);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
                  out.numel() == 4,
              "grad norm: out must be a 4-element float32 GPU tensor");
  checkPlainGpuTensor(out, out.device(), "out");
  TORCH_CHECK(n_partials >= 0 && n_partials < (int64_t{1} << 31),
              "grad norm: n_partials out of range: ", n_partials);
  const double* partials_ptr = nullptr;
  if (n_partials > 0) {
    TORCH_CHECK(partials.has_value() &&
                    partials->scalar_type() == at::kDouble &&
                    partials->numel() >= n_partials,
                "grad norm: partials must be a float64 tensor of at least "
                "n_partials elements");
    checkPlainGpuTensor(*partials, out.device(), "partials");
    partials_ptr = static_cast<const double*>(partials->const_data_ptr());
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      grad_norm_finalize_resident_kernel, dim3(1), dim3(kThreads), 0,
      stream.stream(), partials_ptr, static_cast<int>(n_partials),
      max_norm.value_or(0.0), max_norm.has_value(),
      deviceScalarPtr(loss_scale, out.device(), "loss_scale"),
      deviceScalarPtr(found_inf, out.device(), "found_inf"),
      static_cast<float*>(out.data_ptr()));
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

}  // namespace tdx
