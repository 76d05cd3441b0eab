// The table the multi-tensor AnyPrecisionAdamW kernel (adamw_q8_kernel,
// anyprecision_adamw_q8.hip) walks, shared between its two owners: the
// per-call blob of anyprecision_adamw_q8_step and the resident table of
// AdamWResidentPlan (anyprecision_adamw_resident.hip).
//
//   per call:  int64 prefix[n] | Q8TensorMeta[n]
//   resident:  int64 prefix[n] | ResidentTensorMeta[n] | ResidentScalars[n]
//              | float decay
//
// prefix[t] is the first virtual block (2048 elements) of tensor t. In the
// resident table everything that changes from step to step is written by
// adamw_advance_kernel on the device: the scalar slots and the decay.

#pragma once

#include <hip/hip_runtime.h>

#include <ATen/ATen.h>

#include <cstdint>
#include <optional>

namespace tdx {
namespace adamw_q8 {

constexpr int kQ8EPB = 2048;      // elements per virtual block
constexpr int kQ8Threads = 256;   // 8 elements per lane
constexpr int kQuantBlock = 256;  // elements per scale
constexpr int kQ8MaxGrid = 16384;

struct Q8TensorMeta {
  void* param;
  const void* grad;
  void* exp_avg;
  void* exp_avg_sq;
  void* compensation;       // nullptr -> plain update
  float* exp_avg_scale;     // nullptr unless exp_avg is fp8
  float* exp_avg_sq_scale;  // nullptr unless exp_avg_sq is fp8
  int64_t n;
  int32_t dt_param, dt_grad, dt_m, dt_v, dt_c;
  float step_size;
  float bias_correction2_sqrt;
  // Stochastic rounding only: the tensor's index over all param groups and
  // its step count, the Philox subsequence (step << 32) | ordinal.
  uint32_t ordinal;
  uint32_t step;
};

struct Q8Header {
  int32_t n_tensors;
  int64_t total_vblocks;
  float beta2, eps, weight_decay;
  float one_minus_beta1, one_minus_beta2, decay;  // host-narrowed
  const float* grad_scale;  // nullptr, or one fp32 every gradient is scaled by
  uint64_t sr_seed;         // Philox key of the stochastic rounding
  // Resident steps under a GradScaler only, else nullptr: one fp32 that,
  // when it is not zero, makes the whole step leave everything as it is.
  const float* found_inf;
};

// What the host bakes into Q8TensorMeta and Q8Header per call, formed on
// the device per step instead.
struct ResidentScalars {
  float step_size;
  float bias_correction2_sqrt;
  uint32_t step;
};

// The base's step_size, bias_correction2_sqrt and step are unused (zero):
// the tensor's state["step"] (0-dim fp32, on the device) and its scalar
// slot stand in for them.
struct ResidentTensorMeta : Q8TensorMeta {
  float* step_ptr;
  uint32_t slot;
};

// The checks of one tensor of a multi-tensor step (plain dense contiguous
// GPU tensors of equal numel, dtypes, scale shapes, what stochastic
// rounding excludes) and its meta with pointers, numel and dtype tags
// filled in; the scalars, ordinal and step are zero.
Q8TensorMeta checkedQ8TensorMeta(const at::Tensor& param,
                                 const at::Tensor& grad,
                                 const at::Tensor& exp_avg,
                                 const std::optional<at::Tensor>& exp_avg_scale,
                                 const at::Tensor& exp_avg_sq,
                                 const std::optional<at::Tensor>& exp_avg_sq_scale,
                                 const std::optional<at::Tensor>& compensation,
                                 bool stochastic);

// Launches the kResident instantiation of adamw_q8_kernel over a resident
// table on `stream`. h.decay is ignored (the table's decay slot is read).
// With h.found_inf the kSkip instantiation, which reads it first.
void launchAdamwQ8Resident(const uint8_t* table, const Q8Header& h,
                           bool stochastic, hipStream_t stream);

}  // namespace adamw_q8

// grad_norm.hip: the resident forms of the gradient norm.

// Workgroups, and fp64 partials written, of launchGradSumsqResident over a
// table of total_vblocks virtual blocks.
int64_t gradSumsqResidentGrid(int64_t total_vblocks);

// grad_sumsq_resident_kernel over a resident table on `stream`: one partial
// sum of squares of the gradients per workgroup into partials[0 .. grid).
// Nothing is launched for a table without virtual blocks.
void launchGradSumsqResident(const uint8_t* table, int32_t n_tensors,
                             int64_t total_vblocks, double* partials,
                             hipStream_t stream);

// The device address of an optional 1-element fp32 tensor on `device`
// (`what` names it in the refusal), or nullptr for none.
const float* deviceScalarPtr(const std::optional<at::Tensor>& scalar,
                             const at::Device& device, const char* what);
}  // namespace tdx
