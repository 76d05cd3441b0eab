// AdamWResidentPlan: the device-resident launch plan of one capturable
// AnyPrecisionAdamW param group (anyprecision_adamw_resident.hip;
// docs/anyprecision_adamw.md, "Graph capture").

#pragma once

#include <ATen/ATen.h>

#include <cstdint>
#include <optional>
#include <tuple>
#include <vector>

struct ihipEvent_t;  // hipEvent_t is a pointer to it

namespace tdx {

class AdamWResidentPlan {
 public:
  // The tensor lists of one group, validated as anyprecision_adamw_q8_step
  // validates them; steps[t] is the tensor's state["step"], a 1-element
  // fp32 tensor on the parameters' device, ordinals[t] its index over all
  // param groups. Builds the table and uploads it on the current stream.
  AdamWResidentPlan(std::vector<at::Tensor> params,
                    std::vector<at::Tensor> grads,
                    std::vector<at::Tensor> exp_avgs,
                    std::vector<std::optional<at::Tensor>> exp_avg_scales,
                    std::vector<at::Tensor> exp_avg_sqs,
                    std::vector<std::optional<at::Tensor>> exp_avg_sq_scales,
                    std::vector<std::optional<at::Tensor>> compensations,
                    std::vector<at::Tensor> steps,
                    std::vector<int64_t> ordinals);
  ~AdamWResidentPlan();
  AdamWResidentPlan(const AdamWResidentPlan&) = delete;
  AdamWResidentPlan& operator=(const AdamWResidentPlan&) = delete;

  // Whether these are the gradients the table points at: a pointer
  // comparison, nothing is validated.
  bool matches(const std::vector<at::Tensor>& grads) const;
  // Whether a tensor the plan holds (anything but a gradient) has moved or
  // changed size since the table was built; the plan is then to be rebuilt.
  bool stale() const;
  // New gradients for the same tensors: checks them, rewrites the table's
  // gradient fields and uploads it again.
  void rebind(const std::vector<at::Tensor>& grads);
  // adamw_advance_kernel, then the kResident multi-tensor kernel, on the
  // current stream; nothing else. Exactly one of lr and lr_tensor counts:
  // lr_tensor (1-element fp32 on the parameters' device) when given.
  // found_inf, validated like grad_scale (1-element fp32 on the parameters'
  // device): where it is not zero both kernels leave everything, the step
  // counts included, as it is.
  void step(double lr, const std::optional<at::Tensor>& lr_tensor,
            double beta1, double beta2, double eps, double weight_decay,
            const std::optional<at::Tensor>& grad_scale,
            std::optional<int64_t> sr_seed,
            const std::optional<at::Tensor>& found_inf = std::nullopt);
  // The number of fp64 partials grad_sumsq writes: the grid of its launch.
  int64_t grad_grid() const;
  // grad_sumsq_resident_kernel (grad_norm.hip) over the table on the
  // current stream: the sums of squares of the gradients the table points
  // at, one per workgroup, into partials[offset, offset + grad_grid()) of a
  // contiguous fp64 tensor on the parameters' device. Allocates nothing.
  void grad_sumsq(at::Tensor& partials, int64_t offset);
  // A host copy of the scalar slots as the last step left them:
  // (step_size fp32[n], bias_correction2_sqrt fp32[n], step int64[n],
  // decay fp32[1]). Synchronizes.
  std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> scalars() const;
  int64_t size() const { return static_cast<int64_t>(params_.size()); }

 private:
  void upload(size_t bytes);

  // Every tensor the table points at but the gradients, which the plan
  // does not keep alive: after zero_grad(set_to_none=True) they are free.
  std::vector<at::Tensor> params_, exp_avgs_, exp_avg_sqs_, steps_;
  std::vector<at::ScalarType> grad_dtypes_;
  std::vector<std::optional<at::Tensor>> exp_avg_scales_, exp_avg_sq_scales_,
      compensations_;
  at::Tensor table_host_;  // pinned mirror
  at::Tensor table_;       // device
  size_t meta_bytes_ = 0;  // prefix sums and metas: what rebind uploads
  size_t slots_offset_ = 0;
  int64_t total_vblocks_ = 0;
  // Why sr_seed cannot be given to step(), or nullptr.
  const char* no_stochastic_ = nullptr;
  ihipEvent_t* uploaded_ = nullptr;  // the mirror is free again after it
  // The stream the table was last used on: the allocator is told of every
  // other one (record_stream), so a dropped plan's block is not reused
  // while a kernel still reads it.
  int64_t last_stream_ = 0;
};

}  // namespace tdx
