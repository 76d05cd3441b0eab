// Graph-capturable AnyPrecisionAdamW step (docs/anyprecision_adamw.md,
// "Graph capture"): every input that changes from step to step lives on the
// device, and a step is two launches from a plan that outlives it.
//
// anyprecision_adamw_q8_step bakes step_size, bias_correction2_sqrt, the
// step count and 1 - lr * weight_decay into a pinned blob it allocates,
// fills and copies per call; a captured graph would replay step 1 forever.
// Here the table (adamw_q8_table.h) is built and uploaded once per plan:
//
//   adamw_advance_kernel  one lane per tensor. state["step"] (0-dim fp32 on
//                         the device, as in torch's capturable optimizers)
//                         += 1; the bias corrections in fp64 from the new
//                         count and from lr, which is a kernel argument or a
//                         1-element device tensor; each narrowed once to
//                         fp32 into the tensor's scalar slot. Lane 0 writes
//                         the group's decay.
//   adamw_q8_kernel<.., kResident = true>
//                         the multi-tensor kernel of
//                         anyprecision_adamw_q8.hip, same work split and the
//                         same arithmetic, reading the slots.
//
// Both go to the current stream, in this order, so a capture records a
// linear two-node graph, and a replay advances the counters as an eager
// step does. Nothing is allocated, copied or synchronized in step(). The
// plan keeps the parameters and states alive, not the gradients.
//
// Clipping and a GradScaler ride on the same table: grad_sumsq() runs the
// norm pass of grad_norm.hip over the table's gradient fields, and step()
// takes found_inf, a device flag under which both kernels return before
// they touch anything.

#include <hip/hip_runtime.h>

#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>

#include <cstring>
#include <vector>

#include "adamw_q8_table.h"
#include "adamw_resident_plan.h"

namespace tdx {

// grad_norm.hip
const float* gradScalePtr(const std::optional<at::Tensor>& grad_scale,
                          const at::Tensor& param);

namespace {

using namespace adamw_q8;

constexpr int kAdvanceThreads = 256;

// table: the resident layout of adamw_q8_table.h. lr_ptr == nullptr: lr is
// the argument. The three fp64 expressions are the ones
// AnyPrecisionAdamW.step forms on the host, 1 - beta1^t,
// (1 - beta2^t)^(1/2) and lr / bias_correction1, each narrowed to fp32
// once; an fp64 pow within a few ulp leaves them at most one fp32 rounding
// boundary away from the host's. found_inf: nullptr, or the flag of a
// skipped step (adamw_q8_table.h); a lane that reads it set leaves the
// count and its slot alone, so a skipped step does not count, and the
// stochastic-rounding bits, keyed by the count, do not advance either.
__global__ __launch_bounds__(kAdvanceThreads) void adamw_advance_kernel(
    uint8_t* table, int n_tensors, double lr, const float* lr_ptr,
    double beta1, double beta2, double weight_decay,
    const float* found_inf) {
  const int t = blockIdx.x * kAdvanceThreads + threadIdx.x;
  if (t >= n_tensors) {
    return;
  }
  if (found_inf != nullptr && *found_inf != 0.0f) {
    return;
  }
  const ResidentTensorMeta* metas = reinterpret_cast<const ResidentTensorMeta*>(
      table + sizeof(int64_t) * n_tensors);
  ResidentScalars* slots = reinterpret_cast<ResidentScalars*>(
      const_cast<ResidentTensorMeta*>(metas + n_tensors));
  const double lr_now = lr_ptr != nullptr ? static_cast<double>(*lr_ptr) : lr;

  float* step_ptr = metas[t].step_ptr;
  const float step = *step_ptr + 1.0f;  // exact up to 2^24
  *step_ptr = step;
  const double td = static_cast<double>(step);
  const double bias_correction1 = 1.0 - pow(beta1, td);
  const double bias_correction2_sqrt = sqrt(1.0 - pow(beta2, td));

  ResidentScalars sc;
  sc.step_size = static_cast<float>(lr_now / bias_correction1);
  sc.bias_correction2_sqrt = static_cast<float>(bias_correction2_sqrt);
  sc.step = static_cast<uint32_t>(step);
  slots[metas[t].slot] = sc;
  if (t == 0) {
    *reinterpret_cast<float*>(slots + n_tensors) =
        static_cast<float>(1.0 - lr_now * weight_decay);
  }
}

void hipCheck(hipError_t err, const char* what) {
  TORCH_CHECK(err == hipSuccess, "AdamW resident plan: ", what, ": ",
              hipGetErrorString(err));
}

// A gradient as the table may point at it, next to its parameter.
void checkGrad(const at::Tensor& g, const at::Tensor& p,
               at::ScalarType was) {
  TORCH_CHECK(g.is_cuda() && g.device() == p.device() &&
                  g.is_contiguous() &&
                  g.unsafeGetTensorImpl()->has_storage() &&
                  (g.numel() == 0 || g.const_data_ptr() != nullptr) &&
                  g.numel() == p.numel() &&
                  g.scalar_type() == was,
              "AdamW resident plan: rebind takes plain dense contiguous GPU "
              "gradients of the numel and dtype the plan was built with");
}

// The table is about to be used on `stream`. Its block belongs to the
// stream it was allocated on; every other one is reported to the caching
// allocator, which then does not hand the block out again, once the plan
// is dropped, before the work queued on that stream has finished.
template <class Stream>
void usedOn(const at::Tensor& table, int64_t& last_stream,
            const Stream& stream) {
  if (stream.id() != last_stream) {
    table.record_stream(stream.unwrap());
    last_stream = stream.id();
  }
}

}  // namespace

AdamWResidentPlan::AdamWResidentPlan(
    std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
    std::vector<at::Tensor> exp_avgs,
    std::vector<std::optional<at::Tensor>> exp_avg_scales,
    std::vector<at::Tensor> exp_avg_sqs,
    std::vector<std::optional<at::Tensor>> exp_avg_sq_scales,
    std::vector<std::optional<at::Tensor>> compensations,
    std::vector<at::Tensor> steps, std::vector<int64_t> ordinals)
    : params_(std::move(params)),
      exp_avgs_(std::move(exp_avgs)),
      exp_avg_sqs_(std::move(exp_avg_sqs)),
      steps_(std::move(steps)),
      exp_avg_scales_(std::move(exp_avg_scales)),
      exp_avg_sq_scales_(std::move(exp_avg_sq_scales)),
      compensations_(std::move(compensations)) {
  const size_t n = params_.size();
  TORCH_CHECK(n > 0, "AdamW resident plan: empty tensor list");
  TORCH_CHECK(n < (size_t{1} << 31), "AdamW resident plan: too many tensors");
  TORCH_CHECK(grads.size() == n && exp_avgs_.size() == n &&
                  exp_avg_scales_.size() == n && exp_avg_sqs_.size() == n &&
                  exp_avg_sq_scales_.size() == n &&
                  compensations_.size() == n && steps_.size() == n &&
                  ordinals.size() == n,
              "AdamW resident plan: list length mismatch");

  const size_t prefix_bytes = sizeof(int64_t) * n;
  meta_bytes_ = prefix_bytes + sizeof(ResidentTensorMeta) * n;
  slots_offset_ = meta_bytes_;
  const size_t table_bytes =
      slots_offset_ + sizeof(ResidentScalars) * n + sizeof(float);
  table_host_ = at::zeros(
      {static_cast<int64_t>(table_bytes)},
      at::TensorOptions().dtype(at::kByte).pinned_memory(true));
  auto* host = static_cast<uint8_t*>(table_host_.data_ptr());
  auto* prefix = reinterpret_cast<int64_t*>(host);
  auto* metas = reinterpret_cast<ResidentTensorMeta*>(host + prefix_bytes);

  const at::Device device = params_[0].device();
  for (size_t t = 0; t < n; ++t) {
    TORCH_CHECK(params_[t].device() == device,
                "AdamW resident plan: the parameters of a group must be on "
                "one device");
    ResidentTensorMeta& mt = metas[t];
    static_cast<Q8TensorMeta&>(mt) = checkedQ8TensorMeta(
        params_[t], grads[t], exp_avgs_[t], exp_avg_scales_[t],
        exp_avg_sqs_[t], exp_avg_sq_scales_[t], compensations_[t],
        /*stochastic=*/false);
    // What stochastic rounding excludes is a matter of step(): the seed
    // arrives there.
    if (compensations_[t].has_value()) {
      no_stochastic_ = "stochastic rounding and Kahan summation exclude "
                       "each other";
    } else if (params_[t].scalar_type() == at::kHalf) {
      no_stochastic_ = "stochastic rounding stores bf16 parameters (fp32 "
                       "ones as they are); fp16 is not supported";
    }
    grad_dtypes_.push_back(grads[t].scalar_type());
    const at::Tensor& s = steps_[t];
    TORCH_CHECK(s.is_cuda() && s.device() == device &&
                    s.scalar_type() == at::kFloat && s.numel() == 1 &&
                    s.unsafeGetTensorImpl()->has_storage() &&
                    s.const_data_ptr() != nullptr,
                "AdamW resident plan: a step must be a 1-element float32 "
                "tensor on the parameters' device");
    TORCH_CHECK(ordinals[t] >= 0 && ordinals[t] < (int64_t{1} << 32),
                "AdamW resident plan: ordinals must fit in 32 bits");
    mt.ordinal = static_cast<uint32_t>(ordinals[t]);
    mt.step_ptr = s.data_ptr<float>();
    mt.slot = static_cast<uint32_t>(t);
    prefix[t] = total_vblocks_;
    total_vblocks_ += (mt.n + kQ8EPB - 1) / kQ8EPB;
  }

  table_ = at::empty({static_cast<int64_t>(table_bytes)},
                     at::TensorOptions().dtype(at::kByte).device(device));
  last_stream_ = at::cuda::getCurrentCUDAStream().id();  // it owns the block
  hipCheck(hipEventCreateWithFlags(&uploaded_, hipEventDisableTiming),
           "hipEventCreateWithFlags");
  upload(table_bytes);
}

AdamWResidentPlan::~AdamWResidentPlan() {
  if (uploaded_ != nullptr) {
    // The mirror is freed with the plan: let a pending upload read it.
    (void)hipEventSynchronize(uploaded_);
    (void)hipEventDestroy(uploaded_);
  }
}

// The first `bytes` of the mirror to the device, on the current stream.
void AdamWResidentPlan::upload(size_t bytes) {
  auto stream = at::cuda::getCurrentCUDAStream();
  usedOn(table_, last_stream_, stream);
  hipCheck(hipMemcpyAsync(table_.data_ptr(), table_host_.const_data_ptr(),
                          bytes, hipMemcpyHostToDevice, stream.stream()),
           "hipMemcpyAsync");
  hipCheck(hipEventRecord(uploaded_, stream.stream()), "hipEventRecord");
}

bool AdamWResidentPlan::matches(const std::vector<at::Tensor>& grads) const {
  const size_t n = params_.size();
  if (grads.size() != n) {
    return false;
  }
  const auto* metas = reinterpret_cast<const ResidentTensorMeta*>(
      static_cast<const uint8_t*>(table_host_.const_data_ptr()) +
      sizeof(int64_t) * n);
  for (size_t t = 0; t < n; ++t) {
    if (grads[t].const_data_ptr() != metas[t].grad) {
      return false;
    }
  }
  return true;
}

bool AdamWResidentPlan::stale() const {
  const size_t n = params_.size();
  const auto* metas = reinterpret_cast<const ResidentTensorMeta*>(
      static_cast<const uint8_t*>(table_host_.const_data_ptr()) +
      sizeof(int64_t) * n);
  auto moved = [](const std::optional<at::Tensor>& x, const void* p) {
    return x.has_value() && x->const_data_ptr() != p;
  };
  for (size_t t = 0; t < n; ++t) {
    const ResidentTensorMeta& mt = metas[t];
    if (params_[t].const_data_ptr() != mt.param ||
        params_[t].numel() != mt.n ||
        exp_avgs_[t].const_data_ptr() != mt.exp_avg ||
        exp_avg_sqs_[t].const_data_ptr() != mt.exp_avg_sq ||
        steps_[t].const_data_ptr() != mt.step_ptr ||
        moved(compensations_[t], mt.compensation) ||
        moved(exp_avg_scales_[t], mt.exp_avg_scale) ||
        moved(exp_avg_sq_scales_[t], mt.exp_avg_sq_scale)) {
      return true;
    }
  }
  return false;
}

void AdamWResidentPlan::rebind(const std::vector<at::Tensor>& grads) {
  const size_t n = params_.size();
  TORCH_CHECK(grads.size() == n,
              "AdamW resident plan: rebind takes one gradient per tensor "
              "of the plan");
  for (size_t t = 0; t < n; ++t) {
    checkGrad(grads[t], params_[t], grad_dtypes_[t]);
  }
  // A previous upload may not have read the mirror yet.
  hipCheck(hipEventSynchronize(uploaded_), "hipEventSynchronize");
  auto* metas = reinterpret_cast<ResidentTensorMeta*>(
      static_cast<uint8_t*>(table_host_.data_ptr()) + sizeof(int64_t) * n);
  for (size_t t = 0; t < n; ++t) {
    metas[t].grad = grads[t].const_data_ptr();
  }
  upload(meta_bytes_);
}

int64_t AdamWResidentPlan::grad_grid() const {
  return gradSumsqResidentGrid(total_vblocks_);
}

void AdamWResidentPlan::grad_sumsq(at::Tensor& partials, int64_t offset) {
  const int64_t grid = grad_grid();
  TORCH_CHECK(partials.is_cuda() &&
                  partials.device() == params_[0].device() &&
                  partials.scalar_type() == at::kDouble &&
                  partials.is_contiguous() &&
                  partials.unsafeGetTensorImpl()->has_storage(),
              "AdamW resident plan: partials must be a contiguous float64 "
              "tensor on the parameters' device");
  TORCH_CHECK(offset >= 0 && offset <= partials.numel() &&
                  grid <= partials.numel() - offset,
              "AdamW resident plan: partials has ", partials.numel(),
              " elements, the plan writes ", grid, " at offset ", offset);
  if (grid == 0) {
    return;  // every tensor is empty
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  usedOn(table_, last_stream_, stream);
  launchGradSumsqResident(static_cast<const uint8_t*>(table_.const_data_ptr()),
                          static_cast<int32_t>(params_.size()),
                          total_vblocks_,
                          partials.data_ptr<double>() + offset,
                          stream.stream());
}

void AdamWResidentPlan::step(double lr,
                             const std::optional<at::Tensor>& lr_tensor,
                             double beta1, double beta2, double eps,
                             double weight_decay,
                             const std::optional<at::Tensor>& grad_scale,
                             std::optional<int64_t> sr_seed,
                             const std::optional<at::Tensor>& found_inf) {
  const float* lr_ptr = nullptr;
  if (lr_tensor.has_value()) {
    const at::Tensor& l = *lr_tensor;
    TORCH_CHECK(l.is_cuda() && l.device() == params_[0].device() &&
                    l.scalar_type() == at::kFloat && l.numel() == 1 &&
                    l.unsafeGetTensorImpl()->has_storage() &&
                    l.const_data_ptr() != nullptr,
                "AdamW resident plan: a tensor lr must be a 1-element "
                "float32 tensor on the parameters' device");
    lr_ptr = static_cast<const float*>(l.const_data_ptr());
  }
  if (sr_seed.has_value()) {
    TORCH_CHECK(*sr_seed >= 0,
                "AdamW resident plan: sr_seed must not be negative");
    TORCH_CHECK(no_stochastic_ == nullptr, "AdamW resident plan: ",
                no_stochastic_);
  }

  const int n = static_cast<int>(params_.size());
  Q8Header h;
  h.n_tensors = n;
  h.total_vblocks = total_vblocks_;
  h.beta2 = static_cast<float>(beta2);
  h.eps = static_cast<float>(eps);
  h.weight_decay = static_cast<float>(weight_decay);
  h.one_minus_beta1 = static_cast<float>(1.0 - beta1);
  h.one_minus_beta2 = static_cast<float>(1.0 - beta2);
  h.decay = 0.0f;  // the table's slot counts
  h.grad_scale = gradScalePtr(grad_scale, params_[0]);
  h.sr_seed = sr_seed.has_value() ? static_cast<uint64_t>(*sr_seed) : 0;
  h.found_inf = deviceScalarPtr(found_inf, params_[0].device(), "found_inf");

  auto stream = at::cuda::getCurrentCUDAStream();
  usedOn(table_, last_stream_, stream);
  auto* table = static_cast<uint8_t*>(table_.data_ptr());
  hipLaunchKernelGGL(adamw_advance_kernel,
                     dim3((n + kAdvanceThreads - 1) / kAdvanceThreads),
                     dim3(kAdvanceThreads), 0, stream.stream(), table, n, lr,
                     lr_ptr, beta1, beta2, weight_decay, h.found_inf);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if (total_vblocks_ == 0) {
    // Every tensor is empty: only the counters advance.
    return;
  }
  launchAdamwQ8Resident(table, h, sr_seed.has_value(), stream.stream());
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>
AdamWResidentPlan::scalars() const {
  const int64_t n = size();
  const at::Tensor raw =
      table_.slice(0, static_cast<int64_t>(slots_offset_)).cpu();
  const at::Tensor words = raw.view(at::kFloat);  // 3 per slot, then decay
  const at::Tensor slots = words.slice(0, 0, 3 * n).view({n, 3});
  return {slots.select(1, 0).clone(), slots.select(1, 1).clone(),
          slots.select(1, 2).contiguous().view(at::kInt).to(at::kLong),
          words.slice(0, 3 * n).clone()};
}

}  // namespace tdx
