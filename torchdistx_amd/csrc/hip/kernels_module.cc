// Python module for the CDNA4 kernel extension (torchdistx_amd._K).
// Importing this module also registers the tdx:: init ops with the
// dispatcher (TORCH_LIBRARY in init_kernels.hip), which is what the
// deferred-init replay redirect looks for.

#include <torch/extension.h>

#include <variant>

#include "adamw_resident_plan.h"

namespace tdx {

void anyprecision_adamw_step(at::Tensor& param,
                             const at::Tensor& grad,
                             at::Tensor& exp_avg,
                             at::Tensor& exp_avg_sq,
                             std::optional<at::Tensor> compensation,
                             double lr,
                             double beta1,
                             double beta2,
                             double eps,
                             double weight_decay,
                             double step_size,
                             double bias_correction2_sqrt,
                             std::optional<at::Tensor> grad_scale);

void batched_init_launch(std::vector<at::Tensor> tensors,
                         std::vector<int64_t> dists,
                         std::vector<double> p0s,
                         std::vector<double> p1s,
                         std::vector<int64_t> seeds,
                         std::vector<int64_t> offsets,
                         std::vector<std::vector<int64_t>> tail_ops,
                         std::vector<std::vector<double>> tail_s0,
                         std::vector<std::vector<double>> tail_s1,
                         std::optional<std::vector<std::optional<at::ScalarType>>>
                             src_dtypes);

void anyprecision_adamw_batched_step(
    std::vector<at::Tensor> params,
    std::vector<at::Tensor> grads,
    std::vector<at::Tensor> exp_avgs,
    std::vector<at::Tensor> exp_avg_sqs,
    std::vector<std::optional<at::Tensor>> compensations,
    double lr,
    double beta1,
    double beta2,
    double eps,
    double weight_decay,
    std::vector<double> step_sizes,
    std::vector<double> bias_correction2_sqrts,
    std::optional<at::Tensor> grad_scale);

void anyprecision_adamw_q8_step(
    std::vector<at::Tensor> params,
    std::vector<at::Tensor> grads,
    std::vector<at::Tensor> exp_avgs,
    std::vector<std::optional<at::Tensor>> exp_avg_scales,
    std::vector<at::Tensor> exp_avg_sqs,
    std::vector<std::optional<at::Tensor>> exp_avg_sq_scales,
    std::vector<std::optional<at::Tensor>> compensations,
    double lr,
    double beta1,
    double beta2,
    double eps,
    double weight_decay,
    std::vector<double> step_sizes,
    std::vector<double> bias_correction2_sqrts,
    std::optional<at::Tensor> grad_scale,
    std::optional<int64_t> sr_seed,
    std::optional<std::vector<int64_t>> ordinals,
    std::optional<std::vector<int64_t>> steps);

void grad_norm_clip_coef(std::vector<at::Tensor> grads, double max_norm,
                         at::Tensor& out);

int64_t grad_norm_grid_cap();

void grad_norm_finalize_resident(const std::optional<at::Tensor>& partials,
                                 int64_t n_partials,
                                 std::optional<double> max_norm,
                                 const std::optional<at::Tensor>& loss_scale,
                                 const std::optional<at::Tensor>& found_inf,
                                 at::Tensor& out);

std::tuple<std::vector<int64_t>, int64_t> slowmo_flat_layout(
    const std::vector<at::Tensor>& params);

void slowmo_pack(std::vector<at::Tensor> params, at::Tensor& flat,
                 int64_t world_size);

void slowmo_outer_step(std::vector<at::Tensor> params,
                       std::vector<at::Tensor> prevs,
                       std::vector<at::Tensor> momenta,
                       std::optional<at::Tensor> flat,
                       std::vector<double> lrs, double slowmo_factor,
                       double slowmo_lr);

}  // namespace tdx

PYBIND11_MODULE(_K, m) {
  m.doc() = "torchdistx_amd CDNA4 kernels (gfx950)";

  m.def("has_init_kernels", [] { return true; });
  m.def("has_anyprecision_adamw", [] { return true; });
  m.def("has_anyprecision_adamw_batched", [] { return true; });
  m.def("has_anyprecision_adamw_q8", [] { return true; });
  m.def("has_anyprecision_adamw_resident", [] { return true; });
  m.def("has_grad_norm", [] { return true; });
  m.def("has_slowmo", [] { return true; });
  m.def("has_batched_init", [] { return true; });
  m.def("has_fused_chains", [] { return true; });
  m.def("has_box_kernel", [] { return true; });
  m.def("has_cast_chains", [] { return true; });
  m.def("has_patch_kernel", [] { return true; });

  m.def("batched_init_", &tdx::batched_init_launch,
        pybind11::arg("tensors"), pybind11::arg("dists"),
        pybind11::arg("p0s"), pybind11::arg("p1s"), pybind11::arg("seeds"),
        pybind11::arg("offsets"),
        pybind11::arg("tail_ops") = std::vector<std::vector<int64_t>>{},
        pybind11::arg("tail_s0") = std::vector<std::vector<double>>{},
        pybind11::arg("tail_s1") = std::vector<std::vector<double>>{},
        pybind11::arg("src_dtypes") = pybind11::none(),
        "One launch filling every listed tensor with its reduced init "
        "plan (dist: 0 uniform, 1 normal, 2 bernoulli, 3 fill, 4 zero); "
        "bitwise-identical to the per-tensor tdx kernels. The optional "
        "tail lists give each tensor's fused pointwise tail (opcodes and "
        "scalars as in tdx::rng_chain_; empty for none), applied in "
        "registers before the store. The optional src_dtypes list gives, "
        "per tensor, the dtype an RNG plan was recorded at when a "
        "conversion to the tensor's dtype follows it (None for none): "
        "those tensors fill in a second launch that draws at src_dtype "
        "and stores the tensor's dtype (as tdx::rng_chain_cast_).");

  m.def("anyprecision_adamw_batched_",
        &tdx::anyprecision_adamw_batched_step, pybind11::arg("params"),
        pybind11::arg("grads"), pybind11::arg("exp_avgs"),
        pybind11::arg("exp_avg_sqs"), pybind11::arg("compensations"),
        pybind11::arg("lr"), pybind11::arg("beta1"), pybind11::arg("beta2"),
        pybind11::arg("eps"), pybind11::arg("weight_decay"),
        pybind11::arg("step_sizes"),
        pybind11::arg("bias_correction2_sqrts"),
        pybind11::arg("grad_scale") = pybind11::none(),
        "One-launch AdamW update for a whole list of parameters (kahan "
        "optional per tensor via the compensations list).");

  m.def("anyprecision_adamw_q8_", &tdx::anyprecision_adamw_q8_step,
        pybind11::arg("params"), pybind11::arg("grads"),
        pybind11::arg("exp_avgs"), pybind11::arg("exp_avg_scales"),
        pybind11::arg("exp_avg_sqs"), pybind11::arg("exp_avg_sq_scales"),
        pybind11::arg("compensations"), pybind11::arg("lr"),
        pybind11::arg("beta1"), pybind11::arg("beta2"), pybind11::arg("eps"),
        pybind11::arg("weight_decay"), pybind11::arg("step_sizes"),
        pybind11::arg("bias_correction2_sqrts"),
        pybind11::arg("grad_scale") = pybind11::none(),
        pybind11::arg("sr_seed") = pybind11::none(),
        pybind11::arg("ordinals") = pybind11::none(),
        pybind11::arg("steps") = pybind11::none(),
        "One-launch AdamW update for a list of parameters whose exp_avg "
        "and/or exp_avg_sq are block-scaled fp8 (float8_e4m3fn or "
        "float8_e5m2 codes plus one fp32 power-of-two scale per 256 "
        "elements; the scale entry is None for a state that is not fp8). "
        "With sr_seed, bf16 parameters are stored with stochastic rounding: "
        "Philox4x32-10 keyed by sr_seed, per tensor the subsequence "
        "(steps[t] << 32) | ordinals[t].");

  pybind11::class_<tdx::AdamWResidentPlan>(
      m, "AdamWResidentPlan",
      "Device-resident launch plan of one capturable AnyPrecisionAdamW "
      "param group: the multi-tensor table of anyprecision_adamw_q8_ built, "
      "validated and uploaded once, with each tensor's state['step'] (a "
      "1-element float32 device tensor) in place of the scalars the host "
      "bakes in per call. step() is two launches and can be captured in a "
      "HIP graph.")
      .def(pybind11::init<
               std::vector<at::Tensor>, std::vector<at::Tensor>,
               std::vector<at::Tensor>, std::vector<std::optional<at::Tensor>>,
               std::vector<at::Tensor>, std::vector<std::optional<at::Tensor>>,
               std::vector<std::optional<at::Tensor>>, std::vector<at::Tensor>,
               std::vector<int64_t>>(),
           pybind11::arg("params"), pybind11::arg("grads"),
           pybind11::arg("exp_avgs"), pybind11::arg("exp_avg_scales"),
           pybind11::arg("exp_avg_sqs"), pybind11::arg("exp_avg_sq_scales"),
           pybind11::arg("compensations"), pybind11::arg("steps"),
           pybind11::arg("ordinals"))
      .def("matches", &tdx::AdamWResidentPlan::matches, pybind11::arg("grads"),
           "Whether these are the gradients the table points at (pointer "
           "comparison only).")
      .def("stale", &tdx::AdamWResidentPlan::stale,
           "Whether a parameter or state tensor of the plan has moved or "
           "changed size: build a new plan.")
      .def("rebind", &tdx::AdamWResidentPlan::rebind, pybind11::arg("grads"),
           "Point the table at new gradients of the same tensors and upload "
           "it again.")
      .def(
          "step",
          [](tdx::AdamWResidentPlan& plan,
             std::variant<double, at::Tensor> lr, double beta1, double beta2,
             double eps, double weight_decay,
             std::optional<at::Tensor> grad_scale,
             std::optional<int64_t> sr_seed,
             std::optional<at::Tensor> found_inf) {
            const bool as_tensor = std::holds_alternative<at::Tensor>(lr);
            plan.step(as_tensor ? 0.0 : std::get<double>(lr),
                      as_tensor ? std::optional<at::Tensor>(
                                      std::get<at::Tensor>(lr))
                                : std::nullopt,
                      beta1, beta2, eps, weight_decay, grad_scale, sr_seed,
                      found_inf);
          },
          pybind11::arg("lr"), pybind11::arg("beta1"), pybind11::arg("beta2"),
          pybind11::arg("eps"), pybind11::arg("weight_decay"),
          pybind11::arg("grad_scale") = pybind11::none(),
          pybind11::arg("sr_seed") = pybind11::none(),
          pybind11::arg("found_inf") = pybind11::none(),
          "One optimizer step on the current stream: the advance kernel "
          "(step += 1, bias corrections and decay from lr, a float or a "
          "1-element float32 device tensor), then the multi-tensor update. "
          "found_inf: optional 1-element float32 tensor on the parameters' "
          "device; where it is not zero both kernels return before they "
          "touch a step count, a parameter or a state.")
      .def("grad_grid", &tdx::AdamWResidentPlan::grad_grid,
           "The number of float64 partials grad_sumsq writes.")
      .def(
          "grad_sumsq",
          [](tdx::AdamWResidentPlan& plan, at::Tensor partials,
             int64_t offset) { plan.grad_sumsq(partials, offset); },
          pybind11::arg("partials"), pybind11::arg("offset"),
          "One launch on the current stream: the sums of squares of the "
          "gradients the plan's table points at, accumulated in fp64, one "
          "per workgroup into partials[offset : offset + grad_grid()]. "
          "Allocates and copies nothing.")
      .def("scalars", &tdx::AdamWResidentPlan::scalars,
           "Host copies (step_size, bias_correction2_sqrt, step, decay) of "
           "the scalar slots as the last step left them; synchronizes.")
      .def("__len__", &tdx::AdamWResidentPlan::size);

  m.def(
      "anyprecision_adamw_",
      [](at::Tensor param, at::Tensor grad, at::Tensor exp_avg,
         at::Tensor exp_avg_sq, std::optional<at::Tensor> compensation,
         double lr, double beta1, double beta2, double eps,
         double weight_decay, double step_size,
         double bias_correction2_sqrt,
         std::optional<at::Tensor> grad_scale) {
        tdx::anyprecision_adamw_step(
            param, grad, exp_avg, exp_avg_sq, std::move(compensation), lr,
            beta1, beta2, eps, weight_decay, step_size,
            bias_correction2_sqrt, std::move(grad_scale));
      },
      pybind11::arg("param"), pybind11::arg("grad"), pybind11::arg("exp_avg"),
      pybind11::arg("exp_avg_sq"), pybind11::arg("compensation"),
      pybind11::arg("lr"), pybind11::arg("beta1"), pybind11::arg("beta2"),
      pybind11::arg("eps"), pybind11::arg("weight_decay"),
      pybind11::arg("step_size"), pybind11::arg("bias_correction2_sqrt"),
      pybind11::arg("grad_scale") = pybind11::none(),
      "Fused AdamW update of one parameter. grad_scale (here and in the two "
      "list forms): optional 1-element float32 tensor on the parameters' "
      "device; every gradient is multiplied by it in fp32 as it is loaded.");

  m.def(
      "grad_norm_clip_coef_",
      [](std::vector<at::Tensor> grads, double max_norm, at::Tensor out) {
        tdx::grad_norm_clip_coef(std::move(grads), max_norm, out);
      },
      pybind11::arg("grads"), pybind11::arg("max_norm"), pybind11::arg("out"),
      "Global L2 norm of the listed gradients (float32/bf16/fp16, any mix), "
      "accumulated in fp64, into out[0], and the clip_grad_norm_ coefficient "
      "min(max_norm / (norm + 1e-6), 1) into out[1]; out is a 2-element "
      "float32 tensor on the gradients' device. Nothing returns to the host.");
  m.def(
      "grad_norm_finalize_resident_",
      [](std::optional<at::Tensor> partials, int64_t n_partials,
         std::optional<double> max_norm, std::optional<at::Tensor> loss_scale,
         std::optional<at::Tensor> found_inf, at::Tensor out) {
        tdx::grad_norm_finalize_resident(partials, n_partials, max_norm,
                                         loss_scale, found_inf, out);
      },
      pybind11::arg("partials"), pybind11::arg("n_partials"),
      pybind11::arg("max_norm"), pybind11::arg("loss_scale"),
      pybind11::arg("found_inf"), pybind11::arg("out"),
      "One workgroup: adds partials[:n_partials] (AdamWResidentPlan."
      "grad_sumsq) and writes out = [norm, coef, grad_mult, found_inf] "
      "(4-element float32): the norm of the gradients divided by loss_scale, "
      "the clip_grad_norm_ coefficient for max_norm (1 for None), coef / "
      "loss_scale, and 1 where found_inf is not zero. loss_scale and "
      "found_inf: optional 1-element float32 tensors on out's device.");
  m.def("grad_norm_grid_cap", &tdx::grad_norm_grid_cap,
        "Largest grid of the gradient sum-of-squares kernel; more virtual "
        "blocks than this are covered by its grid-stride loop.");

  m.def("slowmo_flat_layout", &tdx::slowmo_flat_layout,
        pybind11::arg("params"),
        "Host only: (offsets, total_numel) of the flat buffer the SlowMo "
        "kernels use for these parameters, in elements; every slot starts "
        "at a multiple of 8 and total_numel is one too.");
  m.def(
      "slowmo_pack_",
      [](std::vector<at::Tensor> params, at::Tensor flat,
         int64_t world_size) {
        tdx::slowmo_pack(std::move(params), flat, world_size);
      },
      pybind11::arg("params"), pybind11::arg("flat"),
      pybind11::arg("world_size"),
      "One launch writing every listed parameter (float32/bf16/fp16, any "
      "mix), divided by world_size as ATen divides by a host scalar, into "
      "its slot of flat (slowmo_flat_layout); the padding is not written.");
  m.def(
      "slowmo_outer_step_",
      [](std::vector<at::Tensor> params, std::vector<at::Tensor> prevs,
         std::vector<at::Tensor> momenta, std::optional<at::Tensor> flat,
         std::vector<double> lrs, double slowmo_factor, double slowmo_lr) {
        tdx::slowmo_outer_step(std::move(params), std::move(prevs),
                               std::move(momenta), std::move(flat),
                               std::move(lrs), slowmo_factor, slowmo_lr);
      },
      pybind11::arg("params"), pybind11::arg("prevs"),
      pybind11::arg("momenta"), pybind11::arg("flat"), pybind11::arg("lrs"),
      pybind11::arg("slowmo_factor"), pybind11::arg("slowmo_lr"),
      "One-launch slow-momentum outer step for a list of parameters: "
      "m <- fma(prev - a, 1/lr, factor * m), prev <- p <- prev - slowmo_lr * "
      "lr * m in fp32, with a the parameter's slot of flat rounded to the "
      "parameter's dtype, or the parameter itself when flat is None. lrs "
      "gives each tensor's learning rate.");
}
