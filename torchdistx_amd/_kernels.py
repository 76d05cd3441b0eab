# Loader shim for the CDNA4 kernel extension (torchdistx_amd._K).
# Importing this module registers the tdx:: init ops with the dispatcher,
# which the deferred-init replay engine redirects to on GPU targets.
# On machines without the built extension every query degrades to False and
# replay falls back to stock ATen kernels — unless TDX_REQUIRE_NATIVE_INIT
# is set, in which case the C++ redirect fails loudly.

import torch

try:
    from torchdistx_amd import _K  # noqa: F401

    _HAS_K = True
except ImportError:
    _K = None
    _HAS_K = False


def available() -> bool:
    return _HAS_K


def has_init_kernels() -> bool:
    return _HAS_K


def has_anyprecision_adamw() -> bool:
    return _HAS_K and torch.cuda.is_available()


def anyprecision_adamw_(
    param,
    grad,
    exp_avg,
    exp_avg_sq,
    compensation,
    lr,
    beta1,
    beta2,
    eps,
    weight_decay,
    step_size,
    bias_correction2_sqrt,
    grad_scale=None,
):
    _K.anyprecision_adamw_(
        param,
        grad.contiguous(),
        exp_avg,
        exp_avg_sq,
        compensation,
        lr,
        beta1,
        beta2,
        eps,
        weight_decay,
        step_size,
        bias_correction2_sqrt,
        grad_scale,
    )


def anyprecision_adamw_batched_(
    params,
    grads,
    exp_avgs,
    exp_avg_sqs,
    compensations,
    lr,
    beta1,
    beta2,
    eps,
    weight_decay,
    step_sizes,
    bias_correction2_sqrts,
    grad_scale=None,
):
    """One kernel launch updating every listed parameter (see
    csrc/hip/anyprecision_adamw.hip, adamw_batched_kernel)."""
    _K.anyprecision_adamw_batched_(
        params,
        [g.contiguous() for g in grads],
        exp_avgs,
        exp_avg_sqs,
        compensations,
        lr,
        beta1,
        beta2,
        eps,
        weight_decay,
        step_sizes,
        bias_correction2_sqrts,
        grad_scale,
    )


def has_anyprecision_adamw_q8() -> bool:
    return (
        _HAS_K
        and torch.cuda.is_available()
        and hasattr(_K, "has_anyprecision_adamw_q8")
    )


def anyprecision_adamw_q8_(
    params,
    grads,
    exp_avgs,
    exp_avg_scales,
    exp_avg_sqs,
    exp_avg_sq_scales,
    compensations,
    lr,
    beta1,
    beta2,
    eps,
    weight_decay,
    step_sizes,
    bias_correction2_sqrts,
    grad_scale=None,
    sr_seed=None,
    ordinals=None,
    steps=None,
):
    """One kernel launch updating every listed parameter whose exp_avg
    and/or exp_avg_sq are block-scaled fp8 (see
    csrc/hip/anyprecision_adamw_q8.hip; a scale entry is None for a state
    that is not fp8). With sr_seed (an int in [0, 2**63)), bf16 parameters
    are stored with stochastic rounding; ordinals and steps then give each
    tensor's index over all param groups and its integer step count."""
    _K.anyprecision_adamw_q8_(
        params,
        [g.contiguous() for g in grads],
        exp_avgs,
        exp_avg_scales,
        exp_avg_sqs,
        exp_avg_sq_scales,
        compensations,
        lr,
        beta1,
        beta2,
        eps,
        weight_decay,
        step_sizes,
        bias_correction2_sqrts,
        grad_scale,
        sr_seed,
        ordinals,
        steps,
    )


def has_anyprecision_adamw_resident() -> bool:
    return (
        _HAS_K
        and torch.cuda.is_available()
        and hasattr(_K, "has_anyprecision_adamw_resident")
    )


def adamw_resident_plan(params, grads, exp_avgs, exp_avg_scales, exp_avg_sqs,
                        exp_avg_sq_scales, compensations, steps, ordinals):
    """The device-resident launch plan (_K.AdamWResidentPlan; see
    csrc/hip/anyprecision_adamw_resident.hip) of one capturable param group:
    the lists of anyprecision_adamw_q8_, with each tensor's state["step"] (a
    0-dim float32 device tensor) and its index over all param groups in
    place of the host-formed scalars. Validates and uploads once; the plan's
    step(lr, beta1, beta2, eps, weight_decay, grad_scale, sr_seed,
    found_inf) is then two kernel launches and can be captured in a HIP
    graph, and so can its grad_sumsq(partials, offset), the norm pass over
    the same table (see grad_norm_finalize_resident_)."""
    return _K.AdamWResidentPlan(
        params, grads, exp_avgs, exp_avg_scales, exp_avg_sqs,
        exp_avg_sq_scales, compensations, steps, ordinals)


def has_grad_norm() -> bool:
    return (
        _HAS_K
        and torch.cuda.is_available()
        and hasattr(_K, "has_grad_norm")
    )


def grad_norm_clip_coef_(grads, max_norm, out):
    """Global L2 norm of the listed gradients, accumulated in fp64, into
    out[0] and the clip_grad_norm_ coefficient min(max_norm / (norm + 1e-6),
    1) into out[1] (see csrc/hip/grad_norm.hip). out: 2-element float32
    tensor on the gradients' device; nothing returns to the host. The step
    wrappers above take out[1:2] as grad_scale."""
    _K.grad_norm_clip_coef_(grads, max_norm, out)


def grad_norm_finalize_resident_(partials, n_partials, max_norm, loss_scale,
                                 found_inf, out):
    """One workgroup adding partials[:n_partials], the fp64 sums of squares
    the resident plans' grad_sumsq left, into out = [norm, coef, grad_mult,
    found_inf] (4-element float32 on the gradients' device; see
    csrc/hip/grad_norm.hip): the norm of the gradients divided by
    loss_scale, the clip_grad_norm_ coefficient for max_norm (exactly 1 for
    None), coef / loss_scale, and 1 where found_inf is not zero. loss_scale
    and found_inf are 1-element float32 tensors on that device or None.
    AdamWResidentPlan.step takes out[2:3] as grad_scale and out[3:4] as
    found_inf."""
    _K.grad_norm_finalize_resident_(partials, n_partials, max_norm,
                                    loss_scale, found_inf, out)


def has_slowmo() -> bool:
    return (
        _HAS_K
        and torch.cuda.is_available()
        and hasattr(_K, "has_slowmo")
    )


def slowmo_flat_layout(params):
    """(offsets, total_numel), in elements, of the flat buffer the SlowMo
    kernels use for these parameters: every slot starts at a multiple of 8.
    Host only."""
    return _K.slowmo_flat_layout(params)


def slowmo_pack_(params, flat, world_size):
    """One kernel launch writing every listed parameter, divided by
    world_size, into its slot of flat (see csrc/hip/slowmo.hip,
    slowmo_pack_kernel): bitwise what cat(params).div_(world_size) holds."""
    if params:
        with torch.cuda.device(params[0].device):
            _K.slowmo_pack_(params, flat, world_size)


def slowmo_outer_step_(params, prevs, momenta, flat, lrs, slowmo_factor,
                       slowmo_lr):
    """One kernel launch applying the slow-momentum outer step to every
    listed parameter (see csrc/hip/slowmo.hip, slowmo_outer_step_kernel).
    flat: the all-reduced buffer slowmo_pack_ filled, or None to take the
    parameters themselves as the averaged values. lrs: one learning rate
    per tensor."""
    if params:
        with torch.cuda.device(params[0].device):
            _K.slowmo_outer_step_(params, prevs, momenta, flat, lrs,
                                  slowmo_factor, slowmo_lr)
