# AnyPrecisionAdamW — AdamW with user-controlled optimizer-state dtypes and
# optional Kahan-compensated weight updates, so full-bf16 training keeps
# fp32-quality weight updates.
#
# Capability parity with the reference implementation
# (/root/reference/src/python/torchdistx/optimizers/anyprecision_optimizer.py:19-182):
# same constructor surface and defaults, same state layout ("step", "exp_avg",
# "exp_avg_sq", optional "compensation"), and bitwise equivalence with
# torch.optim.AdamW when every dtype is fp32 and Kahan summation is off.
#
# MI355X-native redesign: the update is written against torch 2.10's AdamW
# op sequence (lerp_/addcmul_/addcdiv_) so the fp32 path is bitwise-identical
# to torch.optim.AdamW on this stack, and a fused single-kernel CDNA4 step
# (torchdistx_amd._K.anyprecision_adamw_) is used on ROCm GPUs when available
# instead of the ~10 separate elementwise kernels the eager path launches.

import numbers

import torch
from torch.optim.optimizer import Optimizer


def _local_view(t):
    """DTensor (FSDP2) parameters carry their data in a plain contiguous
    local shard; the fused kernel runs on that shard directly — an
    elementwise optimizer step on the local shard is exactly the sharded
    step. Other tensors pass through unchanged."""
    if t is None:
        return None
    try:
        from torch.distributed.tensor import DTensor
    except ImportError:
        return t
    if isinstance(t, DTensor):
        return t.to_local()
    return t


# Fused-eligible tensors below this element count batch into one kernel
# launch per group; larger ones keep the per-tensor vectorized kernel.
_BATCH_MAX_NUMEL = 1 << 20


# Block-scaled fp8 optimizer states (docs/anyprecision_adamw.md, "8-bit
# states"): codes in the state tensor, one fp32 power-of-two scale per
# _Q8_BLOCK consecutive elements in state["<name>_scale"].
_Q8_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)
_Q8_BLOCK = 256
_FP8_DTYPES = _Q8_DTYPES + tuple(
    getattr(torch, name)
    for name in ("float8_e4m3fnuz", "float8_e5m2fnuz", "float8_e8m0fnu")
    if hasattr(torch, name)
)


def _check_state_dtypes(momentum_dtype, variance_dtype, compensation_dtype):
    for name, dtype in (("momentum_dtype", momentum_dtype),
                        ("variance_dtype", variance_dtype)):
        if dtype in _FP8_DTYPES and dtype not in _Q8_DTYPES:
            raise ValueError(
                f"{name}={dtype} is not supported: the 8-bit optimizer "
                "states are the OCP formats torch.float8_e4m3fn and "
                "torch.float8_e5m2 (gfx950 converts these natively; the "
                "fnuz formats are not supported)"
            )
    if compensation_dtype in _FP8_DTYPES:
        raise ValueError(
            f"compensation_buffer_dtype={compensation_dtype} is not "
            "supported: the Kahan compensation buffer must be float32, "
            "bfloat16 or float16 (fp8 is for exp_avg and exp_avg_sq only)"
        )


def _check_stochastic_rounding(group):
    seed = group["stochastic_rounding_seed"]
    if seed is not None and (isinstance(seed, bool)
                             or not isinstance(seed, numbers.Integral)
                             or not 0 <= seed < 2**63):
        raise ValueError(
            f"stochastic_rounding_seed={seed!r} is not an integer in "
            "[0, 2**63)"
        )
    if group["stochastic_rounding"] and group["use_kahan_summation"]:
        raise ValueError(
            "stochastic_rounding=True and use_kahan_summation=True exclude "
            "each other: they are two answers to the same question (keeping "
            "updates below half a bf16 ulp), and stochastic rounding keeps "
            "no compensation buffer"
        )


def _q8_scale(state_tensor):
    """Fresh scales for a zero-initialized fp8 state: 1.0 per quant block."""
    n_blocks = -(-state_tensor.numel() // _Q8_BLOCK)
    return torch.ones(n_blocks, dtype=torch.float32,
                      device=state_tensor.device)


def _kernel_loaded() -> bool:
    try:
        from torchdistx_amd import _kernels

        return _kernels.has_anyprecision_adamw()
    except Exception:
        return False


def _q8_kernel_loaded() -> bool:
    try:
        from torchdistx_amd import _kernels

        return _kernels.has_anyprecision_adamw_q8()
    except Exception:
        return False


def _resident_kernel_loaded() -> bool:
    try:
        from torchdistx_amd import _kernels

        return _kernels.has_anyprecision_adamw_resident()
    except Exception:
        return False


_CAPTURE_WARM_UP = (
    "run one eager step first and keep gradients in place, "
    "`zero_grad(set_to_none=False)`"
)


def _grad_norm_kernel_loaded() -> bool:
    try:
        from torchdistx_amd import _kernels

        return _kernels.has_grad_norm()
    except Exception:
        return False


_GRAD_NORM_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _fused_grad_norm_refusal(grads):
    """Why the fused norm kernel (csrc/hip/grad_norm.hip) cannot take this
    gradient list, or None if it can."""
    if not _grad_norm_kernel_loaded():
        return ("the kernel extension torchdistx_amd._K (with "
                "grad_norm_clip_coef_) is not loaded")
    for g in grads:
        if g.device.type != "cuda":
            return f"a gradient is on {g.device.type}, not on a GPU"
        if g.device != grads[0].device:
            return "the gradients are on more than one GPU"
        if (g.layout != torch.strided or torch.utils._python_dispatch
                .is_traceable_wrapper_subclass(g)):
            return "a gradient is not a plain dense tensor"
        if g.dtype not in _GRAD_NORM_DTYPES:
            return f"a gradient is {g.dtype}, not float32/bfloat16/float16"
        if not g.is_contiguous():
            return "a gradient is non-contiguous"
    return None


def _is_dtensor(t) -> bool:
    try:
        from torch.distributed.tensor import DTensor
    except ImportError:
        return False
    return isinstance(t, DTensor)


def _fused_step_available(p: torch.Tensor) -> bool:
    p = _local_view(p)
    if p.device.type != "cuda":
        return False
    # Non-DTensor wrapper subclasses (functorch wrappers, fake modes, ...)
    # are storage-less: handing them to the raw HIP kernel would
    # dereference a null device pointer. They take the eager op sequence,
    # which dispatches through the subclass correctly.
    if torch.utils._python_dispatch.is_traceable_wrapper_subclass(p):
        return False
    return _kernel_loaded()


class AnyPrecisionAdamW(Optimizer):
    """AdamW with user-chosen state dtypes and optional Kahan summation.

    Args:
        params: iterable of parameters or dicts defining parameter groups.
        lr: learning rate (default: 1e-3).
        betas: coefficients for the running averages of the gradient and its
            square (default: (0.9, 0.999)).
        eps: denominator fuzz term (default: 1e-8).
        weight_decay: decoupled (AdamW-style) weight decay (default: 0.0).
        use_kahan_summation: keep a compensation buffer so low-precision
            weight updates accumulate with effectively higher precision
            (default: False).
        momentum_dtype: dtype of ``exp_avg`` (default: torch.float32).
        variance_dtype: dtype of ``exp_avg_sq`` (default: torch.bfloat16).
            Either may also be ``torch.float8_e4m3fn`` or
            ``torch.float8_e5m2``: the state then holds fp8 codes next to
            one fp32 power-of-two scale per 256 elements
            (``state["exp_avg_scale"]`` / ``state["exp_avg_sq_scale"]``),
            and exists on the fused GPU path only — ``step`` raises
            ``RuntimeError`` where that path cannot run.
        compensation_buffer_dtype: dtype of the Kahan compensation buffer
            (default: torch.bfloat16).
        use_fused: True forces the fused single-kernel CDNA4 step and
            raises ``RuntimeError`` if it cannot run (so a benchmark can
            never silently measure the eager path); False forbids it;
            None (default) uses it automatically on GPU tensors when the
            kernel extension is loaded. DTensor (FSDP2) parameters are
            unwrapped to their local shard for the fused step. The fused
            step computes in fp32 and rounds once per state store, so it
            is close to but not bitwise-identical with the eager op
            sequence.
        max_grad_norm: clip the global L2 norm of all gradients (every
            param group, as ``clip_grad_norm_`` over ``model.parameters()``)
            to this value inside ``step`` (default: None, no clipping). On
            the fused path a HIP kernel accumulates the norm in fp64 and
            leaves the clip coefficient on the device, and the step kernels
            scale each gradient by it as they load it. ``p.grad`` is never
            modified — the one deliberate difference from calling
            ``torch.nn.utils.clip_grad_norm_`` before ``step``. After a
            step, ``grad_norm`` and ``grad_clip_coef`` hold the norm and the
            coefficient as 0-dim fp32 device tensors (no host
            synchronisation). DTensor parameters are not supported yet.
        stochastic_rounding: store bf16 parameters with stochastic
            rounding (default: False): the stored value is unbiased, so
            updates far below half a bf16 ulp accumulate in expectation,
            with no compensation buffer. fp32 parameters of the group are
            stored as always; an fp16 parameter raises ``ValueError``.
            Excludes ``use_kahan_summation``. Like the fp8 states it
            exists on the fused GPU path only — ``step`` raises
            ``RuntimeError`` where that path cannot run.
        stochastic_rounding_seed: integer in ``[0, 2**63)`` keying the
            random bits, which are a function of (seed, step, index of the
            parameter over all groups, element index) alone. None (default)
            draws one from torch's default CPU generator at construction,
            so ``torch.manual_seed`` decides it; without stochastic
            rounding nothing is drawn. Data-parallel replicas need the
            same seed on every rank — pass it explicitly or seed the ranks
            identically — and then stay bitwise in sync. The seed is part
            of ``state_dict()["param_groups"]``.
        capturable: make ``step`` safe to capture in a HIP graph
            (``torch.cuda.graph``) (default: False). ``state["step"]`` is
            then a 0-dim fp32 tensor on the parameter's device, ``lr`` may
            be a 1-element fp32 tensor on that device (change it in place
            for a schedule), and a step is two kernel launches from a
            device-resident plan kept per param group, with no per-tensor
            host work: one kernel advances the step counts and forms the
            bias corrections on the device, the multi-tensor kernel applies
            the update. Composes with Kahan summation, fp8 states and
            stochastic rounding. When every param group is capturable,
            ``max_grad_norm`` and a ``torch.amp.GradScaler`` run inside
            the step and can be captured with it: the norm is taken over
            the resident plans, the loss scale is folded into the
            multiplier the step kernels load, and a step whose
            ``found_inf`` is set skips itself on the device without
            counting. ``GradScaler.step`` then finds
            ``_step_supports_amp_scaling`` and runs no unscale pass and no
            ``found_inf.item()``; for a captured step set ``grad_scale``
            and ``found_inf`` on the optimizer yourself, as 1-element fp32
            device tensors that persist.
            Exists on the fused GPU path only — ``step`` raises
            ``RuntimeError`` where that path cannot run. Run one eager step
            before capturing and keep the gradient tensors in place
            (``zero_grad(set_to_none=False)``): see
            docs/anyprecision_adamw.md, "Graph capture".
    """

    def __init__(
        self,
        params,
        lr=1e-3,
        betas=(0.9, 0.999),
        eps=1e-8,
        weight_decay=0.0,
        use_kahan_summation=False,
        momentum_dtype=torch.float32,
        variance_dtype=torch.bfloat16,
        compensation_buffer_dtype=torch.bfloat16,
        use_fused=None,
        max_grad_norm=None,
        stochastic_rounding=False,
        stochastic_rounding_seed=None,
        capturable=False,
    ):
        if max_grad_norm is not None and (
                isinstance(max_grad_norm, bool)
                or not isinstance(max_grad_norm, numbers.Real)
                or not max_grad_norm > 0):
            raise ValueError(
                f"max_grad_norm={max_grad_norm!r} is not a positive number"
            )
        defaults = dict(
            lr=lr,
            betas=betas,
            eps=eps,
            weight_decay=weight_decay,
            use_kahan_summation=use_kahan_summation,
            momentum_dtype=momentum_dtype,
            variance_dtype=variance_dtype,
            compensation_buffer_dtype=compensation_buffer_dtype,
            stochastic_rounding=stochastic_rounding,
            stochastic_rounding_seed=stochastic_rounding_seed,
            capturable=capturable,
        )
        _check_state_dtypes(
            momentum_dtype, variance_dtype, compensation_buffer_dtype
        )
        _check_stochastic_rounding(defaults)
        super().__init__(params, defaults)
        for group in self.param_groups:
            _check_state_dtypes(
                group["momentum_dtype"],
                group["variance_dtype"],
                group["compensation_buffer_dtype"],
            )
            _check_stochastic_rounding(group)
            for p in group["params"]:
                if p.dtype in _FP8_DTYPES:
                    raise ValueError(
                        f"parameter dtype {p.dtype} is not supported: fp8 "
                        "is for the optimizer states exp_avg and "
                        "exp_avg_sq only"
                    )
        unseeded = [g for g in self.param_groups
                    if g["stochastic_rounding_seed"] is None]
        if unseeded and any(g["stochastic_rounding"]
                            for g in self.param_groups):
            # One draw from the default CPU generator, and only when
            # stochastic rounding is on.
            seed = int(torch.randint(0, 2**63 - 1, (1,)).item())
            for group in unseeded:
                group["stochastic_rounding_seed"] = seed
        self.use_fused = use_fused
        # Diagnostic: number of parameter updates that took the fused
        # CDNA4 kernel (lets tests and benchmarks assert the fast path
        # actually ran).
        self._fused_steps = 0
        # Optimizer-wide, not per group: the norm spans all param groups.
        self.max_grad_norm = max_grad_norm
        # Views of the [norm, coef] tensor of the last step.
        self.grad_norm = None
        self.grad_clip_coef = None
        # capturable=True: per index of a param group, the parameters that
        # had gradients when its device-resident plan was built, and the
        # plan (_K.AdamWResidentPlan).
        self._resident_plans = {}
        # The resident clipped / amp step: the fp64 partials all plans
        # share, the 4-element fp32 [norm, coef, grad_mult, found_inf], and
        # the views of it handed out (grad_norm, grad_clip_coef and the two
        # the step kernels read).
        self._norm_buffers = (None, None, None)

    @property
    def _step_supports_amp_scaling(self):
        """What ``torch.amp.GradScaler.step`` asks: whether ``step`` unscales
        and skips by itself, from the ``grad_scale`` and ``found_inf``
        tensors the scaler then sets on the optimizer. It does when every
        param group is ``capturable=True``."""
        return all(g.get("capturable", False) for g in self.param_groups)

    def load_state_dict(self, state_dict):
        """Base-class restore, then re-cast the optimizer states to their
        configured dtypes: ``torch.optim.Optimizer.load_state_dict`` casts
        floating state tensors to the *parameter* dtype, which would
        silently destroy the any-precision state layout (e.g. a bf16
        compensation buffer next to fp32 weights)."""
        super().load_state_dict(state_dict)
        # The resident plans point at the state tensors replaced here.
        self._resident_plans.clear()
        for group in self.param_groups:
            for p in group["params"]:
                state = self.state.get(p)
                if not state:
                    continue
                state["exp_avg"] = state["exp_avg"].to(group["momentum_dtype"])
                state["exp_avg_sq"] = state["exp_avg_sq"].to(
                    group["variance_dtype"]
                )
                if "compensation" in state:
                    state["compensation"] = state["compensation"].to(
                        group["compensation_buffer_dtype"]
                    )
        # Block-scaled fp8 states come back bit for bit: codes and fp32
        # scales are taken from the incoming dict itself, not from the base
        # class's detour through the parameter dtype (an fp16 parameter
        # cannot even represent a scale of 2^-100).
        by_index = {}
        for saved_group, group in zip(state_dict["param_groups"],
                                      self.param_groups):
            by_index.update(zip(saved_group["params"], group["params"]))
        for index, saved in state_dict["state"].items():
            state = self.state.get(by_index.get(index))
            if not state:
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                if key not in saved or saved[key].dtype not in _Q8_DTYPES:
                    continue
                for k, dtype in ((key, saved[key].dtype),
                                 (key + "_scale", torch.float32)):
                    state[k] = saved[k].detach().to(
                        device=state[k].device, dtype=dtype, copy=True)

    def _check_q8_can_run(self, p, kernel_loaded, sr=False):
        """fp8 states exist on the fused path only (torch has no fp8
        ``lerp_``/``addcmul_``, and an eager emulation would be a second
        definition of the format), and so does stochastic rounding (``sr``;
        its random bits are defined by the kernel): name why it cannot
        run."""
        reason = None
        if self.use_fused is False:
            reason = "use_fused=False forbids the fused step"
        elif _is_dtensor(p):
            reason = ("the parameter is a DTensor, " + (
                "which stochastic rounding does not cover yet" if sr else
                "and a per-local-shard scale tensor has no DTensor "
                "placement yet"))
        elif p.device.type != "cuda":
            reason = f"the parameter is on {p.device.type}, not on a GPU"
        elif not kernel_loaded:
            reason = ("the kernel extension torchdistx_amd._K (with "
                      "anyprecision_adamw_q8_) is not loaded")
        elif torch.utils._python_dispatch.is_traceable_wrapper_subclass(p):
            reason = "the parameter is a storage-less wrapper subclass"
        elif not p.is_contiguous():
            reason = "the parameter is non-contiguous"
        if reason is not None:
            what = ("stochastic rounding (stochastic_rounding=True) needs"
                    if sr else
                    "fp8 optimizer states (momentum_dtype/variance_dtype = "
                    "float8_e4m3fn/float8_e5m2) need")
            raise RuntimeError(
                f"{what} the fused AnyPrecisionAdamW step, but {reason}"
            )

    def _check_capturable_can_run(self, p, grad):
        """capturable=True exists on the fused path only (the eager op
        sequence keeps its step count on the host): name why it cannot
        run. fp8 states and stochastic rounding have refused DTensors
        before this is called."""
        tensors = [_local_view(p), _local_view(grad)]
        reason = None
        if p.device.type != "cuda":
            reason = f"the parameter is on {p.device.type}, not on a GPU"
        elif not _resident_kernel_loaded():
            reason = ("the kernel extension torchdistx_amd._K (with "
                      "AdamWResidentPlan) is not loaded")
        elif any(torch.utils._python_dispatch.is_traceable_wrapper_subclass(t)
                 for t in tensors):
            reason = ("the parameter or its gradient is a storage-less "
                      "wrapper subclass")
        elif grad.is_sparse:
            reason = "the gradient is sparse"
        elif not all(t.is_contiguous() for t in tensors):
            reason = "the parameter or its gradient is non-contiguous"
        if reason is not None:
            raise RuntimeError(
                "capturable=True needs the fused AnyPrecisionAdamW step, "
                f"but {reason}"
            )

    def _build_resident_plan(self, group, with_grad, first_ordinal):
        """State of the parameters that have none yet, the refusals, and
        the group's _K.AdamWResidentPlan."""
        from torchdistx_amd import _kernels

        momentum_dtype = group["momentum_dtype"]
        variance_dtype = group["variance_dtype"]
        sr = group.get("stochastic_rounding", False)
        q8 = (sr or momentum_dtype in _Q8_DTYPES
              or variance_dtype in _Q8_DTYPES)
        if sr:
            _check_stochastic_rounding(group)
        ordinal_of = {id(p): first_ordinal + i
                      for i, p in enumerate(group["params"])}
        cols = [[] for _ in range(9)]
        for p in with_grad:
            if q8:
                self._check_q8_can_run(p, _q8_kernel_loaded(), sr)
            self._check_capturable_can_run(p, p.grad)
            if sr and p.dtype == torch.float16:
                raise ValueError(
                    "stochastic_rounding=True stores bfloat16 "
                    "parameters (float32 ones as they are); a float16 "
                    "parameter is not supported"
                )
            state = self.state[p]
            if len(state) == 0:
                state["step"] = torch.zeros(
                    (), dtype=torch.float32, device=p.device)
                state["exp_avg"] = torch.zeros_like(p, dtype=momentum_dtype)
                state["exp_avg_sq"] = torch.zeros_like(
                    p, dtype=variance_dtype)
                if group["use_kahan_summation"]:
                    state["compensation"] = torch.zeros_like(
                        p, dtype=group["compensation_buffer_dtype"])
                if momentum_dtype in _Q8_DTYPES:
                    state["exp_avg_scale"] = _q8_scale(state["exp_avg"])
                if variance_dtype in _Q8_DTYPES:
                    state["exp_avg_sq_scale"] = _q8_scale(
                        state["exp_avg_sq"])
            row = (p, p.grad, state["exp_avg"], state.get("exp_avg_scale"),
                   state["exp_avg_sq"], state.get("exp_avg_sq_scale"),
                   state.get("compensation") if group["use_kahan_summation"]
                   else None, state["step"])
            for col, t in zip(cols, row):
                col.append(_local_view(t))
            cols[8].append(ordinal_of[id(p)])
        return _kernels.adamw_resident_plan(*cols)

    def _resident_plan_for(self, index, group, first_ordinal,
                           refused="capturable=True: "):
        """The resident plan of a capturable=True group, pointing at this
        step's gradients: (plan, number of parameters, their device), or
        None for a group without gradients. While the stream is
        capturing a plan cannot be built or rebound: RuntimeError, headed by
        `refused`, before anything is touched."""
        if self.use_fused is False:
            raise RuntimeError(
                "capturable=True needs the fused AnyPrecisionAdamW step, "
                "but use_fused=False forbids the fused step"
            )
        with_grad = [p for p in group["params"] if p.grad is not None]
        if not with_grad:
            return None
        # Before the plan and the states: a refused step leaves nothing.
        lr = group["lr"]
        if isinstance(lr, torch.Tensor) and (
                lr.device != with_grad[0].device
                or lr.dtype != torch.float32 or lr.numel() != 1):
            raise RuntimeError(
                "capturable=True takes lr as a Python float or a 1-element "
                f"float32 tensor on the parameters' device, not {lr.dtype} "
                f"with {lr.numel()} elements on {lr.device}"
            )
        kept, plan, unwrap = self._resident_plans.get(
            index, (None, None, False))
        grads = [p.grad for p in with_grad]
        if unwrap:
            grads = [_local_view(g) for g in grads]
        same = (plan is not None and len(kept) == len(with_grad)
                and all(a is b for a, b in zip(kept, with_grad))
                and not plan.stale())
        if not (same and plan.matches(grads)):
            # The first GPU query of the step: CPU parameters are refused
            # without one.
            if with_grad[0].device.type == "cuda" and \
                    torch.cuda.is_current_stream_capturing():
                raise RuntimeError(
                    f"{refused}the step's device-resident plan would "
                    "have to be " + ("rebound to new gradient tensors"
                                     if same else "built")
                    + f" while the stream is capturing; {_CAPTURE_WARM_UP}"
                )
            if same:
                plan.rebind(grads)
            else:
                plan = self._build_resident_plan(
                    group, with_grad, first_ordinal)
                unwrap = any(_is_dtensor(p) for p in with_grad)
                self._resident_plans[index] = (with_grad, plan, unwrap)
        return plan, len(with_grad), grads[0].device

    @staticmethod
    def _launch_resident_plan(plan, group, grad_scale, found_inf=None):
        beta1, beta2 = group["betas"]
        plan.step(
            group["lr"], beta1, beta2, group["eps"], group["weight_decay"],
            grad_scale,
            group["stochastic_rounding_seed"]
            if group.get("stochastic_rounding", False) else None,
            *(() if found_inf is None else (found_inf,)))

    def _capturable_group_step(self, index, group, first_ordinal, clip_on):
        """One step of a capturable=True group: gather the gradients, check
        them against the group's resident plan, launch it. clip_on(device)
        is the clip coefficient there, or None."""
        got = self._resident_plan_for(index, group, first_ordinal)
        if got is None:
            return
        plan, n, device = got
        self._launch_resident_plan(plan, group, clip_on(device))
        self._fused_steps += n

    def _resident_scaled_step(self, with_grad, loss_scale, found_inf):
        """One step with everything a captured step may need on the device
        (docs/anyprecision_adamw.md, "Graph capture"): every group with
        gradients is capturable=True and its gradients are on one GPU. With
        max_grad_norm each group's resident plan leaves its fp64 partial
        sums of squares in one shared buffer; a one-workgroup finalize folds
        them, the clip formula and 1 / loss_scale into the multiplier the
        step kernels load, next to found_inf, which makes the step skip
        itself. Inside and outside capture the same launches."""
        from torchdistx_amd import _kernels

        clip = self.max_grad_norm is not None
        device = _local_view(with_grad[0][0]).device
        capturing = torch.cuda.is_current_stream_capturing()
        refused = ("max_grad_norm cannot be captured before one eager step "
                   "with it: " if clip else "capturable=True: ")
        for name, t in (("grad_scale", loss_scale), ("found_inf", found_inf)):
            if t is not None and not (
                    isinstance(t, torch.Tensor) and t.device == device
                    and t.dtype == torch.float32 and t.numel() == 1):
                raise RuntimeError(
                    f"{name} must be a 1-element float32 tensor on the "
                    f"parameters' device {device}"
                )
        plans, ordinal = [], 0
        for index, (group, ps) in enumerate(
                zip(self.param_groups, with_grad)):
            if ps:
                plan, n, _ = self._resident_plan_for(
                    index, group, ordinal, refused)
                plans.append((plan, group, n))
            ordinal += len(group["params"])

        # One fp64 partial per workgroup of every plan's norm pass; its size
        # changes only when a plan is built anew.
        n_partials = sum(plan.grad_grid() for plan, _, _ in plans) \
            if clip else 0
        partials, out, views = self._norm_buffers
        fits = (partials is not None and partials.device == device
                and partials.numel() == n_partials)
        if not fits or out is None or out.device != device:
            if capturing:
                raise RuntimeError(
                    f"{refused}the gradient-norm buffers would have to be "
                    "allocated while the stream is capturing; "
                    f"{_CAPTURE_WARM_UP}"
                )
            if not fits:
                partials = torch.empty(
                    n_partials, dtype=torch.float64, device=device)
            if out is None or out.device != device:
                out = torch.tensor([0.0, 1.0, 1.0, 0.0], device=device)
                views = (out[0], out[1], out[2:3], out[3:4])
            self._norm_buffers = (partials, out, views)
        norm, coef, mult, skip = views
        # The same views every step: read them after a replay.
        self.grad_norm, self.grad_clip_coef = norm, coef

        offset = 0
        if clip:
            for plan, _, _ in plans:
                plan.grad_sumsq(partials, offset)
                offset += plan.grad_grid()
        _kernels.grad_norm_finalize_resident_(
            partials, offset, self.max_grad_norm, loss_scale, found_inf, out)
        for plan, group, n in plans:
            self._launch_resident_plan(
                plan, group, mult, None if found_inf is None else skip)
            self._fused_steps += n

    def _clip_norm_and_coef(self):
        """The 2-element fp32 tensor [norm, coef] of this step's gradients:
        their global L2 norm and the coefficient of ``clip_grad_norm_``,
        ``min(max_grad_norm / (norm + 1e-6), 1)``. Stays on the device."""
        grads = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if _is_dtensor(p) or _is_dtensor(p.grad):
                    raise RuntimeError(
                        "max_grad_norm is not supported for DTensor "
                        "parameters or gradients yet: the local sum of "
                        "squares would need a reduction across the mesh"
                    )
                if p.grad.is_sparse:
                    raise RuntimeError(
                        "AnyPrecisionAdamW does not support sparse gradients"
                    )
                grads.append(_local_view(p.grad))
        if not grads:
            return torch.tensor([0.0, 1.0])
        refusal = (
            "use_fused=False forbids it" if self.use_fused is False
            else _fused_grad_norm_refusal(grads)
        )
        if refusal is None:
            from torchdistx_amd import _kernels

            out = torch.empty(2, dtype=torch.float32, device=grads[0].device)
            _kernels.grad_norm_clip_coef_(grads, self.max_grad_norm, out)
            return out
        if self.use_fused is True:
            raise RuntimeError(
                "use_fused=True, but the fused gradient norm for "
                f"max_grad_norm cannot run: {refusal}. Pass use_fused=None "
                "to fall back to torch.nn.utils.get_total_norm "
                "automatically."
            )
        # As torch.nn.utils.clip_grad_norm_ forms them.
        total = torch.nn.utils.get_total_norm(grads, 2.0)
        coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)
        return torch.stack([total, coef]).to(torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        """Performs a single optimization step."""
        if closure is not None:
            with torch.enable_grad():
                closure()

        # As torch's fused optimizers: set by torch.amp.GradScaler.step
        # around this call (or by the user, as persistent tensors, for a
        # captured step); grad_scale is None after an explicit unscale_.
        loss_scale = getattr(self, "grad_scale", None)
        found_inf = getattr(self, "found_inf", None)
        amp = loss_scale is not None or found_inf is not None
        if amp:
            for index, group in enumerate(self.param_groups):
                if not group.get("capturable", False):
                    raise RuntimeError(
                        "grad_scale / found_inf (torch.amp.GradScaler) are "
                        "set on the optimizer, but param group "
                        f"{index} is not capturable=True: unscaling and "
                        "skipping inside the step exist on the resident "
                        "path only"
                    )
        if amp or self.max_grad_norm is not None:
            with_grad = [[p for p in g["params"] if p.grad is not None]
                         for g in self.param_groups]
            flat = [p for ps in with_grad for p in ps]
            # The resident path: every group that has gradients is
            # capturable, on one GPU. Everything else under max_grad_norm
            # is refused or served below as before.
            resident = (
                bool(flat)
                and all(g.get("capturable", False)
                        for g, ps in zip(self.param_groups, with_grad) if ps)
                and flat[0].device.type == "cuda"
                and all(p.device == flat[0].device for p in flat)
                and not (self.max_grad_norm is not None and any(
                    _is_dtensor(p) or _is_dtensor(p.grad) for p in flat))
            )
            if resident:
                self._resident_scaled_step(with_grad, loss_scale, found_inf)
                return
            if amp and flat:
                raise RuntimeError(
                    "grad_scale / found_inf (torch.amp.GradScaler) are set "
                    "on the optimizer, but unscaling and skipping inside "
                    "the step need every gradient on one GPU (and, next to "
                    "max_grad_norm, no DTensor)"
                )

        clip = None  # the coefficient as a 1-element tensor, per device
        if self.max_grad_norm is not None:
            if (any(g.get("capturable", False) for g in self.param_groups)
                    and torch.cuda.is_available()
                    and torch.cuda.is_current_stream_capturing()):
                raise RuntimeError(
                    "max_grad_norm cannot be captured in a graph next to a "
                    "param group that is not capturable=True, or with "
                    "gradients on more than one GPU: the gradient norm "
                    "kernel then builds its tensor table per call. Clip "
                    "outside the captured region, or capture without "
                    "max_grad_norm"
                )
            norm_coef = self._clip_norm_and_coef()
            self.grad_norm, self.grad_clip_coef = norm_coef[0], norm_coef[1]
            clip = {norm_coef.device: norm_coef[1:2]}

        def clip_on(device):
            if clip is None:
                return None
            if device not in clip:
                clip[device] = self.grad_clip_coef.reshape(1).to(device)
            return clip[device]

        ordinal = -1  # of a parameter over all groups, as state_dict counts
        for index, group in enumerate(self.param_groups):
            if group.get("capturable", False):
                self._capturable_group_step(
                    index, group, ordinal + 1, clip_on)
                ordinal += len(group["params"])
                continue
            beta1, beta2 = group["betas"]
            lr = group["lr"]
            weight_decay = group["weight_decay"]
            eps = group["eps"]
            use_kahan = group["use_kahan_summation"]
            momentum_dtype = group["momentum_dtype"]
            variance_dtype = group["variance_dtype"]
            compensation_dtype = group["compensation_buffer_dtype"]

            # Fused-eligible small tensors accumulate here and update in
            # ONE batched kernel launch at the end of the group — a
            # transformer group is hundreds of tensors, and per-tensor
            # launch overhead would otherwise dominate the small ones.
            batch = {k: [] for k in
                     ("p", "g", "m", "v", "c", "step_size", "bc2")}
            # A group with an fp8 state, or with stochastic rounding,
            # takes the block-scaled kernel for every parameter, whatever
            # its size and state dtypes, in one launch.
            sr = group.get("stochastic_rounding", False)
            if sr:
                _check_stochastic_rounding(group)
                batch["ordinal"], batch["step"] = [], []
            q8 = (sr or momentum_dtype in _Q8_DTYPES
                  or variance_dtype in _Q8_DTYPES)
            if q8:
                batch["ms"], batch["vs"] = [], []
                q8_kernel = _q8_kernel_loaded()

            for p in group["params"]:
                ordinal += 1
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError(
                        "AnyPrecisionAdamW does not support sparse gradients"
                    )

                if q8:
                    self._check_q8_can_run(p, q8_kernel, sr)
                if sr and p.dtype == torch.float16:
                    raise ValueError(
                        "stochastic_rounding=True stores bfloat16 "
                        "parameters (float32 ones as they are); a float16 "
                        "parameter is not supported"
                    )

                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0)
                    state["exp_avg"] = torch.zeros_like(p, dtype=momentum_dtype)
                    state["exp_avg_sq"] = torch.zeros_like(p, dtype=variance_dtype)
                    if use_kahan:
                        state["compensation"] = torch.zeros_like(
                            p, dtype=compensation_dtype
                        )
                    if q8:
                        if momentum_dtype in _Q8_DTYPES:
                            state["exp_avg_scale"] = _q8_scale(
                                state["exp_avg"])
                        if variance_dtype in _Q8_DTYPES:
                            state["exp_avg_sq_scale"] = _q8_scale(
                                state["exp_avg_sq"])

                state["step"] += 1
                step = state["step"].item()
                exp_avg = state["exp_avg"]
                exp_avg_sq = state["exp_avg_sq"]
                grad = p.grad

                bias_correction1 = 1 - beta1**step
                bias_correction2_sqrt = (1 - beta2**step) ** 0.5
                step_size = lr / bias_correction1

                # Fused-path eligibility on the local shards (DTensor
                # parameters under FSDP2 unwrap to their plain contiguous
                # shard; the elementwise step on the shard IS the sharded
                # step).
                p_l = _local_view(p)
                g_l = _local_view(grad)
                m_l = _local_view(exp_avg)
                v_l = _local_view(exp_avg_sq)
                c_l = _local_view(state["compensation"]) if use_kahan else None
                can_fuse = (
                    # (_check_q8_can_run has covered the first two.)
                    (q8 or (self.use_fused is not False
                            and _fused_step_available(p)))
                    and p_l.is_contiguous()
                    and g_l.is_contiguous()
                    and m_l.is_contiguous()
                    and v_l.is_contiguous()
                    and (c_l is None or c_l.is_contiguous())
                    and g_l.numel() == p_l.numel()
                    and m_l.numel() == p_l.numel()
                    and v_l.numel() == p_l.numel()
                )
                if q8:
                    if not can_fuse:
                        raise RuntimeError(
                            ("stochastic rounding needs" if sr else
                             "fp8 optimizer states need") + " the fused "
                            "AnyPrecisionAdamW step, which cannot run for "
                            "this parameter: its gradient or states are "
                            "non-contiguous or mismatched in size"
                        )
                    self._fused_steps += 1
                    batch["p"].append(p_l)
                    batch["g"].append(g_l)
                    batch["m"].append(m_l)
                    batch["ms"].append(state.get("exp_avg_scale"))
                    batch["v"].append(v_l)
                    batch["vs"].append(state.get("exp_avg_sq_scale"))
                    batch["c"].append(c_l)
                    batch["step_size"].append(step_size)
                    batch["bc2"].append(bias_correction2_sqrt)
                    if sr:
                        batch["ordinal"].append(ordinal)
                        batch["step"].append(int(step))
                    continue
                if self.use_fused is True and not can_fuse:
                    raise RuntimeError(
                        "use_fused=True, but the fused AnyPrecisionAdamW "
                        "step cannot run for this parameter (kernel "
                        "extension missing, non-GPU tensor, storage-less "
                        "wrapper subclass, or non-contiguous/mismatched "
                        "local shards). Pass use_fused=None to fall back "
                        "to the eager op sequence automatically."
                    )
                if can_fuse:
                    from torchdistx_amd import _kernels

                    self._fused_steps += 1
                    if p_l.numel() >= _BATCH_MAX_NUMEL:
                        # Big tensors take the per-tensor vectorized
                        # kernel (16-byte packed accesses).
                        _kernels.anyprecision_adamw_(
                            p_l,
                            g_l,
                            m_l,
                            v_l,
                            c_l,
                            lr,
                            beta1,
                            beta2,
                            eps,
                            weight_decay,
                            step_size,
                            bias_correction2_sqrt,
                            clip_on(p_l.device),
                        )
                    else:
                        batch["p"].append(p_l)
                        batch["g"].append(g_l)
                        batch["m"].append(m_l)
                        batch["v"].append(v_l)
                        batch["c"].append(c_l)
                        batch["step_size"].append(step_size)
                        batch["bc2"].append(bias_correction2_sqrt)
                    continue

                if clip is not None:
                    # A temporary: p.grad keeps its values.
                    grad = grad.mul(clip_on(grad.device)[0])

                # Decoupled weight decay (AdamW).
                if weight_decay:
                    p.mul_(1 - lr * weight_decay)

                # Moment updates — the exact op sequence torch 2.10's
                # _single_tensor_adam uses, so the all-fp32 configuration is
                # bitwise-equal to torch.optim.AdamW.
                exp_avg.lerp_(grad.to(exp_avg.dtype), 1 - beta1)
                exp_avg_sq.mul_(beta2).addcmul_(
                    grad.to(exp_avg_sq.dtype), grad.to(exp_avg_sq.dtype), value=1 - beta2
                )

                denom = (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)

                if use_kahan:
                    compensation = state["compensation"]
                    # Accumulate the update into the compensation buffer, then
                    # fold it into the weights, keeping the rounding error for
                    # the next step (Kahan/compensated summation).
                    compensation.addcdiv_(
                        exp_avg.to(compensation.dtype),
                        denom.to(compensation.dtype),
                        value=-step_size,
                    )
                    prev = p.detach().clone()
                    p.add_(compensation)
                    compensation.add_(prev.sub_(p))
                else:
                    p.addcdiv_(
                        exp_avg.to(p.dtype), denom.to(p.dtype), value=-step_size
                    )

            if batch["p"] and q8:
                from torchdistx_amd import _kernels

                _kernels.anyprecision_adamw_q8_(
                    batch["p"],
                    batch["g"],
                    batch["m"],
                    batch["ms"],
                    batch["v"],
                    batch["vs"],
                    batch["c"],
                    lr,
                    beta1,
                    beta2,
                    eps,
                    weight_decay,
                    batch["step_size"],
                    batch["bc2"],
                    clip_on(batch["p"][0].device),
                    *((group["stochastic_rounding_seed"], batch["ordinal"],
                       batch["step"]) if sr else ()),
                )
            elif batch["p"]:
                from torchdistx_amd import _kernels

                _kernels.anyprecision_adamw_batched_(
                    batch["p"],
                    batch["g"],
                    batch["m"],
                    batch["v"],
                    batch["c"],
                    lr,
                    beta1,
                    beta2,
                    eps,
                    weight_decay,
                    batch["step_size"],
                    batch["bc2"],
                    clip_on(batch["p"][0].device),
                )
