# Slow Momentum optimizer wrapper (arXiv:1910.00643).
#
# Capability parity with the reference
# (/root/reference/src/python/torchdistx/slowmo/slowmo_optimizer.py:11-235):
# wraps an arbitrary torch.optim.Optimizer; every step runs the base
# optimizer and a PeriodicModelAverager (global exact parameter averaging
# every ``slowmo_freq`` steps); after each averaging round applies the slow
# ("outer") momentum update
#     m   <- slowmo_factor * m + (prev - param) / lr
#     prev <- prev - slowmo_lr * lr * m
#     param <- prev
# State-dict layout matches the reference: the base optimizer dict plus
# "slowmo_freq" / "slowmo_factor" / "slowmo_lr" / "step" entries
# (reference slowmo_optimizer.py:156-189). ``_prev_parameters`` is
# deliberately NOT checkpointed (reconstructed at construction), matching
# reference slowmo_optimizer.py:132-144.
#
# Differences from the reference (intentional fixes):
#   * the slow-momentum buffer is allocated on the parameter's device rather
#     than unconditionally on the current CUDA device, so the optimizer also
#     works on CPU (gloo) test rigs and mixed-device param groups.

import functools

import torch
import torch.distributed as dist
import torch.distributed.algorithms.model_averaging.averagers as averagers


def _check_groups_have_lr(optim: torch.optim.Optimizer) -> None:
    """The slow-momentum update divides by each group's lr, so every group
    must carry one (and the optimizer must have groups at all)."""
    if not optim.param_groups:
        raise ValueError("the base optimizer has no parameter groups")
    if any("lr" not in g for g in optim.param_groups):
        raise ValueError(
            "every parameter group needs an explicit learning rate: the "
            "slow-momentum outer update rescales by 1/lr per group"
        )


_FUSED_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _fused_refusal(params, prevs, momenta):
    """Why the SlowMo kernels (csrc/hip/slowmo.hip) cannot take these
    parameters, previous parameters and (already created) momenta, or None
    if they can."""
    try:
        from torchdistx_amd import _kernels

        loaded = _kernels.has_slowmo()
    except Exception:
        loaded = False
    for p in params:
        if torch.utils._python_dispatch.is_traceable_wrapper_subclass(p):
            return ("a parameter is a DTensor or another wrapper subclass, "
                    "not a plain dense tensor")
        if p.device.type != "cuda":
            return f"a parameter is on {p.device.type}, not on a GPU"
        if p.device != params[0].device:
            return "the parameters are on more than one device"
        if p.dtype not in _FUSED_DTYPES:
            return f"a parameter is {p.dtype}, not float32/bfloat16/float16"
    if not loaded:
        return ("the kernel extension torchdistx_amd._K (with "
                "slowmo_outer_step_) is not loaded")
    for what, tensors in (("parameter", params),
                          ("previous parameter", prevs),
                          ("slow momentum", momenta)):
        for t in tensors:
            if t.layout != torch.strided or not t.is_contiguous():
                return f"a {what} is non-contiguous"
    for p, prev in zip(params, prevs):
        if prev.dtype != p.dtype or prev.device != p.device:
            return ("a previous parameter differs from its parameter in "
                    "dtype or device")
    for m in momenta:
        if m.dtype != torch.float32:
            return f"a slow momentum is {m.dtype}, not float32"
    if not (dist.is_available() and dist.is_initialized()):
        return "torch.distributed is not initialised"
    return None


class SlowMomentumOptimizer(torch.optim.Optimizer):
    """Wraps a base optimizer and runs distributed training with Slow
    Momentum. Designed for FSDP modules with a ``NO_SHARD`` strategy together
    with :func:`torchdistx_amd.slowmo.slowmo_hook`.

    Args:
        base_optim: the base optimizer updating the local model replica.
        slowmo_freq: run parameter averaging + slow momentum every this many
            steps (default: 48).
        slowmo_factor: slow momentum coefficient (default: 0.5).
        slowmo_lr: slow momentum learning-rate scale (default: 1.0).
        use_fused: run the averaging rounds through the multi-tensor HIP
            kernels of ``csrc/hip/slowmo.hip`` (one pack launch, one
            all-reduce of a flat buffer, one outer-step launch, the
            arithmetic once in fp32; see ``docs/slowmo.md``). ``step`` then
            raises ``RuntimeError`` where the kernels cannot take the
            parameters; it never falls back to the eager update.
            ``_fused_outer_steps`` counts the outer updates the kernel
            applied. Default ``False``: the eager update.
    """

    def __init__(
        self,
        base_optim: torch.optim.Optimizer,
        slowmo_freq: int = 48,
        slowmo_factor: float = 0.5,
        slowmo_lr: float = 1.0,
        use_fused: bool = False,
    ):
        if base_optim is None:
            raise ValueError("a base optimizer is required (got None)")
        self._base_optim = base_optim
        _check_groups_have_lr(base_optim)
        self.param_groups = self._base_optim.param_groups

        if slowmo_freq < 1:
            raise ValueError(f"slowmo_freq must be >= 1, got {slowmo_freq}")
        self.slowmo_freq = slowmo_freq
        if slowmo_factor < 0.0:
            raise ValueError(
                f"slowmo_factor must be >= 0, got {slowmo_factor}"
            )
        self.slowmo_factor = slowmo_factor
        if slowmo_lr < 0.0:
            raise ValueError(f"slowmo_lr must be >= 0, got {slowmo_lr}")
        self.slowmo_lr = slowmo_lr
        self.use_fused = bool(use_fused)
        self._fused_outer_steps = 0
        # The buffer the fused rounds all-reduce, and the layout it was
        # allocated for.
        self._flat = None
        self._flat_key = None

        self.averager = averagers.PeriodicModelAverager(
            period=slowmo_freq, warmup_steps=0
        )

        # Snapshot of the parameters at the last slow-momentum update, in
        # flattened param_groups order. Kept outside ``self.state`` because
        # many base optimizers use an empty per-param state as the "first
        # step" signal.
        self._prev_parameters = [
            param.detach().clone()
            for group in self.param_groups
            for param in group["params"]
        ]

    @property
    def state(self):
        """Forwards to the base optimizer's ``state``."""
        return self._base_optim.state

    def __repr__(self):
        return self._base_optim.__repr__()

    def state_dict(self):
        """Base optimizer ``state_dict`` plus the SlowMo hyper-parameters and
        the averager step counter."""
        sd = self._base_optim.state_dict()
        sd["slowmo_freq"] = self.slowmo_freq
        sd["slowmo_factor"] = self.slowmo_factor
        sd["slowmo_lr"] = self.slowmo_lr
        sd["step"] = self.averager.step
        return sd

    def load_state_dict(self, state_dict):
        """Restores the base optimizer state and the SlowMo entries written
        by :meth:`state_dict`."""
        state_dict = dict(state_dict)
        self.slowmo_freq = state_dict.pop("slowmo_freq")
        self.averager.period = self.slowmo_freq
        self.slowmo_factor = state_dict.pop("slowmo_factor")
        self.slowmo_lr = state_dict.pop("slowmo_lr")
        self.averager.step = state_dict.pop("step")
        self._base_optim.load_state_dict(state_dict)
        _check_groups_have_lr(self._base_optim)

    def _flat_params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _slow_momenta(self, params):
        """The fp32 momentum of every parameter, created on first use."""
        momenta = []
        for param in params:
            pstate = self.state[param]
            if "slow_momentum" not in pstate:
                pstate["slow_momentum"] = torch.zeros(
                    param.shape, device=param.device
                )
            momenta.append(pstate["slow_momentum"])
        return momenta

    def _fused_step(self):
        """``step`` under ``use_fused=True``: the averaging rounds run as
        pack kernel, all-reduce of one flat buffer, outer-step kernel
        (csrc/hip/slowmo.hip)."""
        averager = self.averager
        # The period rule of PeriodicModelAverager.average_parameters.
        averaging = (
            averager.step >= averager.warmup_steps
            and (averager.step - averager.warmup_steps) % averager.period == 0
        )
        if not averaging:
            self._base_optim.step()
            averager.step += 1
            return

        params = self._flat_params()
        prevs = self._prev_parameters
        refusal = _fused_refusal(
            params, prevs,
            [self.state[p]["slow_momentum"] for p in params
             if "slow_momentum" in self.state.get(p, ())])
        if refusal is not None:
            raise RuntimeError(
                f"SlowMomentumOptimizer(use_fused=True) cannot run: "
                f"{refusal}. Pass use_fused=False for the eager update."
            )
        self._base_optim.step()
        if averager.step == 0:
            # The very first call averages without an outer update: nothing
            # to fuse, the stock averager does it.
            averager.average_parameters(params=self.param_groups)
            return

        from torchdistx_amd import _kernels

        lrs = [
            float(g["lr"]) for g in self.param_groups for _ in g["params"]
        ]
        rows = list(zip(params, prevs, self._slow_momenta(params), lrs))
        # The stock averager averages the parameters that have a gradient;
        # the outer update applies to all of them.
        averaged = [r for r in rows if r[0].grad is not None]
        local = [r for r in rows if r[0].grad is None]
        if averaged:
            ps = [r[0] for r in averaged]
            offsets, total = _kernels.slowmo_flat_layout(ps)
            dtype = functools.reduce(torch.promote_types,
                                     (p.dtype for p in ps))
            key = (tuple(offsets), total, dtype, ps[0].device)
            if self._flat_key != key:
                # Zero-filled once: the kernels never write the padding
                # between slots, and zeros stay zero under all-reduce.
                self._flat = torch.zeros(total, dtype=dtype,
                                         device=ps[0].device)
                self._flat_key = key
            group = averager.process_group
            _kernels.slowmo_pack_(ps, self._flat, dist.get_world_size(group))
            dist.all_reduce(self._flat, group=group)
        for part, flat in ((averaged, self._flat), (local, None)):
            if part:
                ps, pv, ms, ls = map(list, zip(*part))
                _kernels.slowmo_outer_step_(ps, pv, ms, flat, ls,
                                            self.slowmo_factor,
                                            self.slowmo_lr)
        averager.step += 1
        self._fused_outer_steps += 1

    @torch.no_grad()
    def step(self):
        """One local step; every ``slowmo_freq`` steps a global parameter
        average followed by the slow momentum update."""
        if self.use_fused:
            return self._fused_step()
        self._base_optim.step()
        # The averager all-reduce-averages the parameters every
        # ``slowmo_freq`` calls and increments its step counter every call.
        self.averager.average_parameters(params=self.param_groups)
        just_averaged = (
            self.averager.step != 1
            and (self.averager.step - 1) % self.slowmo_freq == 0
        )
        if not just_averaged:
            return

        idx = 0
        for group in self.param_groups:
            inv_lr = 1.0 / group["lr"]
            for param in group["params"]:
                pstate = self.state[param]
                if "slow_momentum" not in pstate:
                    pstate["slow_momentum"] = torch.zeros(
                        param.shape, device=param.device
                    )
                momentum = pstate["slow_momentum"]
                prev = self._prev_parameters[idx]
                # m <- factor*m + (prev - param)/lr
                momentum.mul_(self.slowmo_factor).sub_(param, alpha=inv_lr).add_(
                    prev, alpha=inv_lr
                )
                # prev <- prev - slowmo_lr*lr*m ; param <- prev
                prev.add_(momentum, alpha=-self.slowmo_lr * group["lr"])
                param.copy_(prev)
                idx += 1

    def zero_grad(self, set_to_none: bool = False):  # type: ignore[override]
        self._base_optim.zero_grad(set_to_none=set_to_none)

    def add_param_group(self, param_group):
        self._base_optim.add_param_group(param_group)
        for param in param_group["params"]:
            self._prev_parameters.append(param.detach().clone())
