# Typing stub for the CDNA4 kernel extension.

from typing import List, Optional, Tuple, Union

import torch

def has_init_kernels() -> bool: ...
def has_anyprecision_adamw() -> bool: ...
def has_anyprecision_adamw_batched() -> bool: ...
def has_anyprecision_adamw_q8() -> bool: ...
def has_grad_norm() -> bool: ...
def has_batched_init() -> bool: ...
def has_fused_chains() -> bool: ...
def has_box_kernel() -> bool: ...
def has_cast_chains() -> bool: ...
def has_patch_kernel() -> bool: ...
def anyprecision_adamw_(
    param: torch.Tensor,
    grad: torch.Tensor,
    exp_avg: torch.Tensor,
    exp_avg_sq: torch.Tensor,
    compensation: Optional[torch.Tensor],
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step_size: float,
    bias_correction2_sqrt: float,
    grad_scale: Optional[torch.Tensor] = None,
) -> None: ...
def anyprecision_adamw_batched_(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    exp_avgs: List[torch.Tensor],
    exp_avg_sqs: List[torch.Tensor],
    compensations: List[Optional[torch.Tensor]],
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step_sizes: List[float],
    bias_correction2_sqrts: List[float],
    grad_scale: Optional[torch.Tensor] = None,
) -> None: ...
def anyprecision_adamw_q8_(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    exp_avgs: List[torch.Tensor],
    exp_avg_scales: List[Optional[torch.Tensor]],
    exp_avg_sqs: List[torch.Tensor],
    exp_avg_sq_scales: List[Optional[torch.Tensor]],
    compensations: List[Optional[torch.Tensor]],
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
    step_sizes: List[float],
    bias_correction2_sqrts: List[float],
    grad_scale: Optional[torch.Tensor] = None,
    sr_seed: Optional[int] = None,
    ordinals: Optional[List[int]] = None,
    steps: Optional[List[int]] = None,
) -> None: ...
def has_anyprecision_adamw_resident() -> bool: ...

class AdamWResidentPlan:
    def __init__(
        self,
        params: List[torch.Tensor],
        grads: List[torch.Tensor],
        exp_avgs: List[torch.Tensor],
        exp_avg_scales: List[Optional[torch.Tensor]],
        exp_avg_sqs: List[torch.Tensor],
        exp_avg_sq_scales: List[Optional[torch.Tensor]],
        compensations: List[Optional[torch.Tensor]],
        steps: List[torch.Tensor],
        ordinals: List[int],
    ) -> None: ...
    def matches(self, grads: List[torch.Tensor]) -> bool: ...
    def stale(self) -> bool: ...
    def rebind(self, grads: List[torch.Tensor]) -> None: ...
    def step(
        self,
        lr: Union[float, torch.Tensor],
        beta1: float,
        beta2: float,
        eps: float,
        weight_decay: float,
        grad_scale: Optional[torch.Tensor] = None,
        sr_seed: Optional[int] = None,
        found_inf: Optional[torch.Tensor] = None,
    ) -> None: ...
    def grad_grid(self) -> int: ...
    def grad_sumsq(self, partials: torch.Tensor, offset: int) -> None: ...
    def scalars(
        self,
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]: ...
    def __len__(self) -> int: ...

def grad_norm_clip_coef_(
    grads: List[torch.Tensor],
    max_norm: float,
    out: torch.Tensor,
) -> None: ...
def grad_norm_finalize_resident_(
    partials: Optional[torch.Tensor],
    n_partials: int,
    max_norm: Optional[float],
    loss_scale: Optional[torch.Tensor],
    found_inf: Optional[torch.Tensor],
    out: torch.Tensor,
) -> None: ...
def grad_norm_grid_cap() -> int: ...
def has_slowmo() -> bool: ...
def slowmo_flat_layout(
    params: List[torch.Tensor],
) -> Tuple[List[int], int]: ...
def slowmo_pack_(
    params: List[torch.Tensor],
    flat: torch.Tensor,
    world_size: int,
) -> None: ...
def slowmo_outer_step_(
    params: List[torch.Tensor],
    prevs: List[torch.Tensor],
    momenta: List[torch.Tensor],
    flat: Optional[torch.Tensor],
    lrs: List[float],
    slowmo_factor: float,
    slowmo_lr: float,
) -> None: ...
def batched_init_(
    tensors: List[torch.Tensor],
    dists: List[int],
    p0s: List[float],
    p1s: List[float],
    seeds: List[int],
    offsets: List[int],
    tail_ops: List[List[int]] = ...,
    tail_s0: List[List[float]] = ...,
    tail_s1: List[List[float]] = ...,
    src_dtypes: Optional[List[Optional[torch.dtype]]] = None,
) -> None: ...
