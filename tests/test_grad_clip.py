# AnyPrecisionAdamW(max_grad_norm=...) on the CPU: the eager path must be
# clip_grad_norm_ followed by the unclipped step, bit for bit, except that
# p.grad keeps its values.

import pytest
import torch
from torch.nn.utils import clip_grad_norm_, get_total_norm

from torchdistx_amd.optimizers import AnyPrecisionAdamW

SIZES = [1, 7, 2049]


def _bits(t):
    return t.contiguous().view(torch.uint8)


# Gradient norm ~ sqrt(2057) ~ 45: 0.5 clips, 1e30 does not.
@pytest.mark.parametrize("max_norm", [0.5, 1e30], ids=["active", "inactive"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["f32", "bf16"])
def test_eager_step_equals_clip_grad_norm_then_step(dtype, max_norm) -> None:
    gen = torch.Generator().manual_seed(11)
    a = [torch.nn.Parameter(torch.randn(n, generator=gen).to(dtype))
         for n in SIZES]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    kw = dict(lr=1e-2, weight_decay=0.01, use_kahan_summation=True,
              use_fused=False)
    opt_a = AnyPrecisionAdamW(a, **kw)
    opt_b = AnyPrecisionAdamW(b, max_grad_norm=max_norm, **kw)
    assert opt_b.grad_norm is None and opt_b.grad_clip_coef is None
    for _ in range(3):
        grads = [torch.randn(n, generator=gen).to(dtype) for n in SIZES]
        for p, q, g in zip(a, b, grads):
            p.grad, q.grad = g.clone(), g.clone()
        want_norm = get_total_norm(grads, 2.0)
        clip_grad_norm_(a, max_norm)
        opt_a.step()
        opt_b.step()
        assert opt_b.grad_norm.dtype == torch.float32
        assert opt_b.grad_norm.dim() == opt_b.grad_clip_coef.dim() == 0
        assert opt_b.grad_norm == want_norm
        assert (opt_b.grad_clip_coef < 1) == (max_norm < 1)
        for p, q, g in zip(a, b, grads):
            assert torch.equal(_bits(q.grad), _bits(g))
            assert torch.equal(p, q)
            assert set(opt_a.state[p]) == set(opt_b.state[q])
            for k, v in opt_a.state[p].items():
                assert torch.equal(v, opt_b.state[q][k]), k


@pytest.mark.parametrize("bad", [0, -1.0, float("nan"), "x"])
def test_max_grad_norm_must_be_a_positive_number(bad) -> None:
    with pytest.raises(ValueError, match="max_grad_norm"):
        AnyPrecisionAdamW([torch.nn.Parameter(torch.zeros(3))],
                          max_grad_norm=bad)


def test_without_max_grad_norm_nothing_is_recorded() -> None:
    p = torch.nn.Parameter(torch.ones(5))
    p.grad = torch.ones(5)
    opt = AnyPrecisionAdamW([p], use_fused=False)
    opt.step()
    assert opt.max_grad_norm is None
    assert opt.grad_norm is None and opt.grad_clip_coef is None
