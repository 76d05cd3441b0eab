# SlowMomentumOptimizer(use_fused=...) where no GPU is needed: the refusal
# on CPU parameters, and use_fused=False being the default path bit for
# bit. The kernels themselves are covered in test_slowmo_fused_gpu.py.

import pytest
import torch

from tests.test_slowmo import single_proc_group  # noqa: F401
from torchdistx_amd.slowmo import SlowMomentumOptimizer


def _run(steps, **kwargs):
    torch.manual_seed(0)
    model = torch.nn.Linear(4, 3)
    opt = SlowMomentumOptimizer(
        torch.optim.SGD(model.parameters(), lr=0.1), slowmo_freq=2, **kwargs)
    for step in range(steps):
        for p in model.parameters():
            p.grad = torch.full_like(p, 0.01 * (step + 1))
        opt.step()
    return model, opt


def test_fused_refuses_cpu_parameters(single_proc_group):  # noqa: F811
    with pytest.raises(RuntimeError, match="a parameter is on cpu"):
        _run(1, use_fused=True)


def test_unfused_is_the_default_bitwise(single_proc_group):  # noqa: F811
    (ma, a), (mb, b) = _run(5), _run(5, use_fused=False)
    assert a.use_fused is False and a._fused_outer_steps == 0
    assert a.averager.step == b.averager.step == 5
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
        assert torch.equal(a.state[pa]["slow_momentum"],
                           b.state[pb]["slow_momentum"])
