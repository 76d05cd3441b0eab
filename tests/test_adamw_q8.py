# CPU tests of AnyPrecisionAdamW's fp8 state rules: what the constructor
# refuses, and that step names why fp8 states cannot run off the fused path.

import pytest
import torch

from torchdistx_amd.optimizers import AnyPrecisionAdamW

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


def _param():
    p = torch.nn.Parameter(torch.ones(300))
    p.grad = torch.ones(300)
    return p


@pytest.mark.parametrize("kwargs", [
    {"compensation_buffer_dtype": E4M3},
    {"compensation_buffer_dtype": E5M2},
    {"momentum_dtype": torch.float8_e4m3fnuz},
    {"variance_dtype": torch.float8_e5m2fnuz},
], ids=str)
def test_constructor_rejects(kwargs) -> None:
    with pytest.raises(ValueError, match="not supported"):
        AnyPrecisionAdamW([_param()], **kwargs)


@pytest.mark.parametrize("use_fused,reason", [
    (None, "on cpu"), (True, "on cpu"), (False, "use_fused=False"),
])
def test_step_names_why_fp8_states_cannot_run(use_fused, reason) -> None:
    p = _param()
    opt = AnyPrecisionAdamW([p], momentum_dtype=E4M3, variance_dtype=E5M2,
                            use_fused=use_fused)
    with pytest.raises(RuntimeError, match=reason):
        opt.step()
    assert not opt.state[p] and torch.equal(p.detach(), torch.ones(300))
