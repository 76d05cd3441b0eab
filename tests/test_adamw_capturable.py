# capturable=True of AnyPrecisionAdamW where no GPU is needed: the option
# itself and the refusals of the paths it cannot run on. The resident step
# is checked in tests/test_adamw_capturable_gpu.py.

import pytest
import torch

from torchdistx_amd.optimizers import AnyPrecisionAdamW


def _optimizer(**kw):
    p = torch.nn.Parameter(torch.ones(8))
    p.grad = torch.ones(8)
    return p, AnyPrecisionAdamW([p], capturable=True, **kw)


def test_option_is_a_group_default_and_travels_in_the_state_dict() -> None:
    p, opt = _optimizer()
    assert opt.param_groups[0]["capturable"] is True
    assert opt.state_dict()["param_groups"][0]["capturable"] is True
    plain = AnyPrecisionAdamW([p])
    assert plain.param_groups[0]["capturable"] is False
    plain.load_state_dict(opt.state_dict())
    assert plain.param_groups[0]["capturable"] is True


@pytest.mark.parametrize("kw, reason", [
    ({}, "the parameter is on cpu, not on a GPU"),
    ({"use_fused": False}, "use_fused=False forbids the fused step"),
    ({"lr": torch.tensor([1e-3, 1e-3])}, "takes lr as .* with 2 elements"),
    ({"lr": torch.tensor(1e-3, dtype=torch.float64)}, "not torch.float64"),
], ids=["cpu", "use_fused_false", "lr_size", "lr_dtype"])
def test_step_names_why_it_cannot_run(kw, reason) -> None:
    p, opt = _optimizer(**kw)
    with pytest.raises(RuntimeError, match="capturable=True .*" + reason):
        opt.step()
    assert len(opt.state[p]) == 0 and (p == 1).all()
