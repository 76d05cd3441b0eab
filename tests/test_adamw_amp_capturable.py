# The GradScaler protocol of AnyPrecisionAdamW where no GPU is needed: who
# advertises _step_supports_amp_scaling, who refuses grad_scale / found_inf,
# and that an optimizer without capturable=True is what it was. The resident
# step is checked in tests/test_adamw_amp_capturable_gpu.py.

import pytest
import torch

from torchdistx_amd.optimizers import AnyPrecisionAdamW


def _param():
    p = torch.nn.Parameter(torch.linspace(-1, 1, 8))
    p.grad = torch.linspace(1, 2, 8)
    return p


def test_amp_support_is_every_group_capturable() -> None:
    opt = AnyPrecisionAdamW([_param()], capturable=True)
    assert opt._step_supports_amp_scaling is True
    opt.add_param_group({"params": [_param()], "capturable": False})
    assert opt._step_supports_amp_scaling is False
    mixed = AnyPrecisionAdamW([{"params": [_param()], "capturable": True},
                               {"params": [_param()]}])
    assert mixed._step_supports_amp_scaling is False
    mixed.add_param_group({"params": [_param()], "capturable": True})
    assert mixed._step_supports_amp_scaling is False
    assert AnyPrecisionAdamW([_param()])._step_supports_amp_scaling is False


@pytest.mark.parametrize("attr", ["grad_scale", "found_inf"])
def test_amp_attributes_next_to_a_plain_group_are_refused(attr) -> None:
    p = _param()
    opt = AnyPrecisionAdamW([{"params": [_param()], "capturable": True},
                             {"params": [p]}])
    setattr(opt, attr, torch.ones(()))
    with pytest.raises(RuntimeError, match="param group 1 is not capturable"):
        opt.step()
    assert len(opt.state[p]) == 0 and torch.equal(p, _param())


def test_plain_optimizer_steps_as_before() -> None:
    p, q = _param(), _param()
    opt = AnyPrecisionAdamW([p], weight_decay=0.01, max_grad_norm=0.5,
                            momentum_dtype=torch.float32,
                            variance_dtype=torch.float32)
    ref = torch.optim.AdamW([q], weight_decay=0.01)
    for _ in range(3):
        torch.nn.utils.clip_grad_norm_([q], 0.5)
        opt.step()
        ref.step()
        q.grad = p.grad.clone()
        assert torch.equal(p, q)
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    assert opt._norm_buffers == (None, None, None)
    assert opt.state[p]["step"].device.type == "cpu"
