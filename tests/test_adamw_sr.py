# CPU tests of the stochastic-rounding reference (tests/_adamw_sr_reference.py)
# and of the stochastic_rounding interface of AnyPrecisionAdamW.

import numpy as np
import pytest
import torch

from tests._adamw_sr_reference import philox10, sr_code
from torchdistx_amd.optimizers import AnyPrecisionAdamW

ONES = 0xFFFFFFFFFFFFFFFF


# Random123's published known answers for Philox4x32-10; counter words
# (c0, c1, c2, c3) = (offset lo, offset hi, subsequence lo, subsequence hi).
@pytest.mark.parametrize("offset, subsequence, seed, want", [
    (0, 0, 0, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    (ONES, ONES, ONES, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    (0x85A308D3243F6A88, 0x0370734413198A2E, 0x299F31D0A4093822,
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(offset, subsequence, seed, want) -> None:
    words = philox10(seed, subsequence, [offset])
    assert " ".join(f"{int(w[0]):08x}" for w in words) == want


def _f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("bits, rand, want", [
    (0x3F800000, 0xFFFF, 0x3F80),  # representable: never moves
    (0xBF810000, 0xFFFF, 0xBF81),
    (0x3F808000, 0x7FFF, 0x3F80),  # low half 0x8000: the carry needs 0x8000
    (0x3F808000, 0x8000, 0x3F81),
    (0xBF808000, 0x7FFF, 0xBF80),  # negative: away from zero on a carry
    (0xBF808000, 0x8000, 0xBF81),
    (0xBF7FFFFF, 0x0001, 0xBF80),  # the carry runs into the exponent
    (0x80000000, 0xFFFF, 0x8000),  # -0.0
    (0x00000001, 0xFFFF, 0x0001),  # fp32 subnormal to the smallest bf16
    (0x00000001, 0xFFFE, 0x0000),
    (0x7F7FFFFF, 0xFFFF, 0x7F7F),  # never an infinity from a finite value
    (0xFF7FFFFF, 0x0001, 0xFF7F),
    (0x7F800000, 0xFFFF, 0x7F80),  # inf
    (0xFF800000, 0x1234, 0xFF80),
    (0x7F800001, 0xFFFF, 0x7FC0),  # NaN stays NaN
])
def test_recipe_on_bit_patterns(bits, rand, want) -> None:
    assert int(sr_code(_f32(bits), [rand])[0]) == want


def _param(dtype=torch.bfloat16, n=8):
    p = torch.nn.Parameter(torch.ones(n, dtype=dtype))
    p.grad = torch.ones_like(p)
    return p


def test_refusals() -> None:
    with pytest.raises(ValueError, match="use_kahan_summation"):
        AnyPrecisionAdamW([_param()], stochastic_rounding=True,
                          use_kahan_summation=True)
    with pytest.raises(ValueError, match="use_kahan_summation"):
        AnyPrecisionAdamW([{"params": [_param()],
                            "use_kahan_summation": True}],
                          stochastic_rounding=True)
    with pytest.raises(ValueError, match="seed"):
        AnyPrecisionAdamW([_param()], stochastic_rounding=True,
                          stochastic_rounding_seed=-1)
    with pytest.raises(RuntimeError, match="stochastic rounding.*cpu"):
        AnyPrecisionAdamW([_param()], stochastic_rounding=True).step()
    with pytest.raises(RuntimeError, match="use_fused=False"):
        AnyPrecisionAdamW([_param()], stochastic_rounding=True,
                          use_fused=False).step()


def test_seed_default_and_state_dict() -> None:
    torch.manual_seed(7)
    a = AnyPrecisionAdamW([_param()], stochastic_rounding=True)
    torch.manual_seed(7)
    b = AnyPrecisionAdamW([_param()], stochastic_rounding=True)
    seed = a.param_groups[0]["stochastic_rounding_seed"]
    assert isinstance(seed, int) and 0 <= seed < 2**63
    assert seed == b.param_groups[0]["stochastic_rounding_seed"]
    group = a.state_dict()["param_groups"][0]
    assert group["stochastic_rounding"] is True
    assert group["stochastic_rounding_seed"] == seed
    given = AnyPrecisionAdamW([_param()], stochastic_rounding=True,
                              stochastic_rounding_seed=11)
    assert given.param_groups[0]["stochastic_rounding_seed"] == 11


def test_default_off_adds_two_keys_and_draws_nothing() -> None:
    torch.manual_seed(7)
    before = torch.get_rng_state()
    opt = AnyPrecisionAdamW([_param(torch.float32)])
    assert torch.equal(torch.get_rng_state(), before)
    group = opt.param_groups[0]
    assert group["stochastic_rounding"] is False
    assert group["stochastic_rounding_seed"] is None
    plain = torch.optim.AdamW([_param(torch.float32)]).param_groups[0]
    ours = {"use_kahan_summation", "momentum_dtype", "variance_dtype",
            "compensation_buffer_dtype", "stochastic_rounding",
            "stochastic_rounding_seed"}
    assert set(group) - set(plain) == ours
    opt.step()  # the eager CPU step, as ever
    assert set(opt.state[group["params"][0]]) == {"step", "exp_avg",
                                                  "exp_avg_sq"}
