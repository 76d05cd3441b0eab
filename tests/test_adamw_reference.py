# CPU proof of the AdamW checker in tests/_adamw_reference.py: a pure-torch
# fp32 emulation of the fused kernels' arithmetic (every operation rounded
# to fp32, the momentum alone through fp64 as in the kernels, rounding to the storage
# dtypes exactly where the kernels store) stays inside the bound for the
# whole dtype matrix, and seven deliberately wrong emulations each fall
# outside it. So the fp64 reference is one the kernels can meet, and the
# bound is tight enough to matter.

import dataclasses

import pytest
import torch

from tests._adamw_reference import (
    ALL_F32,
    BF16,
    DTYPE_MATRIX,
    F32,
    FLAGSHIP,
    K_ROUNDINGS,
    Case,
    Scalars,
    check_step,
    layout_id,
    narrow,
)

N = 4096
WEIGHT_DECAYS = (0.0, 0.01)
# (first step?, step number): the real first step from m = v = 0, and the
# step-1000 scalars on non-zero state.
STEPS = ((True, 1), (False, 1000))


def _t(x):
    return torch.tensor(x, dtype=F32)


def _lerp_momentum(m, g, w):
    """lerpMomentum of the kernels: m + w * (g - m) formed in fp64 and
    rounded to fp32 once."""
    return (m.double() + w * (g.double() - m.double())).float()


def emulate(p, g, m, v, c, scalars, mutant=None):
    """One fused step in fp32 as the kernels order it. Returns (p', m', v',
    c') in the storage dtypes of p, m, v, c. `mutant` names one deliberate
    defect."""
    s = scalars.narrowed()
    pf, gf, mf, vf = p.float(), g.float(), m.float(), v.float()
    omb2 = _t(s.one_minus_beta2)
    if mutant == "fp32_one_minus_beta2":
        omb2 = _t(1.0) - _t(s.beta2)
    undecayed = pf
    if s.weight_decay != 0.0:
        pf = pf * _t(s.decay)
    if mutant == "uncompensated_momentum":
        mf = mf + _t(s.one_minus_beta1) * (gf - mf)
    else:
        mf = _lerp_momentum(mf, gf, s.one_minus_beta1)
    vf = vf * _t(s.beta2) + gf * gf * omb2
    v_root = vf
    if mutant == "variance_rounded_before_sqrt":
        v_root = vf.to(v.dtype).float()
    denom = v_root.sqrt() / _t(s.bias_correction2_sqrt) + _t(s.eps)
    update = -_t(s.step_size) * (mf / denom)
    if c is None:
        c_out = None
        p_out = (pf + update).to(p.dtype)
    else:
        cf = c.float() + update
        if mutant == "compensation_rounded_before_add":
            cf = cf.to(c.dtype).float()
        prev = undecayed if mutant == "prev_before_decay" else pf
        p_new = pf + cf
        p_out = p_new.to(p.dtype)
        stored = p_new if mutant == "remainder_from_unrounded" else (
            p_out.float())
        c_out = (cf + (prev - stored)).to(c.dtype)
    return p_out, mf.to(m.dtype), vf.to(v.dtype), c_out


def _run(layout, first_step, step, wd, mutant=None, seed=11):
    case = Case(N, layout, first_step, "cpu", seed)
    scalars = Scalars.for_step(step, weight_decay=wd)
    after = emulate(*case.operands(), scalars, mutant=mutant)
    return check_step(case.before(), after, scalars,
                      where=f"{layout_id(layout)} step {step} wd {wd}")


@pytest.mark.parametrize("wd", WEIGHT_DECAYS)
@pytest.mark.parametrize("first_step,step", STEPS)
def test_emulation_meets_bound_for_dtype_matrix(first_step, step, wd) -> None:
    worst = 0.0
    for layout in DTYPE_MATRIX:
        needed = _run(layout, first_step, step, wd)
        worst = max(worst, max(needed.values()))
    print(f"largest K needed by the emulation: {worst:.2f}")
    assert worst <= K_ROUNDINGS


def test_narrowed_complements_are_formed_in_double() -> None:
    s = Scalars.for_step(1, weight_decay=0.01).narrowed()
    assert s.one_minus_beta2 == narrow(1.0 - 0.999)
    fp32_formed = (_t(1.0) - _t(0.999)).item()
    # 111 fp32 ulps: the spacing of fp32 at 1e-3 is 2^-33.
    assert round(abs(fp32_formed - s.one_minus_beta2) / 2.0**-33) == 111


def _assert_mutant_fails(layout, first_step, step, wd, mutant, output):
    # The unmutated emulation passes the very same case ...
    _run(layout, first_step, step, wd)
    # ... and the mutant is caught, at the output it corrupts.
    with pytest.raises(AssertionError, match=output):
        _run(layout, first_step, step, wd, mutant=mutant)


def test_mutant_fp32_one_minus_beta2_fails() -> None:
    # fp32 variance on the first step: v' = g^2 * (1 - beta2) carries the
    # full 1.29e-5 relative error of 1.0f - beta2.
    _assert_mutant_fails(ALL_F32, True, 1, 0.01, "fp32_one_minus_beta2",
                         "exp_avg_sq")
    # A bf16 variance hides the defect by design: the 2^-9 storage
    # rounding swamps it, so the stored variance of the flagship layout
    # stays inside its bound. (The update still moves by 6.5e-6 relative
    # through the denominator, which the Kahan outputs may show.)
    try:
        _run(FLAGSHIP, True, 1, 0.01, mutant="fp32_one_minus_beta2")
    except AssertionError as e:
        assert "exp_avg_sq" not in str(e)


def test_mutant_kahan_remainder_from_unrounded_sum_fails() -> None:
    _assert_mutant_fails(FLAGSHIP, False, 1000, 0.01,
                         "remainder_from_unrounded", "compensation")


def test_mutant_prev_before_weight_decay_fails() -> None:
    _assert_mutant_fails(FLAGSHIP, False, 1000, 0.01, "prev_before_decay",
                         "compensation")


def test_mutant_compensation_rounded_before_add_fails() -> None:
    _assert_mutant_fails(FLAGSHIP, False, 1000, 0.01,
                         "compensation_rounded_before_add", "compensation")


def test_mutant_variance_rounded_before_sqrt_fails() -> None:
    # bf16 variance, fp32 everything else: the 2^-9 error of the rounded
    # variance reaches the fp32 parameter through the update.
    layout = (F32, F32, F32, BF16, None)
    _assert_mutant_fails(layout, False, 1000, 0.0,
                         "variance_rounded_before_sqrt", "param")
    # With Kahan it shows in the compensation of a bf16 parameter.
    _assert_mutant_fails(FLAGSHIP, False, 1000, 0.0,
                         "variance_rounded_before_sqrt", "compensation")


def test_mutant_neighbour_step_size_fails() -> None:
    # A batch of tensors on steps 1..4: tensor t updated with tensor
    # t+1's step_size, as an off-by-one in the batched blob would.
    cases = [Case(N, FLAGSHIP, False, "cpu", 20 + t) for t in range(4)]
    scalars = [Scalars.for_step(t + 1, weight_decay=0.01) for t in range(4)]
    for case, s in zip(cases, scalars):
        check_step(case.before(), emulate(*case.operands(), s), s)
    for t in range(3):
        wrong = dataclasses.replace(scalars[t],
                                    step_size=scalars[t + 1].step_size)
        after = emulate(*cases[t].operands(), wrong)
        with pytest.raises(AssertionError, match="param|compensation"):
            check_step(cases[t].before(), after, scalars[t])


def test_mutant_uncompensated_momentum_fails_where_it_cancels() -> None:
    # With g ~ -9 m the new momentum m + (1 - beta1)(g - m) cancels. Formed
    # plainly in fp32 its rounding error, a few 2^-24 (|m| + |g|), is
    # inside the exp_avg bound, but the update is step_size * exp_avg' /
    # denom and inherits it, and the parameter's mag (|p_decayed| + |c| +
    # |update|) holds neither |m| nor |g|: next to a parameter far smaller
    # than the update scale that needs K well above 32 (K up to 557 seen
    # in 3.4e7 elements of the test distribution, where it takes g / m
    # within about 1e-2 of -9 together with |p| < 4e-5: a few elements in
    # 10^7, none in the 4096-element matrix above). lerpMomentum of the
    # kernels rounds the momentum once instead, and stays inside.
    gen = torch.Generator().manual_seed(5)
    n = 4096
    m = 1e-2 * torch.randn(n, generator=gen)
    g = -9.0 * m * (1 + 1e-3 * torch.randn(n, generator=gen))
    v = m * m
    p = 1e-6 * torch.randn(n, generator=gen)
    c = torch.zeros(n)
    s = Scalars.for_step(1000, weight_decay=0.01)
    for layout, output in (
        ((p.bfloat16(), g, m, v, c.bfloat16()), "compensation"),
        # Twice as many parameter bits do not help: the error is in the
        # update.
        ((p, g, m, v, None), "param"),
    ):
        needed = check_step(layout, emulate(*layout, s), s)
        assert max(needed.values()) <= 8
        after = emulate(*layout, s, mutant="uncompensated_momentum")
        with pytest.raises(AssertionError, match=output) as info:
            check_step(layout, after, s)
        assert "exp_avg" not in str(info.value).replace("exp_avg_sq", "")


def test_checker_flags_mask_mismatch_and_written_guard() -> None:
    case = Case(64, ALL_F32, False, "cpu", 3)
    s = Scalars.for_step(1000)
    p, m, v, _ = emulate(*case.operands(), s)
    bad = p.clone()
    bad[5] = float("nan")
    with pytest.raises(AssertionError, match="nan mask"):
        check_step(case.before(), (bad, m, v, None), s)
    bad = v.clone()
    bad[9] = float("inf")
    with pytest.raises(AssertionError, match="inf mask"):
        check_step(case.before(), (p, m, bad, None), s)
    case.assert_guards_and_grad_intact()
    case.buffers["m"][case.offsets["m"] + 64] = 0.0
    with pytest.raises(AssertionError, match="guard after m"):
        case.assert_guards_and_grad_intact()
    case = Case(64, ALL_F32, False, "cpu", 3)
    case.views["g"][0] = 1.0
    with pytest.raises(AssertionError, match="grad was written"):
        case.assert_guards_and_grad_intact()
