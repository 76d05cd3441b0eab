# GPU (MI355X) tests of the stochastic rounding of bf16 parameters in the
# fused AnyPrecisionAdamW step: every stored bit against the fp64 reference
# and the numpy Philox of tests/_adamw_sr_reference.py, the unbiased mean
# where round-to-nearest stalls, and determinism through a checkpoint.

import copy

import pytest
import torch

from tests._adamw_reference import (
    BF16, F32, K_ROUNDINGS, Scalars, reference_step)
from tests._adamw_q8_reference import E4M3, E5M2, check_q8_step, dequantize
from tests._adamw_sr_reference import rand16, sr_bounds
from tests.test_adamw_q8_gpu import Q8Case, _lid

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs a ROCm GPU")]

LAYOUTS = [
    (BF16, BF16, F32, BF16, None),
    (BF16, BF16, BF16, BF16, None),
    (BF16, BF16, E4M3, E5M2, None),
]
SIZES = [1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097]
SEED = 0x5EED0123456789AB
SCALE = 0.37


def _sr_step(cases, steps, ordinals, scale=None):
    """One stochastic-rounding launch over the cases; returns Scalars."""
    from torchdistx_amd import _kernels

    scalars = [Scalars.for_step(t, weight_decay=0.01) for t in steps]
    cols = [list(col) for col in zip(*(c.kernel_lists() for c in cases))]
    s0 = scalars[0]
    _kernels.anyprecision_adamw_q8_(
        *cols, s0.lr, s0.beta1, s0.beta2, s0.eps, s0.weight_decay,
        [s.step_size for s in scalars],
        [s.bias_correction2_sqrt for s in scalars],
        None if scale is None else torch.tensor([scale], device="cuda"),
        SEED, ordinals, steps)
    torch.cuda.synchronize()
    return scalars


def _check(case, s, step, ordinal, scale=None, where="", spans=None):
    """States to the bounds of check_q8_step; a bf16 parameter between the
    codes the recipe gives exact -/+ K * 2^-24 * mag, on the index ranges
    `spans` (default: everywhere)."""
    case.base.assert_guards_and_grad_intact(where)
    p0, g0 = case.base.before()[:2]
    if scale is not None:
        g0 = g0.double() * torch.tensor(scale, dtype=F32).double()
    (m0, ms0), (v0, vs0) = case._state("m", True), case._state("v", True)
    ex = reference_step(p0, g0,
                        m0 if ms0 is None else dequantize(m0, ms0),
                        v0 if vs0 is None else dequantize(v0, vs0), None, s)
    p1 = case.base.views["p"]
    sr = p1.dtype == BF16
    # (For the state bounds a bf16 parameter is stood in for by the
    # reference's own; it has its bound below.)
    check_q8_step(
        (p0, g0, m0, ms0, v0, vs0, None),
        (ex.p.to(F32).to(BF16) if sr else p1, *case._state("m", False),
         *case._state("v", False), None), s, where=where)
    if not sr or case.n == 0:
        return
    tol = K_ROUNDINGS * 2.0**-24 * (ex.p_decayed.abs() + ex.update.abs())
    differ = 0
    for lo_i, hi_i in spans or [(0, case.n)]:
        sl = slice(lo_i, hi_i)
        r = rand16(SEED, step, ordinal, range(lo_i, hi_i))
        lo, hi = sr_bounds(ex.p[sl].cpu().numpy(), tol[sl].cpu().numpy(), r)
        out = p1[sl].double().cpu().numpy()
        bad = ~((lo <= out) & (out <= hi))
        assert not bad.any(), (
            f"{where}: {bad.sum()} parameters outside the stochastic "
            f"rounding bounds, first at {lo_i + int(bad.argmax())}")
        differ += int((lo != hi).sum())
    total = sum(b - a for a, b in spans or [(0, case.n)])
    print(where, "bounds differ for", differ, "of", total)
    # Otherwise the bounds pin nothing (expected: 2K / 65536, about 0.1 %).
    assert differ < 0.01 * total, f"{where}: {differ} of {total} not pinned"


@pytest.mark.parametrize("scale", [None, SCALE], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("step", [1, 1000], ids=["step1", "step1000"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
@pytest.mark.parametrize("n", SIZES)
def test_exact_bits(n, layout, step, scale) -> None:
    case = Q8Case(n, layout, step == 1, seed=3000 + n)
    (s,) = _sr_step([case], [step], [3], scale)
    _check(case, s, step, 3, scale, f"{_lid(layout)} n={n} step={step}")


def test_mixed_list_ordinals_offset_view_and_fp32_parameter() -> None:
    # An empty tensor, a parameter view off the 16-byte alignment (the
    # element-wise path: same bits as a function of i) and an fp32
    # parameter, which is stored as ever.
    specs = [(300, LAYOUTS[0], ()), (0, LAYOUTS[1], ()),
             (2 * 2048 + 77, LAYOUTS[2], ("p",)),
             (2049, (F32, BF16, E4M3, E5M2, None), ()),
             (4097, LAYOUTS[1], ("p", "g", "m"))]
    steps = [1, 5, 1000, 7, 2]
    ordinals = [4, 0, 9, 2, 70000]
    for scale in (None, SCALE):
        cases = [Q8Case(n, layout, t == 0, 3100 + t, misalign=mis)
                 for t, (n, layout, mis) in enumerate(specs)]
        assert cases[2].base.views["p"].data_ptr() % 16 != 0
        scalars = _sr_step(cases, steps, ordinals, scale)
        for t, (case, s) in enumerate(zip(cases, scalars)):
            _check(case, s, steps[t], ordinals[t], scale,
                   f"tensor {t} n={case.n} {_lid(case.layout)}")


def test_grid_wraps() -> None:
    # One virtual block more than the capped grid, and a partial one. The
    # states are checked everywhere, the parameter's bits at both ends of
    # the first pass over the grid and in the wrapped blocks.
    n = 16384 * 2048 + 2048 + 5
    case = Q8Case(n, LAYOUTS[2], False, seed=3200)
    (s,) = _sr_step([case], [1000], [1])
    _check(case, s, 1000, 1, where="grid wrap",
           spans=[(0, 4096), (16383 * 2048, n)])


def test_unbiased_where_round_to_nearest_stalls() -> None:
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    n, steps, lr = 4096, 200, 1e-4

    def run(dtype, **kw):
        p = torch.nn.Parameter(torch.ones(n, device="cuda", dtype=dtype))
        opt = AnyPrecisionAdamW([p], lr=lr, weight_decay=0.0, **kw)
        p.grad = torch.ones_like(p)
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        assert opt._fused_steps == steps
        return p.detach().double()

    # Every update is lr = 1e-4, below half the bf16 spacing under 1.0
    # (2^-9 ~ 2e-3): round-to-nearest never leaves 1.0.
    assert (run(BF16) == 1.0).all()
    want = run(F32).mean().item()
    assert 0.975 < want < 0.985  # 1 - steps * lr, under a bf16 variance
    got = run(BF16, stochastic_rounding=True, stochastic_rounding_seed=1)
    # Each stored value is unbiased with a rounding variance of at most
    # ulp^2 / 4 per step, ulp = 2^-8 (the spacing just below 1.0, where
    # the values live). The T = 200 roundings of an element add up to a
    # variance of at most T ulp^2 / 4, and the mean over n = 4096
    # independent elements has sigma <= ulp / 2 * sqrt(T / n)
    # = 2^-9 * sqrt(200 / 4096) ~ 4.3e-4, against a drift of 0.02.
    sigma = 2.0**-9 * (steps / n) ** 0.5
    print("mean", got.mean().item(), "fp32", want, "sigma", sigma)
    assert abs(got.mean().item() - want) < 6 * sigma


# (States no wider than the parameters: the base class's load_state_dict
# takes a wider one through the parameter dtype.)
@pytest.mark.parametrize("m_dt, v_dt", [(BF16, BF16), (E4M3, E5M2)],
                         ids=["bf16", "fp8"])
def test_determinism_and_checkpoint(m_dt, v_dt) -> None:
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    sizes = [300, 5000, (1 << 20) + 7]

    def make(seed):
        gen = torch.Generator(device="cuda").manual_seed(3300)
        params = [torch.nn.Parameter(torch.randn(
            k, device="cuda", generator=gen).to(BF16)) for k in sizes]
        opt = AnyPrecisionAdamW(
            [{"params": params[:1]}, {"params": params[1:]}], lr=1e-3,
            weight_decay=0.01, momentum_dtype=m_dt, variance_dtype=v_dt,
            max_grad_norm=1.0, stochastic_rounding=True,
            stochastic_rounding_seed=seed)
        return params, opt

    def step(params, opt, t):
        gen = torch.Generator(device="cuda").manual_seed(3310 + t)
        for p in params:
            p.grad = torch.randn(p.numel(), device="cuda",
                                 generator=gen).to(BF16)
        opt.step()

    (pa, oa), (pb, ob), (pc, oc) = make(5), make(5), make(6)
    for t in range(3):
        for params, opt in ((pa, oa), (pb, ob), (pc, oc)):
            step(params, opt, t)
    assert oa._fused_steps == 3 * len(sizes)
    assert all("compensation" not in oa.state[p] for p in pa)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert not any(torch.equal(a, c) for a, c in zip(pa, pc))

    # A resumed run continues bit for bit; the seed travels in the groups.
    twins = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    resumed = AnyPrecisionAdamW(
        [{"params": twins[:1]}, {"params": twins[1:]}], momentum_dtype=m_dt,
        variance_dtype=v_dt, max_grad_norm=1.0)
    resumed.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert resumed.param_groups[1]["stochastic_rounding"] is True
    assert resumed.param_groups[1]["stochastic_rounding_seed"] == 5
    step(pa, oa, 3)
    step(twins, resumed, 3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(pa, twins))
