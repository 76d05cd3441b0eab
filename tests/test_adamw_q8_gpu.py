# GPU (MI355X) tests of the block-scaled fp8 AnyPrecisionAdamW step against
# tests/_adamw_q8_reference.py. Operands are views into guarded buffers;
# guards (scale tensors included) and the gradient must stay bit-identical.

import copy

import pytest
import torch

from tests._adamw_reference import (
    BF16, F16, F32, GUARD, Case, Scalars)
from tests._adamw_q8_reference import (
    E4M3, E5M2, FP8, QBLOCK, check_q8_step, dequantize, quantize)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs a ROCm GPU")]

LAYOUTS = [
    (BF16, BF16, E4M3, E5M2, None),
    (BF16, BF16, E4M3, E5M2, BF16),
    (F32, F32, E4M3, E4M3, None),
    (BF16, BF16, F32, E5M2, None),
    (F16, F16, E5M2, BF16, None),
]
SIZES = [1, 255, 256, 257, 2048, 2049, 3 * 2048 + 300]


def _lid(layout):
    return "-".join(str(d).replace("torch.", "") for d in layout)


def _guarded(values, fill):
    """values inside a buffer with GUARD sentinel elements on each side."""
    buf = torch.empty(values.numel() + 2 * GUARD, dtype=values.dtype,
                      device=values.device)
    raw = buf.view(torch.uint8)
    raw.fill_(fill)
    view = buf[GUARD:GUARD + values.numel()]
    view.copy_(values)
    return buf, view


class Q8Case:
    """Case with its fp8 states quantized by the reference quantizer into
    guarded code and scale buffers of their own."""

    def __init__(self, n, layout, first_step, seed, **kw):
        plain = tuple(F32 if d in FP8 else d for d in layout)
        self.base = Case(n, plain, first_step, "cuda", seed, **kw)
        self.n, self.layout = n, layout
        self.q8 = {}
        for name, dtype in (("m", layout[2]), ("v", layout[3])):
            if dtype in FP8:
                codes, scale = quantize(self.base.views[name], dtype,
                                        variance=name == "v")
                bufs = _guarded(codes, 0x7F) + _guarded(scale, 0xFF)
                self.q8[name] = bufs + tuple(
                    b.clone() for b in (bufs[0], bufs[2]))

    def _state(self, name, snapshot):
        if name in self.q8:
            cb, cv, sb, sv, cb0, sb0 = self.q8[name]
            if snapshot:
                return (cb0[GUARD:GUARD + self.n],
                        sb0[GUARD:GUARD + sv.numel()])
            return cv, sv
        view = (self.base.before()["pgmvc".index(name)] if snapshot
                else self.base.views[name])
        return view, None

    def kernel_lists(self):
        v = self.base.views
        return (v["p"], v["g"], *self._state("m", False),
                *self._state("v", False), v["c"])

    def check(self, scalars, where=""):
        self.base.assert_guards_and_grad_intact(where)
        for name, (cb, cv, sb, sv, cb0, sb0) in self.q8.items():
            for buf, was, k in ((cb, cb0, self.n), (sb, sb0, sv.numel())):
                now, old = buf.view(torch.uint8), was.view(torch.uint8)
                lo = GUARD * buf.element_size()
                hi = lo + k * buf.element_size()
                assert torch.equal(now[:lo], old[:lo]) and torch.equal(
                    now[hi:], old[hi:]), f"{where}: guard of {name} written"
        p0, g0, _, _, c0 = self.base.before()
        v = self.base.views
        return check_q8_step(
            (p0, g0, *self._state("m", True), *self._state("v", True), c0),
            (v["p"], *self._state("m", False), *self._state("v", False),
             v["c"]),
            scalars, where=where)


def _step(cases, scalars):
    from torchdistx_amd import _kernels

    cols = list(zip(*(c.kernel_lists() for c in cases)))
    s0 = scalars[0]
    _kernels.anyprecision_adamw_q8_(
        *(list(col) for col in cols), s0.lr, s0.beta1, s0.beta2, s0.eps,
        s0.weight_decay, [s.step_size for s in scalars],
        [s.bias_correction2_sqrt for s in scalars])
    torch.cuda.synchronize()


def _run(n, layout, first, seed, **kw):
    case = Q8Case(n, layout, first, seed, **kw)
    s = Scalars.for_step(1 if first else 1000, weight_decay=0.01)
    _step([case], [s])
    case.check(s, where=f"{_lid(layout)} n={n} first={first}")
    return case


@pytest.mark.parametrize("first", [True, False], ids=["step1", "step1000"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_layouts(n, layout, first) -> None:
    _run(n, layout, first, seed=2000 + n)


def test_mixed_list() -> None:
    sizes = [300, 0, 2 * 2048 + 77, 1, 2048, 255]
    cases, scalars = [], []
    for t, n in enumerate(sizes):
        cases.append(Q8Case(n, LAYOUTS[t % len(LAYOUTS)], t == 0, 2100 + t,
                            misalign=("p", "g")))
        scalars.append(Scalars.for_step(t + 1, weight_decay=0.01))
    assert cases[0].base.views["p"].data_ptr() % 16 != 0
    _step(cases, scalars)
    for t, (case, s) in enumerate(zip(cases, scalars)):
        case.check(s, where=f"tensor {t} n={case.n} {_lid(case.layout)}")


def test_grid_wraps() -> None:
    # One virtual block more than the capped grid, and a partial one.
    _run(16384 * 2048 + 2048 + 5, LAYOUTS[0], False, seed=2200)


@pytest.mark.parametrize("layout", LAYOUTS[:3], ids=_lid)
def test_range_within_a_block(layout) -> None:
    # Block 1: one gradient element 2^20 times the others. Block 2: all
    # zero (g = m = v = 0).
    n = 4 * QBLOCK
    g = torch.full((n,), 1e-3, device="cuda")
    g[QBLOCK + 17] = 1e-3 * 2.0**20
    g[2 * QBLOCK:3 * QBLOCK] = 0.0
    case = Q8Case(n, layout, True, 2300, grad_overrides=[(slice(None), g)])
    s = Scalars.for_step(1, weight_decay=0.01)
    p0, g0 = (t.double() for t in case.base.before()[:2])
    _step([case], [s])
    case.check(s, where=f"range {_lid(layout)}")
    (mc, ms), (vc, vs) = case._state("m", False), case._state("v", False)
    small = slice(QBLOCK, QBLOCK + 17)
    assert (dequantize(vc, vs)[small] > 0).all()
    want_m = quantize(s.narrowed().one_minus_beta1 * g0, layout[2],
                      variance=False)[0]
    assert torch.equal(mc.view(torch.uint8)[small],
                       want_m.view(torch.uint8)[small])
    zero = slice(2 * QBLOCK, 3 * QBLOCK)
    assert ms[2] == 1.0 and vs[2] == 1.0
    assert not mc.view(torch.uint8)[zero].any()
    assert not vc.view(torch.uint8)[zero].any()
    if layout[4] is None:
        decayed = (p0[zero] * s.narrowed().decay).to(F32).to(layout[0])
        assert torch.equal(case.base.views["p"][zero], decayed)


@pytest.mark.parametrize("layout", LAYOUTS[:3], ids=_lid)
def test_non_finite_gradients_stay_in_their_elements(layout) -> None:
    n = 3 * QBLOCK + 9
    bad = [(5, float("inf")), (2 * QBLOCK + 3, float("nan"))]
    case = _run(n, layout, False, 2400, grad_overrides=bad)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    mask[[i for i, _ in bad]] = True
    assert torch.equal(~case.base.views["p"].isfinite(), mask)
    for name in ("m", "v"):
        assert torch.equal(~dequantize(*case._state(name, False)).isfinite(),
                           mask)


def test_optimizer_three_steps_and_state_dict_round_trip() -> None:
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    keys = ("exp_avg", "exp_avg_scale", "exp_avg_sq", "exp_avg_sq_scale",
            "compensation")
    dtypes = (E4M3, F32, E5M2, F32, BF16)

    def make(params):
        return AnyPrecisionAdamW(
            params, lr=1e-3, weight_decay=0.01, use_kahan_summation=True,
            momentum_dtype=E4M3, variance_dtype=E5M2,
            compensation_buffer_dtype=BF16)

    def values(n, seed, name):
        return Case(n, (BF16,) * 5, True, "cuda", seed).views[name].clone()

    params = [torch.nn.Parameter(values(n, 2500 + i, "p"))
              for i, n in enumerate([300, (1 << 20) + 7])]
    opt = make(params)
    for step in (1, 2, 3):
        before = []
        for i, p in enumerate(params):
            p.grad = values(p.numel(), 2510 + 10 * step + i, "g")
            nb = -(-p.numel() // QBLOCK)
            fresh = [torch.ones(nb, device="cuda") if k.endswith("scale")
                     else torch.zeros_like(p, dtype=d)
                     for k, d in zip(keys, dtypes)]
            state = [opt.state[p][k].clone() for k in keys] if step > 1 else fresh
            before.append((p.detach().clone(), p.grad.clone(), *state))
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            st = opt.state[p]
            assert set(st) == {"step", *keys}
            assert tuple(st[k].dtype for k in keys) == dtypes
            assert st["exp_avg"].shape == st["exp_avg_sq"].shape == p.shape
            assert st["exp_avg_scale"].numel() == -(-p.numel() // QBLOCK)
            assert st["exp_avg_sq_scale"].numel() == -(-p.numel() // QBLOCK)
            check_q8_step(before[i], (p.detach(), *(st[k] for k in keys)),
                          Scalars.for_step(step, weight_decay=0.01),
                          where=f"optimizer step {step} n={p.numel()}")
    assert opt._fused_steps == 6

    def bits(t):
        return t.view(torch.uint8) if t.dtype in FP8 else t

    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt2 = make(twins)
    # A deep copy, as a checkpoint is: load_state_dict may keep its tensors.
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    for again in (False, True):
        for p, q in zip(params, twins):
            q.grad = p.grad.clone()
            assert torch.equal(p, q)
            for k, a in opt.state[p].items():
                b = opt2.state[q][k]
                assert a.dtype == b.dtype and torch.equal(bits(a), bits(b)), k
        if not again:
            opt.step()
            opt2.step()
            torch.cuda.synchronize()
