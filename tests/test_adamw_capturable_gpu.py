# GPU (MI355X) tests of the graph-capturable AnyPrecisionAdamW step
# (capturable=True; csrc/hip/anyprecision_adamw_resident.hip): the scalars
# the advance kernel forms against the host's, the step against the fp64
# references of tests/_adamw_*_reference.py, a graph replay against the eager
# step bit for bit, and a resumed run.

import copy

import pytest
import torch

from tests._adamw_reference import (
    ALL_F32, BF16, F32, FLAGSHIP, K_ROUNDINGS, Case, Scalars, reference_step)
from tests._adamw_q8_reference import (
    E4M3, E5M2, FP8, check_q8_step, dequantize, quantize)
from tests._adamw_sr_reference import rand16, sr_bounds

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs a ROCm GPU")]

# name: ((param, grad, exp_avg, exp_avg_sq, compensation), stochastic)
LAYOUTS = {
    "all-fp32": (ALL_F32, False),
    "flagship": (FLAGSHIP, False),
    "fp8": ((BF16, BF16, E4M3, E5M2, None), False),
    "fp8-sr": ((BF16, BF16, E4M3, E5M2, None), True),
}
# A lone element, a straddling lane, both sides of a virtual-block edge,
# three blocks; the last is a view off the 16-byte alignment.
SIZES = [1, 7, 2047, 2049, 4097, 3]
KEYS = ("exp_avg", "exp_avg_scale", "exp_avg_sq", "exp_avg_sq_scale",
        "compensation")
LR, SEED = 1e-3, 0x5EED0123456789AB
LR32 = torch.tensor(LR, dtype=F32).item()  # what a tensor lr holds


def _optimizer(params, name, lr=LR, **kw):
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    layout, sr = LAYOUTS[name]
    return AnyPrecisionAdamW(
        params, lr=lr, weight_decay=0.01, capturable=True,
        use_kahan_summation=layout[4] is not None, momentum_dtype=layout[2],
        variance_dtype=layout[3], compensation_buffer_dtype=layout[4] or BF16,
        stochastic_rounding=sr, stochastic_rounding_seed=SEED if sr else None,
        **kw)


def _make(name, start=None, lr=LR, **kw):
    """One group over SIZES, parameters and gradients views into guarded
    buffers; with `start`, states as after start - 1 steps (else the
    optimizer creates them)."""
    layout = LAYOUTS[name][0]
    plain = tuple(F32 if d in FP8 else d for d in layout)
    cases = [Case(n, plain, start in (None, 1), "cuda", 5000 + i,
                  misalign=("p", "g") if i == len(SIZES) - 1 else ())
             for i, n in enumerate(SIZES)]
    params = [torch.nn.Parameter(c.views["p"]) for c in cases]
    assert params[-1].data_ptr() % 16 != 0
    opt = _optimizer(params, name, lr, **kw)
    for p, c in zip(params, cases):
        p.grad = c.views["g"]
        if start is None:
            continue
        state = {"step": torch.tensor(start - 1.0, device="cuda")}
        for key, v, dtype in (("exp_avg", "m", layout[2]),
                              ("exp_avg_sq", "v", layout[3])):
            state[key] = c.views[v]
            if dtype in FP8:
                state[key], state[key + "_scale"] = quantize(
                    c.views[v], dtype, variance=v == "v")
        if layout[4] is not None:
            state["compensation"] = c.views["c"]
        opt.state[p] = state
    return cases, params, opt


def _snapshot(params, opt):
    """Per parameter (p, g, m, m_scale, v, v_scale, c, step), cloned."""
    return [(p.detach().clone(), p.grad.clone(),
             *(opt.state[p][k].clone() if k in opt.state[p] else None
               for k in KEYS), opt.state[p]["step"].clone()) for p in params]


def _assert_bitwise_equal(a, b):
    for row_a, row_b in zip(a, b):
        for x, y in zip(row_a, row_b):
            assert (x is None) == (y is None)
            assert x is None or (x.dtype == y.dtype and torch.equal(
                x.reshape(-1).view(torch.uint8),
                y.reshape(-1).view(torch.uint8)))


@pytest.mark.parametrize("lr_as", ["float", "tensor"])
@pytest.mark.parametrize("t", [1, 2, 3, 10, 1000, 100000])
def test_scalars_within_one_ulp_of_the_host(t, lr_as) -> None:
    lr = LR if lr_as == "float" else torch.tensor([LR], device="cuda")
    _, params, opt = _make("flagship", start=t, lr=lr)
    opt.step()
    step_size, bc2, step, decay = opt._resident_plans[0][1].scalars()
    lr = LR if lr_as == "float" else LR32
    want = Scalars.for_step(t, lr=lr, weight_decay=0.01)
    assert (step == t).all() and step.numel() == len(SIZES)
    assert all(opt.state[p]["step"].item() == t for p in params)
    for got, host in ((step_size, want.step_size),
                      (bc2, want.bias_correction2_sqrt),
                      (decay, 1.0 - lr * 0.01)):
        host = torch.tensor(host, dtype=torch.float64).to(F32)
        ulps = (got.view(torch.int32) - host.view(torch.int32)).abs().max()
        print(t, lr_as, got[0].item(), host.item(), "ulps", int(ulps))
        assert ulps <= 1


def _check(name, params, opt, before, t, scale=None):
    """Every output of step t to the bounds of check_q8_step; a
    stochastically rounded parameter between the codes the recipe gives
    exact -/+ K * 2^-24 * mag. Returns {output: K needed}."""
    s = Scalars.for_step(t, lr=LR, weight_decay=0.01)
    differ = total = 0
    worst = {}
    for i, (p, (p0, g0, m0, ms0, v0, vs0, c0, _)) in enumerate(
            zip(params, before)):
        if scale is not None:
            g0 = g0.double() * scale  # the exactly scaled gradient
        p1, st = p.detach(), opt.state[p]
        sr = LAYOUTS[name][1] and p1.dtype == BF16
        ex = reference_step(p0, g0, m0 if ms0 is None else dequantize(m0, ms0),
                            v0 if vs0 is None else dequantize(v0, vs0), c0, s)
        needed = check_q8_step(
            (p0, g0, m0, ms0, v0, vs0, c0),
            (ex.p.to(F32).to(BF16) if sr else p1, *(st.get(k) for k in KEYS)),
            s, where=f"{name} n={p.numel()} step={t}")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in needed.items()}
        if sr:
            tol = K_ROUNDINGS * 2.0**-24 * (ex.p_decayed.abs()
                                            + ex.update.abs())
            lo, hi = sr_bounds(ex.p.cpu().numpy(), tol.cpu().numpy(),
                               rand16(SEED, t, i, range(p.numel())))
            out = p1.double().cpu().numpy()
            assert ((lo <= out) & (out <= hi)).all(), (name, p.numel(), t)
            differ, total = differ + int((lo != hi).sum()), total + p.numel()
    print(name, "step", t, "K needed", worst, "brackets open", differ, total)
    # Otherwise the brackets pin nothing (expected: 2K / 65536, about 0.1 %).
    assert total == 0 or differ < 0.01 * total
    return worst


@pytest.mark.parametrize("start", [1, 1000], ids=["fresh", "from999"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_eager_steps_against_fp64(name, start) -> None:
    cases, params, opt = _make(name, start=start)
    steps = 3 if start == 1 else 1
    for t in range(start, start + steps):
        before = _snapshot(params, opt)
        opt.step()
        torch.cuda.synchronize()
        _check(name, params, opt, before, t)
        for c in cases:
            c.assert_guards_and_grad_intact(f"{name} step {t}")
    assert opt._fused_steps == steps * len(SIZES)
    assert all(opt.state[p]["step"].item() == start + steps - 1
               for p in params)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_graph_replay_is_the_eager_step_bit_for_bit(name) -> None:
    runs = [_make(name, lr=torch.full((1,), LR, device="cuda"))
            for _ in range(2)]
    (_, pa, oa), (_, pb, ob) = runs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
        ob.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    gen = torch.Generator(device="cuda").manual_seed(5100)
    for k in range(3):
        for a, b in zip(pa, pb):
            g = 1e-2 * torch.randn(a.numel(), device="cuda", generator=gen)
            a.grad.copy_(g)
            b.grad.copy_(g)
        for opt in (oa, ob):
            opt.param_groups[0]["lr"].fill_(LR * (k + 2))
        graph.replay()
        ob.step()
        torch.cuda.synchronize()
        _assert_bitwise_equal(_snapshot(pa, oa), _snapshot(pb, ob))
    assert all(o.state[p]["step"].item() == 4
               for o, ps in ((oa, pa), (ob, pb)) for p in ps)


def _round_wide_momentum(params, opt):
    """The base class's load_state_dict takes a state wider than the
    parameter (flagship: fp32 exp_avg, bf16 parameter) through the parameter
    dtype. The run that is not interrupted takes the same rounding, in
    place; every other state comes back as it was saved."""
    for p in params:
        m = opt.state[p]["exp_avg"]
        if m.dtype == F32 and p.dtype == BF16:
            m.copy_(m.to(BF16))


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_resumed_run_continues_bit_for_bit(name) -> None:
    _, params, opt = _make(name)
    opt.step()
    opt.step()
    _round_wide_momentum(params, opt)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    resumed = _optimizer(twins, name)
    resumed.load_state_dict(copy.deepcopy(opt.state_dict()))
    for p, q in zip(params, twins):
        q.grad = p.grad.clone()
    # Then the other way round, into an optimizer that has a plan: the load
    # drops it, and the next step builds one over the loaded tensors.
    for a, pa, b, pb, t in ((opt, params, resumed, twins, 3),
                            (resumed, twins, opt, params, 4)):
        for q in pb:
            step = b.state[q]["step"]
            assert step.dtype == F32 and step.dim() == 0 and step.is_cuda
        assert not b._resident_plans
        a.step()
        b.step()
        torch.cuda.synchronize()
        _assert_bitwise_equal(_snapshot(pa, a), _snapshot(pb, b))
        assert all(b.state[q]["step"].item() == t for q in pb)
        _round_wide_momentum(pb, b)
        a.load_state_dict(copy.deepcopy(b.state_dict()))


def test_max_grad_norm_outside_capture() -> None:
    _, params, opt = _make("flagship", start=1000, max_grad_norm=1e-3)
    before = _snapshot(params, opt)
    opt.step()
    torch.cuda.synchronize()
    assert opt.grad_clip_coef < 1
    _check("flagship", params, opt, before, 1000,
           scale=opt.grad_clip_coef.double())


def test_capture_without_a_warm_up_step_is_refused(monkeypatch) -> None:
    _, params, opt = _make("flagship")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing",
                        lambda: True)
    with pytest.raises(RuntimeError, match="run one eager step first and "
                       "keep gradients in place"):
        opt.step()
    assert all(len(opt.state[p]) == 0 for p in params)
    opt.max_grad_norm = 1.0
    with pytest.raises(RuntimeError, match="max_grad_norm cannot be "
                       "captured"):
        opt.step()
