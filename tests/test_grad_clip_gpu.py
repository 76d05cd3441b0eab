# GPU (MI355X) tests of fused gradient clipping: the norm kernels of
# csrc/hip/grad_norm.hip against an fp64 reference, and the three step
# kernels under a device-resident gradient scale against
# tests/_adamw_reference.py and tests/_adamw_q8_reference.py.

import pytest
import torch

from tests._adamw_reference import (
    ALL_F32, BF16, F16, F32, FLAGSHIP, Case, Scalars, check_step, layout_id)
from tests._adamw_q8_reference import E4M3, check_q8_step, quantize

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs a ROCm GPU")]

INF, NAN = float("inf"), float("nan")
# One fp32 rounding of the output (2^-24), doubled for the order of the fp64
# summation; its n * 2^-53 is negligible at these sizes.
REL = 2.0**-23

LISTS = [(1,), (7,), (2047, 2049), (3 * 2048 + 5, 0, 8), "misaligned",
         "over_cap"]


def _grads(kind, dtype, scale=1.0, seed=7):
    from torchdistx_amd import _kernels

    gen = torch.Generator(device="cuda").manual_seed(seed)

    def rnd(n):
        g = torch.randn(n, generator=gen, device="cuda") * scale
        return g.to(dtype)

    if kind == "misaligned":  # storage offset of one element
        return [rnd(2050)[1:]]
    if kind == "over_cap":  # more one-element tensors than the grid cap
        return list(rnd(_kernels._K.grad_norm_grid_cap() + 3).split(1))
    return [rnd(n) for n in kind]


def _norm_coef(grads, max_norm):
    from torchdistx_amd import _kernels

    out = torch.full((2,), -1.0, device="cuda")
    _kernels.grad_norm_clip_coef_(grads, max_norm, out)
    norm = torch.cat([g.double() for g in grads]).square().sum().sqrt()
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return out.double(), torch.stack([norm, coef])


@pytest.mark.parametrize("kind", LISTS, ids=str)
@pytest.mark.parametrize("dtype,scale", [
    (F32, 1.0), (BF16, 1.0), (F16, 1.0),
    (F32, 1e-25), (F32, 1e25),  # squares underflow / overflow fp32
], ids=["f32", "bf16", "f16", "f32-tiny", "f32-huge"])
def test_norm_and_coef_against_fp64(kind, dtype, scale) -> None:
    grads = _grads(kind, dtype, scale)
    out, ref = _norm_coef(grads, 0.25 * scale)
    print(kind, dtype, scale, "rel err", ((out - ref).abs() / ref).tolist())
    assert ((out - ref).abs() <= REL * ref.abs()).all(), (out, ref)


def test_norm_of_mixed_dtypes() -> None:
    grads = [_grads((n,), d, seed=n)[0]
             for n, d in ((2049, F32), (300, BF16), (4097, F16), (5, BF16))]
    out, ref = _norm_coef(grads, 1.0)
    assert ((out - ref).abs() <= REL * ref.abs()).all(), (out, ref)


@pytest.mark.parametrize("bad", [INF, NAN], ids=["inf", "nan"])
def test_non_finite_gradient_behaves_as_clip_grad_norm(bad) -> None:
    grads = _grads((2049, 7), BF16)
    grads[0][100] = bad
    out, _ = _norm_coef(grads, 1.0)
    if bad == INF:
        assert out[0] == INF and out[1] == 0
    else:
        assert out.isnan().all()


# ---------------------------------------------------------------------------
# The step kernels under the clip coefficient, through the public optimizer
# ---------------------------------------------------------------------------

# kernel: (sizes, fp8 momentum). 2^20 + 9: vector path and tail of the
# per-tensor kernel; smaller tensors batch; an fp8 state takes the q8 kernel.
KERNELS = {"vec": ([2**20 + 9], False), "batched": ([1, 2049], False),
           "q8": ([257, 2049], True)}
KEYS = ("exp_avg", "exp_avg_scale", "exp_avg_sq", "exp_avg_sq_scale",
        "compensation")
HYPER = dict(lr=1e-3, weight_decay=0.01)


def _optimizer(kernel, layout, kahan, step, **kw):
    """Parameters with gradients and states of `step - 1` steps."""
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    sizes, q8 = KERNELS[kernel]
    layout = layout[:4] + ((layout[4] or BF16) if kahan else None,)
    cases = [Case(n, layout, step == 1, "cuda", 3000 + n) for n in sizes]
    params = [torch.nn.Parameter(c.views["p"].clone()) for c in cases]
    opt = AnyPrecisionAdamW(
        params, use_kahan_summation=kahan, use_fused=True,
        momentum_dtype=E4M3 if q8 else layout[2], variance_dtype=layout[3],
        compensation_buffer_dtype=layout[4] or BF16, **HYPER, **kw)
    for p, c in zip(params, cases):
        p.grad = c.views["g"].clone()
        state = {"step": torch.tensor(step - 1.0),
                 "exp_avg": c.views["m"].clone(),
                 "exp_avg_sq": c.views["v"].clone()}
        if q8:
            state["exp_avg"], state["exp_avg_scale"] = quantize(
                c.views["m"], E4M3, variance=False)
        if kahan:
            state["compensation"] = c.views["c"].clone()
        opt.state[p] = state
    return params, opt


def _snapshot(params, opt):
    return [(p.detach().clone(), p.grad.clone(),
             *(opt.state[p][k].clone() if k in opt.state[p] else None
               for k in KEYS)) for p in params]


def _raw(t):
    return t if t is None else t.view(torch.uint8)


@pytest.mark.parametrize("step", [1, 1000], ids=["step1", "step1000"])
@pytest.mark.parametrize("kahan", [False, True], ids=["plain", "kahan"])
@pytest.mark.parametrize("layout", [FLAGSHIP, ALL_F32], ids=layout_id)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_clipped_step(kernel, layout, kahan, step) -> None:
    params, opt = _optimizer(kernel, layout, kahan, step, max_grad_norm=1e-3)
    before = _snapshot(params, opt)
    opt.step()
    torch.cuda.synchronize()
    coef = opt.grad_clip_coef.double()
    assert coef < 1 and opt._fused_steps == len(params)
    scalars = Scalars.for_step(step, **HYPER)
    for p, (p0, g, m0, ms0, v0, vs0, c0) in zip(params, before):
        assert torch.equal(_raw(p.grad), _raw(g)), "p.grad was written"
        g0 = g.double() * coef  # the exactly scaled gradient
        m1, ms1, v1, vs1, c1 = (opt.state[p].get(k) for k in KEYS)
        where = (f"{kernel} {layout_id(layout)} kahan={kahan} "
                 f"n={p.numel()} step={step}")
        if kernel == "q8":
            needed = check_q8_step((p0, g0, m0, ms0, v0, vs0, c0),
                                   (p.detach(), m1, ms1, v1, vs1, c1),
                                   scalars, where=where)
        else:
            needed = check_step((p0, g0, m0, v0, c0),
                                (p.detach(), m1, v1, c1), scalars,
                                where=where)
        print(where, "K needed", needed)


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_inactive_clip_is_invisible(kernel) -> None:
    runs = []
    for kw in ({}, {"max_grad_norm": 1e30}):
        params, opt = _optimizer(kernel, FLAGSHIP, True, 1000, **kw)
        opt.step()
        torch.cuda.synchronize()
        runs.append(_snapshot(params, opt))
    assert opt.grad_clip_coef == 1.0
    for plain, clipped in zip(*runs):
        for a, b in zip(plain, clipped):
            assert (a is None) == (b is None)
            assert a is None or torch.equal(_raw(a), _raw(b))


def test_use_fused_true_with_a_cpu_parameter_raises() -> None:
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    p = torch.nn.Parameter(torch.ones(8))
    p.grad = torch.ones(8)
    opt = AnyPrecisionAdamW([p], use_fused=True, max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match="max_grad_norm cannot run"):
        opt.step()
