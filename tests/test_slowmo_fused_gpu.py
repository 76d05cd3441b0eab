# The SlowMo kernels (csrc/hip/slowmo.hip) against the fp64 reference of
# tests/_slowmo_reference.py, and SlowMomentumOptimizer(use_fused=True)
# against the eager optimizer on a single-rank RCCL group.
#
# Bounds, with u = 2^-24 and everything on the right in fp64:
#   |m' - m_ref| <= tol_m = 4u (|factor m| + |d_ref| / lr)
#   |p' - q_ref| <= 4u (|prev| + coef |m_ref|) + coef tol_m  [+ ulp_P(q_ref)/2]
# m' takes the roundings of prev - a, of 1/lr, of factor * m and of the fma
# (at most 3u on either term); p' those of coef and of the fma, plus the
# error m' carries in, plus for a 16-bit P the rounding of the store.

import os
import socket

import pytest
import torch

from tests._adamw_reference import BF16, F16, F32, ulp
from tests._slowmo_reference import reference_outer_step, reference_pack
from torchdistx_amd import _kernels
from torchdistx_amd.slowmo import SlowMomentumOptimizer

pytestmark = pytest.mark.gpu

U = 2.0**-24
# Lane tail, virtual-block edge, table search across tensors.
NUMELS = (1, 7, 8, 9, 2047, 2048, 2049)
LRS = (0.1, 0.05)
FACTOR, SLOWMO_LR = 0.5, 0.7
DTYPE_CASES = {"f32": (F32,), "bf16": (BF16,), "f16": (F16,),
               "mixed": (F32, BF16, F16)}


def _view(values, dtype, offset):
    """values as a dtype view at storage offset `offset` (8: 16-byte
    aligned, 1: not) of a buffer whose other elements are sentinels."""
    n = values.numel()
    buf = torch.full((offset + n + 1,), 77.0, device="cuda", dtype=dtype)
    buf[offset:offset + n] = values.to(dtype)
    return buf[offset:offset + n], buf


def _tensors(dtypes):
    """Per tensor (dtype, averaged value, prev, m) with prev about 1e-2
    relative away from the averaged value; the 2048-element tensor's views
    sit at storage offset 1 (the element-wise path)."""
    gen = torch.Generator(device="cuda").manual_seed(11)
    out = []
    for i, n in enumerate(NUMELS):
        dtype = dtypes[i % len(dtypes)]
        a32 = torch.randn(n, generator=gen, device="cuda")
        rel = 1e-2 * torch.randn(n, generator=gen, device="cuda")
        m = 0.1 * torch.randn(n, generator=gen, device="cuda")
        off = 1 if n == 2048 else 8
        out.append((dtype, a32, _view(a32 * (1 + rel), dtype, off),
                    _view(m, F32, off)))
    return out


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _assert_within(name, out, ref, tol):
    err = (out.to(torch.float64) - ref).abs()
    ratio = float((err / tol).max())
    print(f"{name}: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("with_flat", [True, False], ids=["flat", "noflat"])
@pytest.mark.parametrize("dtypes", list(DTYPE_CASES))
def test_outer_step_within_fp32_bounds(dtypes, with_flat):
    tensors = _tensors(DTYPE_CASES[dtypes])
    flat_dtype = torch.float32 if dtypes == "mixed" else DTYPE_CASES[dtypes][0]
    shapes = [torch.empty(n) for n in NUMELS]
    offsets, total = _kernels.slowmo_flat_layout(shapes)
    assert all(o % 8 == 0 for o in offsets) and total % 8 == 0
    flat = torch.zeros(total, device="cuda", dtype=flat_dtype)

    params, prevs, moms, bufs, avgs = [], [], [], [], []
    for (dtype, a32, (prev, prev_buf), (m, m_buf)), off in zip(
            tensors, offsets):
        slot = a32.to(flat_dtype)
        a = slot.to(dtype)  # what the copy-back would have stored
        if with_flat:
            flat[off:off + a.numel()] = slot
            # The kernel must not read the parameter in this mode.
            p, p_buf = _view(torch.full_like(a32, 123.0), dtype,
                             prev.storage_offset())
        else:
            p, p_buf = _view(a, dtype, prev.storage_offset())
        params.append(p), prevs.append(prev), moms.append(m), avgs.append(a)
        bufs += [(p_buf, p), (prev_buf, prev), (m_buf, m)]
    lrs = [LRS[i % 2] for i in range(len(NUMELS))]
    before = [(prev.clone(), m.clone()) for prev, m in zip(prevs, moms)]
    flat_before = flat.clone()

    _kernels.slowmo_outer_step_(params, prevs, moms,
                                flat if with_flat else None, lrs, FACTOR,
                                SLOWMO_LR)

    assert torch.equal(_bits(flat), _bits(flat_before))  # padding included
    for buf, view in bufs:
        assert (buf[:view.storage_offset()] == 77.0).all() and buf[-1] == 77.0
    for i, (a, (prev0, m0), lr) in enumerate(zip(avgs, before, lrs)):
        m_ref, q_ref = reference_outer_step(a, prev0, m0, lr, FACTOR,
                                            SLOWMO_LR)
        d_ref = prev0.to(torch.float64) - a.to(torch.float64)
        coef = SLOWMO_LR * lr
        tol_m = 4 * U * ((FACTOR * m0.to(torch.float64)).abs()
                         + d_ref.abs() / lr)
        tol_p = (4 * U * (prev0.to(torch.float64).abs() + coef * m_ref.abs())
                 + coef * tol_m)
        if a.dtype != F32:
            tol_p = tol_p + 0.5 * ulp(q_ref, a.dtype)
        _assert_within(f"m[{i}]", moms[i], m_ref, tol_m)
        _assert_within(f"p[{i}] {a.dtype}", params[i], q_ref, tol_p)
        assert torch.equal(_bits(prevs[i]), _bits(params[i]))


@pytest.mark.parametrize("world_size", [1, 3])
@pytest.mark.parametrize("dtypes", list(DTYPE_CASES))
def test_pack_matches_cat_div_bitwise(dtypes, world_size):
    params = [_view(a32, dtype, prev.storage_offset())[0]
              for dtype, a32, (prev, _), _ in _tensors(DTYPE_CASES[dtypes])]
    offsets, total = _kernels.slowmo_flat_layout(params)
    expected = reference_pack(params, offsets, total, world_size)
    flat = torch.zeros_like(expected)
    _kernels.slowmo_pack_(params, flat, world_size)
    assert torch.equal(_bits(flat), _bits(expected))


@pytest.fixture()
def rccl_world1():
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        os.environ["MASTER_PORT"] = str(s.getsockname()[1])
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_optimizer_fused_matches_eager(rccl_world1):
    """Two groups, SGD, slowmo_freq=2, 5 steps with fixed gradients: outer
    updates on calls 3 and 5. The eager update rounds a/lr and prev/lr
    before they cancel, an error of order u |a| / lr that the bounds (in
    |d| / lr) do not cover in general; here |p0| << lr |g|, so |a| is of
    the order of |d| and both paths stay inside them."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    shapes, group_lrs = [(33, 65), (7,), (2049,)], (0.3, 0.3, 0.1)
    init = [0.02 * torch.randn(s, generator=gen, device="cuda")
            for s in shapes]
    grads = [(0.5 + torch.rand(s, generator=gen, device="cuda"))
             * (1 - 2 * torch.randint(0, 2, s, generator=gen, device="cuda"))
             for s in shapes]

    def make(use_fused):
        ps = [torch.nn.Parameter(t.clone()) for t in init]
        base = torch.optim.SGD([{"params": ps[:2], "lr": 0.3},
                                {"params": ps[2:], "lr": 0.1}])
        return ps, SlowMomentumOptimizer(base, slowmo_freq=2,
                                         slowmo_factor=FACTOR,
                                         slowmo_lr=SLOWMO_LR,
                                         use_fused=use_fused)

    (pe, eager), (pf, fused) = make(False), make(True)
    tol_m = [torch.zeros_like(t, dtype=torch.float64) for t in init]
    tol_p = [torch.zeros_like(t, dtype=torch.float64) for t in init]
    for call in range(1, 6):
        for ps, opt in ((pe, eager), (pf, fused)):
            for p, g in zip(ps, grads):
                p.grad = g.clone()
        if call in (3, 5):  # the bounds of this outer step, from eager
            for i, (p, g, lr) in enumerate(zip(pe, grads, group_lrs)):
                m = eager.state[p].get("slow_momentum", torch.zeros_like(p))
                prev = eager._prev_parameters[i].to(torch.float64)
                d = prev - (p.detach().to(torch.float64) - lr * g)
                fm = FACTOR * m.to(torch.float64)
                tm = 4 * U * (fm.abs() + d.abs() / lr)
                coef = SLOWMO_LR * lr
                tol_m[i] += tm
                tol_p[i] += (4 * U * (prev.abs() + coef * (fm + d / lr).abs())
                             + coef * tm)
        eager.step()
        fused.step()

    assert fused._fused_outer_steps == 2 and eager._fused_outer_steps == 0
    assert fused.averager.step == eager.averager.step == 5
    for i, (a, b) in enumerate(zip(pe, pf)):
        assert eager.state[a].keys() == fused.state[b].keys()
        _assert_within(f"e2e m[{i}]", fused.state[b]["slow_momentum"],
                       eager.state[a]["slow_momentum"].to(torch.float64),
                       tol_m[i])
        _assert_within(f"e2e p[{i}]", b.detach(),
                       a.detach().to(torch.float64), tol_p[i])
        assert torch.equal(fused._prev_parameters[i], b.detach())

    sd = fused.state_dict()
    _, fresh = make(True)
    fresh.load_state_dict(sd)
    assert fresh.averager.step == 5 and fresh.slowmo_freq == 2
    again = fresh.state_dict()
    assert again.keys() == sd.keys()
    for k, st in sd["state"].items():
        assert torch.equal(again["state"][k]["slow_momentum"],
                           st["slow_momentum"])
