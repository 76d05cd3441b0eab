# GPU (MI355X) tests of clipping and GradScaler skipping inside the
# capturable AnyPrecisionAdamW step: the resident norm pass and its finalize
# (csrc/hip/grad_norm.hip) against fp64, the captured step against the eager
# one bit for bit and against the fp64 step reference, the step that skips
# itself, and torch.amp.GradScaler end to end.

import pytest
import torch

from tests._adamw_reference import BF16, F16, F32, Case
from tests._adamw_q8_reference import FP8
from tests.test_adamw_capturable_gpu import (
    LAYOUTS, LR, SIZES, _assert_bitwise_equal, _check, _optimizer, _snapshot)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs a ROCm GPU")]

# One fp32 rounding of the output (2^-24), doubled for the order of the fp64
# summation: the bound of tests/test_grad_clip_gpu.py.
REL = 2.0**-23
SCALE = 65536.0
# Below the norm of the Case gradients (taken as the scaled ones) over SCALE,
# so that the step clips: the 16-bit float layouts draw narrower gradients.
MAX_NORM = {F32: 1e-4, BF16: 1e-4, F16: 1e-5}


def _cuda(x):
    return torch.tensor(float(x), device="cuda")


def _make(name, grad_dtype, groups=2, amp=True, **kw):
    """SIZES (the last a view off 16-byte alignment) over `groups` param
    groups, so that two plans share one partials buffer; with `amp`, a loss
    scale and a clear found_inf set as a GradScaler would."""
    layout = LAYOUTS[name][0]
    plain = tuple(F32 if d in FP8 else d for d in layout)
    plain = (plain[0], grad_dtype) + plain[2:]
    cases = [Case(n, plain, True, "cuda", 5200 + i,
                  misalign=("p", "g") if n == 3 else ())
             for i, n in enumerate(SIZES)]
    params = [torch.nn.Parameter(c.views["p"]) for c in cases]
    split = [params] if groups == 1 else [params[:3], params[3:]]
    opt = _optimizer([{"params": ps} for ps in split], name,
                     max_grad_norm=MAX_NORM[grad_dtype], **kw)
    for p, c in zip(params, cases):
        p.grad_dtype = None  # the gradient's dtype is the case's, not p's
        p.grad = c.views["g"]
    if amp:
        opt.grad_scale, opt.found_inf = _cuda(SCALE), _cuda(0)
    return params, opt


def _expected(grads, max_norm, scale):
    """[norm, coef, grad_mult] in fp64."""
    norm = torch.cat([g.double().reshape(-1) for g in grads]
                     ).square().sum().sqrt() / scale
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return torch.stack([norm, coef, coef / scale])


@pytest.mark.parametrize("scale", [None, SCALE], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_norm_coef_and_multiplier_against_fp64(dtype, scale) -> None:
    params, opt = _make("flagship", dtype, amp=False)
    if scale is not None:
        opt.grad_scale = _cuda(scale)
    opt.step()
    out = opt._norm_buffers[1].double()
    ref = _expected([p.grad for p in params], MAX_NORM[dtype], scale or 1.0)
    print(dtype, scale, "rel err", ((out[:3] - ref).abs() / ref).tolist())
    assert ((out[:3] - ref).abs() <= REL * ref).all(), (out, ref)
    assert ref[1] < 1 and out[3] == 0
    assert opt.grad_norm.data_ptr() == opt._norm_buffers[1].data_ptr()


@pytest.mark.parametrize("kind", ["sizes", "over_cap"])
def test_one_group_is_the_list_kernel_bit_for_bit(kind) -> None:
    from torchdistx_amd import _kernels

    if kind == "sizes":
        params, opt = _make("flagship", BF16, groups=1, amp=False)
    else:  # one-element tensors, more virtual blocks than the grid
        n = _kernels._K.grad_norm_grid_cap() + 3
        params = [torch.nn.Parameter(t) for t in torch.zeros(
            n, device="cuda").split(1)]
        opt = _optimizer(params, "all-fp32", max_grad_norm=1e-3)
    gen = torch.Generator(device="cuda").manual_seed(5300)
    # The second round after zero_grad(set_to_none=True): a rebound plan.
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        for p in params:
            p.grad = torch.randn(p.numel(), device="cuda",
                                 generator=gen).to(p.dtype)
        opt.step()
        grads = [p.grad for p in params]
        want = torch.full((2,), -1.0, device="cuda")
        _kernels.grad_norm_clip_coef_(grads, opt.max_grad_norm, want)
        got = opt._norm_buffers[1]
        assert torch.equal(got[:2].view(torch.int32), want.view(torch.int32))
        ref = _expected(grads, opt.max_grad_norm, 1.0)
        assert ((got[:3].double() - ref).abs() <= REL * ref).all()
    assert opt._resident_plans[0][1].grad_grid() == min(
        _kernels._K.grad_norm_grid_cap(),
        sum(-(-p.numel() // 2048) for p in params))


def _twins(name, dtype):
    """Two equal optimizers after one eager step with tensor lr, loss scale
    and found_inf, and the snapshot before it; the first's next step
    captured. A step skipped ahead of it all leaves the states it creates
    at zero and the step counts at 0."""
    runs = [_make(name, dtype, lr=torch.full((1,), LR, device="cuda"))
            for _ in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _, opt in runs:
            opt.found_inf.fill_(1)
            opt.step()
            opt.found_inf.fill_(0)
        before = _snapshot(*runs[0])
        assert all(row[-1] == 0 for row in before)
        for _, opt in runs:
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        runs[0][1].step()
    return runs, graph, before


def _assert_same(a, b):
    torch.cuda.synchronize()
    _assert_bitwise_equal(_snapshot(*a), _snapshot(*b))
    _assert_bitwise_equal([a[1]._norm_buffers[1:2]], [b[1]._norm_buffers[1:2]])


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["flagship", "fp8-sr"])
def test_captured_clipped_scaled_step(name, dtype) -> None:
    (a, b), graph, before = _twins(name, dtype)
    _assert_same(a, b)
    out = a[1]._norm_buffers[1]
    assert out[1] < 1 and out[3] == 0
    # The first step at the stock K, under the kernel's own multiplier.
    _check(name, a[0], a[1], before, 1, scale=out[2].double())
    gen = torch.Generator(device="cuda").manual_seed(5400)
    for k in range(3):
        for p, q in zip(a[0], b[0]):
            g = 1e-2 * torch.randn(p.numel(), device="cuda", generator=gen)
            p.grad.copy_(g)
            q.grad.copy_(g)
        for _, opt in (a, b):
            opt.param_groups[0]["lr"].fill_(LR * (k + 2))
            opt.grad_scale.fill_(SCALE / 2 ** (k + 1))
        graph.replay()
        b[1].step()
        _assert_same(a, b)
        # Fresh values behind the views handed out before the capture.
        ref = _expected([p.grad for p in a[0]], a[1].max_grad_norm,
                        SCALE / 2 ** (k + 1))
        got = torch.stack([a[1].grad_norm, a[1].grad_clip_coef]).double()
        assert ((got - ref[:2]).abs() <= REL * ref[:2]).all()
    assert all(o.state[p]["step"].item() == 4 for ps, o in (a, b) for p in ps)


@pytest.mark.parametrize("name", ["flagship", "fp8-sr"])
def test_found_inf_skips_the_step_on_the_device(name) -> None:
    (a, b), graph, _ = _twins(name, BF16)
    a[1].found_inf.fill_(1)
    a[0][4].grad[100] = float("inf")
    before = _snapshot(*a)
    for step in (a[1].step, graph.replay):
        step()
        torch.cuda.synchronize()
        _assert_bitwise_equal(_snapshot(*a), before)
    assert a[1]._norm_buffers[1][3] == 1
    a[0][4].grad.copy_(b[0][4].grad)
    a[1].found_inf.fill_(0)
    graph.replay()
    b[1].step()
    _assert_same(a, b)
    assert all(o.state[p]["step"].item() == 2 for ps, o in (a, b) for p in ps)


def test_grad_scaler_skips_and_steps_without_a_host_sync(monkeypatch) -> None:
    params, opt = _make("all-fp32", F32, amp=False)
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    twin = _optimizer([{"params": twins[:3]}, {"params": twins[3:]}],
                      "all-fp32", max_grad_norm=opt.max_grad_norm)
    scaler = torch.amp.GradScaler("cuda", init_scale=SCALE)

    def item(self):
        raise AssertionError("Tensor.item() inside GradScaler.step")

    for bad in (True, False):
        opt.zero_grad()
        scaler.scale(sum((p * p).sum() for p in params)).backward()
        if bad:
            params[3].grad[2048] = float("inf")
        scale = scaler.get_scale()
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "item", item)
            scaler.step(opt)
        scaler.update()
        assert not hasattr(opt, "grad_scale")
        if bad:  # skipped, and the scale halved
            assert scaler.get_scale() == scale / 2
            assert all(opt.state[p]["step"].item() == 0 for p in params)
            assert all(torch.equal(p, q) for p, q in zip(params, twins))
            continue
        assert scaler.get_scale() == scale
        # 1 / scale is a power of two: the step is the twin's over the
        # unscaled gradients, bit for bit.
        for p, q in zip(params, twins):
            q.grad = p.grad / scale
        twin.step()
        _assert_bitwise_equal(
            [row[:1] + row[2:] for row in _snapshot(params, opt)],
            [row[:1] + row[2:] for row in _snapshot(twins, twin)])
        assert all(opt.state[p]["step"].item() == 1 for p in params)
