# GPU (MI355X) tests of the three fused AnyPrecisionAdamW kernels
# (csrc/hip/anyprecision_adamw.hip: adamw_vec_kernel,
# anyprecision_adamw_kernel, adamw_batched_kernel) against the fp64
# reference and rounding-count bound of tests/_adamw_reference.py, at the
# dtypes, sizes, alignments and grid sizes where each kernel takes another
# path. tests/test_adamw_reference.py proves that checker on the CPU.
#
# Every operand is a view into a larger buffer whose guard elements hold
# NaN; the guards and the gradient must come back bit-identical.

import os

import pytest
import torch

from tests._adamw_reference import (
    ALL_F32,
    DTYPE_MATRIX,
    F32,
    FLAGSHIP,
    KAHAN_LAYOUTS,
    MAX_K_NEEDED,
    MAX_K_WITHIN_BOUND,
    NO_KAHAN_LAYOUTS,
    OPERANDS,
    Case,
    Scalars,
    check_step,
    layout_id,
)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    os.environ.setdefault("TDX_REQUIRE_NATIVE_INIT", "1")

# (first step from m = v = 0?, step number, weight decay)
CONFIGS = [
    (True, 1, 0.0),
    (True, 1, 0.01),
    (False, 1000, 0.0),
    (False, 1000, 0.01),
]
CONFIG_IDS = ["step1-wd0", "step1-wd0.01", "step1000-wd0", "step1000-wd0.01"]

# 128 vector groups and a 7-element tail: the vec kernel, the generic
# kernel and the i0 seam between them.
N_SEAM = 1031

# The per-tensor grid caps at 8192 blocks of 256 threads.
GRID_CAP_THREADS = 8192 * 256


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from torchdistx_amd import _kernels

    assert _kernels.available(), "torchdistx_amd._K must load on a GPU box"
    assert _kernels._K.has_anyprecision_adamw_batched()


@pytest.fixture(scope="module", autouse=True)
def _report_largest_k():
    yield
    for title, record in (("largest K needed", MAX_K_NEEDED),
                          ("largest K within the bound", MAX_K_WITHIN_BOUND)):
        for name, (k, where) in sorted(record.items()):
            print(f"\n{title}: {name} {k:.2f} ({where})", end="")
    print()


def _step_one(case, scalars):
    from torchdistx_amd import _kernels

    _kernels.anyprecision_adamw_(*case.operands(), *scalars.kernel_args())
    torch.cuda.synchronize()


def _step_batched(cases, scalars):
    """One batched launch over `cases`; scalars[t] gives tensor t's
    step_size and bias_correction2_sqrt, scalars[0] the shared ones."""
    from torchdistx_amd import _kernels

    ops = [c.operands() for c in cases]
    s0 = scalars[0]
    _kernels.anyprecision_adamw_batched_(
        [o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops],
        [o[3] for o in ops], [o[4] for o in ops],
        s0.lr, s0.beta1, s0.beta2, s0.eps, s0.weight_decay,
        [s.step_size for s in scalars],
        [s.bias_correction2_sqrt for s in scalars],
    )
    torch.cuda.synchronize()


def _run_one(n, layout, config, seed, misalign=(), grad_overrides=None):
    first, step, wd = config
    case = Case(n, layout, first, "cuda", seed, misalign=misalign,
                grad_overrides=grad_overrides)
    scalars = Scalars.for_step(step, weight_decay=wd)
    _step_one(case, scalars)
    case.check(scalars, where=f"{layout_id(layout)} n={n} step={step} "
                              f"wd={wd} misalign={misalign}")
    return case


# ---------------------------------------------------------------------------
# Per-tensor entry point
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("kahan", [False, True], ids=["plain", "kahan"])
def test_dtype_matrix(kahan, config) -> None:
    layouts = KAHAN_LAYOUTS if kahan else NO_KAHAN_LAYOUTS
    assert len(NO_KAHAN_LAYOUTS) == 81
    for i, layout in enumerate(layouts):
        _run_one(N_SEAM, layout, config, seed=100 + i)


@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize(
    "n", [1, 7, 8, 9, 255, 256, 2047, 2048, 2049, 6149])
def test_sizes(n, config) -> None:
    _run_one(n, FLAGSHIP, config, seed=200 + n)
    _run_one(n, ALL_F32, config, seed=300 + n)


@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("layout", [FLAGSHIP, ALL_F32], ids=layout_id)
def test_misaligned_operands(layout, config) -> None:
    # One element into its buffer an operand is 2 or 4 bytes off a 16-byte
    # boundary, which routes the whole tensor through the generic kernel.
    names = [k for k, d in zip(OPERANDS, layout) if d is not None]
    for i, name in enumerate(names):
        case = _run_one(N_SEAM, layout, config, seed=400 + i,
                        misalign=(name,))
        assert case.views[name].data_ptr() % 16 != 0
        others = [k for k in names if k != name]
        assert all(case.views[k].data_ptr() % 16 == 0 for k in others)
    _run_one(N_SEAM, layout, config, seed=410, misalign=tuple(names))


@pytest.mark.parametrize(
    "layout,config",
    [(FLAGSHIP, CONFIGS[3]), (ALL_F32, CONFIGS[0])],
    ids=["flagship-kahan", "f32-plain"],
)
def test_vec_grid_stride_wraps(layout, config) -> None:
    # More vector groups than the capped grid has threads, plus a tail.
    # At this size the flagship case also holds elements where g ~ -9 m
    # cancels the new momentum next to a parameter below 4e-5: formed
    # plainly in fp32 the momentum's rounding error reached the update and
    # three compensations needed K = 66.0, 49.6 and 32.4 (tests/
    # test_adamw_reference.py::
    # test_mutant_uncompensated_momentum_fails_where_it_cancels).
    n = GRID_CAP_THREADS * 8 + 6149
    _run_one(n, layout, config, seed=500)


@pytest.mark.parametrize(
    "layout,config",
    [(FLAGSHIP, CONFIGS[1]), (ALL_F32, CONFIGS[2])],
    ids=["flagship-kahan", "f32-plain"],
)
def test_generic_grid_stride_wraps(layout, config) -> None:
    # Misaligned, so the generic kernel takes the whole tensor, which has
    # more elements than its capped grid has threads.
    n = GRID_CAP_THREADS + 6149
    _run_one(n, layout, config, seed=510, misalign=("p",))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_zero_gradient_on_first_step(wd) -> None:
    # g = 0 and m = v = 0: the update is exactly 0 (0 / eps), so without
    # Kahan p' is the correctly rounded fp32 product p * decay, stored
    # (p itself when weight_decay == 0), and the moments stay 0. With
    # Kahan, p' + c' still meets the bound (that is the compensation
    # check of Case.check).
    config = (True, 1, wd)
    scalars = Scalars.for_step(1, weight_decay=wd)
    for i, layout in enumerate(DTYPE_MATRIX):
        case = _run_one(N_SEAM, layout, config, seed=600 + i,
                        grad_overrides=[(slice(None), 0.0)])
        p0 = case.before()[0]
        p1, m1, v1, c1 = case.after()
        assert not m1.any() and not v1.any(), layout_id(layout)
        if c1 is None:
            expect = p0.double()
            if wd:
                # 24 x 24 bits: exact in fp64, then rounded once to fp32.
                expect = (expect * scalars.narrowed().decay).to(F32)
            assert torch.equal(p1, expect.to(p1.dtype)), layout_id(layout)


@pytest.mark.parametrize("config", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("layout", [FLAGSHIP, ALL_F32], ids=layout_id)
def test_non_finite_gradients_stay_in_their_elements(layout, config) -> None:
    # Two different vector groups and the tail.
    bad = {3: float("inf"), 517: float("-inf"), 1027: float("nan")}
    case = _run_one(N_SEAM, layout, config, seed=700,
                    grad_overrides=list(bad.items()))
    p1, m1, v1, c1 = case.after()
    for i in bad:
        assert p1[i].isnan()
    assert m1[3] == float("inf") and m1[517] == float("-inf")
    assert m1[1027].isnan()
    # Every other element is bit for bit what a run without them gives.
    clean = _run_one(N_SEAM, layout, config, seed=700,
                     grad_overrides=[(i, 0.0) for i in bad])
    keep = torch.ones(N_SEAM, dtype=torch.bool, device="cuda")
    keep[list(bad)] = False
    for got, want in zip(case.after(), clean.after()):
        if got is not None:
            assert torch.equal(got[keep], want[keep])


def test_mismatched_compensation_is_refused() -> None:
    # The compensation buffer is written like the other three; a shorter
    # one must be refused on the host, before any launch.
    from torchdistx_amd import _kernels

    case = Case(64, FLAGSHIP, False, "cuda", 710)
    p, g, m, v, c = case.operands()
    s = Scalars.for_step(3)
    with pytest.raises(RuntimeError, match="size mismatch"):
        _kernels.anyprecision_adamw_(p, g, m, v, c[:63], *s.kernel_args())
    with pytest.raises(RuntimeError, match="equal numel"):
        _kernels.anyprecision_adamw_batched_(
            [p], [g], [m], [v], [c[:63]], s.lr, s.beta1, s.beta2, s.eps,
            s.weight_decay, [s.step_size], [s.bias_correction2_sqrt])
    torch.cuda.synchronize()
    case.assert_guards_and_grad_intact()


# ---------------------------------------------------------------------------
# Batched entry point
# ---------------------------------------------------------------------------

BATCH_SIZES = {
    "given": [3, 0, 2047, 2048, 2049, 1, 4097, 0, 65537],
    "empty-first": [0, 3, 2047, 2048, 2049, 1, 4097, 0, 65537],
    "empty-last": [3, 0, 2047, 2048, 2049, 1, 4097, 65537, 0],
}


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("order", list(BATCH_SIZES))
def test_batched_mixed_list(order, wd) -> None:
    sizes = BATCH_SIZES[order]
    cases, scalars = [], []
    for t, n in enumerate(sizes):
        # Layouts rotate over the Kahan ones of the dtype matrix; every
        # other tensor drops its compensation buffer.
        layout = KAHAN_LAYOUTS[(5 * t + 1) % len(KAHAN_LAYOUTS)]
        if t % 2 == 1:
            layout = layout[:4] + (None,)
        # Misaligned views: two non-empty tensors in every order, among
        # them the largest.
        misalign = {2: ("p",), 7: ("g", "v"), 8: ("m",)}.get(t, ())
        step = t + 1  # a distinct step_size / bias_correction2 each
        cases.append(Case(n, layout, step == 1, "cuda", 800 + t,
                          misalign=misalign))
        scalars.append(Scalars.for_step(step, weight_decay=wd))
    assert len({s.step_size for s in scalars}) == len(sizes)
    assert any(c.views["c"] is None and c.n for c in cases)
    assert any(c.views["c"] is not None and c.n for c in cases)
    _step_batched(cases, scalars)
    for t, (case, s) in enumerate(zip(cases, scalars)):
        case.check(s, where=f"{order} tensor {t} n={case.n} "
                            f"{layout_id(case.layout)}")


def test_batched_all_empty_list() -> None:
    from torchdistx_amd import _kernels

    s = Scalars.for_step(1, weight_decay=0.01)
    # Empty views into live buffers, and fresh empty tensors (null device
    # pointers).
    views = [Case(0, FLAGSHIP, True, "cuda", 900 + t) for t in range(2)]
    _step_batched(views, [s, s])
    for case in views:
        case.assert_guards_and_grad_intact()

    def empty(dtype):
        return torch.empty(0, device="cuda", dtype=dtype)

    fresh = [[empty(d) for _ in range(2)] for d in FLAGSHIP]
    _kernels.anyprecision_adamw_batched_(
        *fresh, s.lr, s.beta1, s.beta2, s.eps, s.weight_decay,
        [s.step_size] * 2, [s.bias_correction2_sqrt] * 2)
    _kernels.anyprecision_adamw_(*(col[0] for col in fresh),
                                 *s.kernel_args())
    torch.cuda.synchronize()


def test_batched_virtual_block_wrap() -> None:
    # 36 x 489 = 17604 virtual blocks of 2048 elements against the 16384
    # grid cap: the first 1220 real blocks take a second virtual block, in
    # another tensor.
    n, count = 1_000_000, 36
    assert count * -(-n // 2048) == 17604 > 16384
    s = Scalars.for_step(1000, weight_decay=0.01)
    cases = [Case(n, FLAGSHIP, False, "cuda", 1000 + t)
             for t in range(count)]
    _step_batched(cases, [s] * count)
    for t, case in enumerate(cases):
        case.check(s, where=f"tensor {t}")


# ---------------------------------------------------------------------------
# Optimizer level
# ---------------------------------------------------------------------------


def _values(n, seed, first_step=True):
    return Case(n, FLAGSHIP, first_step, "cuda", seed).views


def test_optimizer_routing_at_batch_threshold() -> None:
    # One tensor below _BATCH_MAX_NUMEL (batched kernel) and one at it
    # (per-tensor kernel), flagship dtypes, Kahan on, two steps; the
    # reference gets the optimizer's own state before each step.
    from torchdistx_amd.optimizers import AnyPrecisionAdamW
    from torchdistx_amd.optimizers.anyprecision_optimizer import (
        _BATCH_MAX_NUMEL,
    )

    sizes = [_BATCH_MAX_NUMEL - 1, _BATCH_MAX_NUMEL]
    params = [
        torch.nn.Parameter(_values(n, 1100 + i)["p"].clone())
        for i, n in enumerate(sizes)
    ]
    wd = 0.01
    opt = AnyPrecisionAdamW(
        params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd,
        use_kahan_summation=True, momentum_dtype=torch.float32,
        variance_dtype=torch.bfloat16,
        compensation_buffer_dtype=torch.bfloat16, use_fused=True,
    )
    for step in (1, 2):
        before = []
        for i, p in enumerate(params):
            p.grad = _values(p.numel(), 1110 + 10 * step + i)["g"].clone()
            state = opt.state[p]
            if step == 1:
                assert not state
                zeros = [torch.zeros_like(p, dtype=d) for d in FLAGSHIP[2:]]
            else:
                zeros = [state[k].clone() for k in
                         ("exp_avg", "exp_avg_sq", "compensation")]
            before.append((p.detach().clone(), p.grad.clone(), *zeros))
        opt.step()
        torch.cuda.synchronize()
        s = Scalars.for_step(step, weight_decay=wd)
        for i, p in enumerate(params):
            state = opt.state[p]
            assert state["step"].item() == step
            assert torch.equal(p.grad, before[i][1])
            check_step(
                before[i],
                (p.detach(), state["exp_avg"], state["exp_avg_sq"],
                 state["compensation"]),
                s, where=f"optimizer step {step} n={p.numel()}")
    assert opt._fused_steps == 4


def _ordered(t):
    """fp32 bit patterns as integers ordered like the values."""
    b = t.view(torch.int32).to(torch.int64)
    return torch.where(b < 0, -(b & 0x7FFFFFFF), b)


def first_step_ulps_fused_vs_eager(n=4099):
    """Largest fp32 ulp distance of exp_avg and exp_avg_sq between the
    fused and the eager optimizer after one step from fresh state."""
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    vals = Case(n, ALL_F32, True, "cuda", 1200).views
    out = []
    for fused in (True, False):
        p = torch.nn.Parameter(vals["p"].clone())
        p.grad = vals["g"].clone()
        opt = AnyPrecisionAdamW(
            [p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01,
            momentum_dtype=torch.float32, variance_dtype=torch.float32,
            use_fused=fused,
        )
        opt.step()
        torch.cuda.synchronize()
        assert opt._fused_steps == (1 if fused else 0)
        out.append(opt.state[p])
    return tuple(
        int((_ordered(out[0][k]) - _ordered(out[1][k])).abs().max())
        for k in ("exp_avg", "exp_avg_sq"))


def test_first_step_moments_match_eager() -> None:
    # From m = v = 0 each side forms exp_avg with one rounding and
    # exp_avg_sq with two, so they agree within 4 fp32 ulps. With
    # 1.0f - beta2 formed on the device exp_avg_sq was 111 ulps off.
    ulps_m, ulps_v = first_step_ulps_fused_vs_eager()
    print(f"\nfused vs eager, first step: exp_avg {ulps_m} ulps, "
          f"exp_avg_sq {ulps_v} ulps")
    assert ulps_m <= 4
    assert ulps_v <= 4


def test_kahan_bf16_tracks_fp32_updates_fused() -> None:
    # tests/test_anyprecision_optimizer.py::
    # test_kahan_bf16_tracks_fp32_updates on the fused path: same step
    # count, same criterion.
    from torchdistx_amd.optimizers import AnyPrecisionAdamW

    steps = 1000
    p_kahan = torch.nn.Parameter(
        torch.ones(64, dtype=torch.bfloat16, device="cuda"))
    p_plain = torch.nn.Parameter(
        torch.ones(64, dtype=torch.bfloat16, device="cuda"))

    def run(param, use_kahan):
        opt = AnyPrecisionAdamW(
            [param],
            lr=1e-5,
            weight_decay=0.0,
            use_kahan_summation=use_kahan,
            momentum_dtype=torch.float32,
            variance_dtype=torch.float32,
            compensation_buffer_dtype=torch.bfloat16,
            use_fused=True,
        )
        for _ in range(steps):
            param.grad = torch.full_like(param, 1.0)
            opt.step()
        assert opt._fused_steps == steps

    run(p_kahan, True)
    run(p_plain, False)
    torch.cuda.synchronize()

    expected_drop = 1e-5 * steps
    kahan_drop = (1.0 - p_kahan.detach().to(torch.float64)).mean().item()
    plain_drop = (1.0 - p_plain.detach().to(torch.float64)).mean().item()

    assert kahan_drop > 0.7 * expected_drop
    assert plain_drop < 0.3 * expected_drop
