# Fused init chains (an RNG value step plus a fusable pointwise-scalar
# tail in one op): plan extraction, the CPU reference op, and the slice
# path — everything that can be checked without a GPU. The unfused replay
# is the oracle throughout.

import math
import os
import subprocess
import sys

import pytest
import torch

from torchdistx_amd import _C, deferred_init

DTYPES = [torch.float32, torch.bfloat16, torch.float16]

# TailOp codes (csrc/core/deferred_init.h).
ERFINV, MUL, ADD, SUB, CLAMP, CLAMP_MIN, CLAMP_MAX, NEG, ABS = range(9)


@pytest.fixture(autouse=True)
def _restore_switches():
    fused = _C.fused_init_chains_enabled()
    explicit = _C.fused_init_chains_explicit()
    native_cpu = _C.native_init_cpu_enabled()
    env = os.environ.get("TDX_FUSED_INIT_CHAINS")
    yield
    if explicit or not fused:
        _C.set_fused_init_chains(fused)
    else:
        _C.reset_fused_init_chains()
    _C.set_native_init_cpu(native_cpu)
    if env is None:
        os.environ.pop("TDX_FUSED_INIT_CHAINS", None)
    else:
        os.environ["TDX_FUSED_INIT_CHAINS"] = env


def _module(**builders):
    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for name, fn in builders.items():
                setattr(self, name, torch.nn.Parameter(fn()))

    return deferred_init(M)


def _trunc(shape=(16, 24), dtype=torch.float32):
    w = torch.empty(shape, dtype=dtype)
    torch.nn.init.trunc_normal_(w, mean=0.1, std=0.7, a=-1.0, b=1.5)
    return w


def test_chain_plan_extraction() -> None:
    # Explicitly on: the float32 erfinv_ step fuses only then (see
    # test_f32_erfinv_needs_the_explicit_switch).
    _C.set_fused_init_chains(True)
    torch.manual_seed(11)
    gen = torch.Generator().manual_seed(3)

    def nine_steps():
        t = torch.empty(8).uniform_()
        for _ in range(9):
            t.neg_()
        return t

    m = _module(
        w=_trunc,
        div=lambda: torch.empty(8).uniform_().div_(2.0),
        alpha=lambda: torch.empty(8).uniform_().add_(1.0, alpha=2),
        sqrt=lambda: torch.empty(8).uniform_().sqrt_(),
        nine=nine_steps,
        gen=lambda: torch.empty(8).uniform_(generator=gen).mul_(2.0),
        n=lambda: torch.empty(8).normal_().mul_(3),
        dead=lambda: torch.empty(8).uniform_().mul_(2).normal_(),
        fill=lambda: torch.empty(8).fill_(2.0).mul_(2.0),
        plain=lambda: torch.empty(8).uniform_(-1, 1),
        sub=lambda: torch.empty(8).uniform_().sub_(0.5).abs_().clamp_(max=0.4),
    )

    plan = _C.tensor_chain_plan(m.w)
    assert plan is not None
    assert plan["kind"] == "uniform"
    # trunc_normal_'s own arithmetic for the uniform bounds.
    lo = (1.0 + math.erf((-1.0 - 0.1) / 0.7 / math.sqrt(2.0))) / 2.0
    hi = (1.0 + math.erf((1.5 - 0.1) / 0.7 / math.sqrt(2.0))) / 2.0
    assert plan["p0"] == 2 * lo - 1 and plan["p1"] == 2 * hi - 1
    assert plan["sizes"] == [16, 24] and plan["dtype"] == torch.float32
    assert plan["tail"] == [
        ("erfinv", 0.0, 0.0),
        ("mul", 0.7 * math.sqrt(2.0), 0.0),
        ("add", 0.1, 0.0),
        ("clamp", -1.0, 1.5),
    ]
    # Pinned Philox state: the one the tape carries for the uniform_ step,
    # which the tail-free planner reports for a plain uniform_ tensor.
    plain = _C.tensor_chain_plan(m.plain)
    assert plain == {**_C.tensor_init_plan(m.plain), "tail": []}
    assert plan["seed"] == plain["seed"]
    assert plan["offset"] > 0 and plan["offset"] != plain["offset"]

    for name in ("div", "alpha", "sqrt", "nine", "gen", "fill"):
        assert _C.tensor_chain_plan(getattr(m, name)) is None, name

    n = _C.tensor_chain_plan(m.n)
    assert n["kind"] == "normal" and n["tail"] == [("mul", 3.0, 0.0)]
    dead = _C.tensor_chain_plan(m.dead)
    assert dead["kind"] == "normal" and dead["tail"] == []
    assert dead["p0"] == 0.0 and dead["p1"] == 1.0
    sub = _C.tensor_chain_plan(m.sub)
    assert sub["tail"] == [
        ("sub", 0.5, 0.0), ("abs", 0.0, 0.0), ("clamp_max", 0.4, 0.0),
    ]

    # The tail-free planner keeps refusing tails.
    assert _C.tensor_init_plan(m.w) is None
    assert _C.tensor_init_plan(m.dead) is None

    _C.set_fused_init_chains(False)
    assert not _C.fused_init_chains_enabled()
    for name in ("w", "n", "sub", "dead"):
        assert _C.tensor_chain_plan(getattr(m, name)) is None, name
    assert _C.tensor_chain_plan(m.plain) == plain
    _C.set_fused_init_chains(True)
    assert _C.tensor_chain_plan(m.w) == plan


def test_f32_erfinv_needs_the_explicit_switch() -> None:
    # On the GPU, erfinv_ on a float32 tensor is 1-2 ulp away from ATen's
    # kernel. By default only what is bitwise equal fuses — bf16/fp16
    # trunc_normal_ chains and every other tail; float32 erfinv_ needs the
    # explicit opt-in.
    _C.reset_fused_init_chains()
    assert _C.fused_init_chains_enabled()
    assert not _C.fused_init_chains_explicit()
    torch.manual_seed(13)
    m = _module(
        f32=_trunc,
        bf16=lambda: _trunc(dtype=torch.bfloat16),
        f16=lambda: _trunc(dtype=torch.float16),
        exact=lambda: torch.empty(8).uniform_().mul_(2.0).add_(1.0),
    )
    assert _C.tensor_chain_plan(m.f32) is None
    for name in ("bf16", "f16"):
        tail = _C.tensor_chain_plan(getattr(m, name))["tail"]
        assert [t[0] for t in tail] == ["erfinv", "mul", "add", "clamp"]
    assert len(_C.tensor_chain_plan(m.exact)["tail"]) == 2
    _C.set_fused_init_chains(True)
    assert _C.fused_init_chains_explicit()
    assert len(_C.tensor_chain_plan(m.f32)["tail"]) == 4
    _C.set_fused_init_chains(False)
    assert not _C.fused_init_chains_explicit()
    assert _C.tensor_chain_plan(m.bf16) is None


def test_tensor_operand_must_be_a_wrapped_number() -> None:
    # A real 0-dim tensor operand promotes differently from a python
    # scalar; only the latter is an immediate.
    torch.manual_seed(12)
    scale = torch.tensor(2.0)
    m = _module(
        t=lambda: torch.empty(8).uniform_().mul_(scale),
        s=lambda: torch.empty(8).uniform_().mul_(2.0),
    )
    assert _C.tensor_chain_plan(m.t) is None
    assert _C.tensor_chain_plan(m.s)["tail"] == [("mul", 2.0, 0.0)]


def test_env_switch_starts_off() -> None:
    env = dict(os.environ, TDX_FUSED_INIT_CHAINS="0")
    out = subprocess.run(
        [sys.executable, "-c",
         "from torchdistx_amd import _C;"
         "print(_C.fused_init_chains_enabled())"],
        env=env, capture_output=True, text=True, check=True,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
    )
    assert out.stdout.strip() == "False"


TRUNC_TAIL = (
    [ERFINV, MUL, ADD, CLAMP],
    [0.0, 0.7 * math.sqrt(2.0), 0.1, -1.0],
    [0.0, 0.0, 0.0, 1.5],
)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("numel", [1, 7, 8, 9, 4099])
def test_cpu_op_matches_unfused(dtype, numel) -> None:
    seed, offset = 1234567, 8
    ref = torch.empty(numel, dtype=dtype)
    torch.ops.tdx.uniform_(ref, -0.9, 0.95, seed=seed, offset=offset)
    ref.erfinv_().mul_(0.7 * math.sqrt(2.0)).add_(0.1).clamp_(-1.0, 1.5)
    out = torch.empty(numel, dtype=dtype)
    ops, s0, s1 = TRUNC_TAIL
    torch.ops.tdx.rng_chain_(out, 0, -0.9, 0.95, ops, s0, s1,
                             seed=seed, offset=offset)
    assert not ref.isnan().any()
    assert torch.equal(out, ref)

    # Exact-op tail on a normal start, one-sided clamps included.
    ref = torch.empty(numel, dtype=dtype)
    torch.ops.tdx.normal_(ref, 0.2, 1.5, seed=seed, offset=offset)
    ref.sub_(0.25).neg_().abs_().clamp_min_(0.5).clamp_max_(2.0)
    out = torch.empty(numel, dtype=dtype)
    torch.ops.tdx.rng_chain_(
        out, 1, 0.2, 1.5, [SUB, NEG, ABS, CLAMP_MIN, CLAMP_MAX],
        [0.25, 0.0, 0.0, 0.5, 2.0], [0.0] * 5, seed=seed, offset=offset)
    assert torch.equal(out, ref)


def test_cpu_op_rejects_bad_programs() -> None:
    t = torch.empty(8)
    with pytest.raises(RuntimeError):
        torch.ops.tdx.rng_chain_(t, 0, 0.0, 1.0, [NEG] * 9, [0.0] * 9,
                                 [0.0] * 9, seed=1, offset=4)
    with pytest.raises(RuntimeError):
        torch.ops.tdx.rng_chain_(t, 0, 0.0, 1.0, [99], [0.0], [0.0],
                                 seed=1, offset=4)
    with pytest.raises(RuntimeError):
        torch.ops.tdx.rng_chain_(t, 3, 0.0, 1.0, [], [], [], seed=1, offset=4)


def _slice_ranges(n):
    # empty, full, first row, last row, and an interior range
    ranges = {(0, 0), (n, n), (0, n), (0, 1), (n - 1, n)}
    if n > 3:
        ranges.add((1, n - 1))
    return sorted(ranges)


@pytest.mark.parametrize("shape", [(16, 24), (33, 9), (5, 3, 17)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_slices_match_unfused_and_full(shape, dtype) -> None:
    _C.set_native_init_cpu(True)
    _C.set_fused_init_chains(True)  # explicit: covers float32 erfinv too
    torch.manual_seed(21)
    m = _module(w=lambda: _trunc(shape, dtype))
    assert _C.tensor_chain_plan(m.w)["tail"]

    cases = [
        (dim, lo, hi)
        for dim in range(len(shape))
        for lo, hi in _slice_ranges(shape[dim])
    ]
    fused = {}
    for dim, lo, hi in cases:
        fused[dim, lo, hi] = _C.materialize_tensor_shard(m.w, lo, hi, dim)
    _C.set_fused_init_chains(False)
    unfused = {}
    for dim, lo, hi in cases:
        unfused[dim, lo, hi] = _C.materialize_tensor_shard(m.w, lo, hi, dim)
    full = _C.materialize_tensor(m.w).detach()
    assert full.dtype == dtype and not full.isnan().any()
    for dim, lo, hi in cases:
        want = full.narrow(dim, lo, hi - lo)
        assert torch.equal(unfused[dim, lo, hi], want), (dim, lo, hi)
        assert torch.equal(fused[dim, lo, hi], want), (dim, lo, hi)


def test_slice_path_launches_the_fused_op() -> None:
    # The collapse must actually happen: one tdx::rng_chain_shard_win_
    # call instead of the uniform shard op plus four ATen ops.
    from torch.utils._python_dispatch import TorchDispatchMode

    class Trace(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.names.append(func.name())
            return func(*args, **(kwargs or {}))

    _C.set_native_init_cpu(True)
    _C.set_fused_init_chains(True)
    torch.manual_seed(22)
    m = _module(w=_trunc, d=lambda: torch.empty(16, 24).uniform_().div_(2.0))

    def traced(t):
        with Trace() as tr:
            _C.materialize_tensor_shard(t, 2, 5, 1)
        return [n for n in tr.names if not n.startswith("aten::empty")]

    assert traced(m.w) == ["tdx::rng_chain_shard_win_"]
    # div_ is outside the fusable set: step by step, as before.
    assert traced(m.d) == ["tdx::uniform_shard_win_", "aten::div_.Tensor"]
    _C.set_fused_init_chains(False)
    assert traced(m.w)[0] == "tdx::uniform_shard_win_"
    assert len(traced(m.w)) == 5
