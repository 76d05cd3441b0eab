# Init chains that end in a dtype conversion (`Model(cfg).to(bf16)` inside
# the builder, `Parameter(empty(..).normal_().to(bf16))`): the chain model,
# the planner, slice/block materialization and the CPU reference ops —
# everything that can be checked without a GPU. The oracle throughout is
# the ordinary node-by-node replay of the same tape (materialize_tensor):
# plans, slices and blocks must equal it bit for bit.

import itertools
import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from torchdistx_amd import _C, deferred_init
from torchdistx_amd.deferred_init import materialize_module
from torchdistx_amd.models import TINY, build_model
from torchdistx_amd.parallel import (
    materialize_tensor_block,
    materialize_tensor_shard,
)

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FP8 = torch.float8_e4m3fn
PAIRS = [(s, d) for s in (F32, BF16, F16) for d in (F32, BF16, F16) if s != d]
SHAPES = [(16, 24), (33, 9), (5, 3, 17)]

# TailOp codes (csrc/core/deferred_init.h).
ERFINV, MUL, ADD, SUB, CLAMP, CLAMP_MIN, CLAMP_MAX, NEG, ABS = range(9)

SEED, OFFSET = 987654321, 12


@pytest.fixture(autouse=True)
def _restore_switches():
    fused = _C.fused_init_chains_enabled()
    explicit = _C.fused_init_chains_explicit()
    native_cpu = _C.native_init_cpu_enabled()
    env = os.environ.get("TDX_FUSED_INIT_CHAINS")
    _C.set_native_init_cpu(True)
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
                t = fn()
                grad = t.dtype != FP8
                setattr(self, name, torch.nn.Parameter(t, requires_grad=grad))

    return deferred_init(M)


def _trunc(shape, dtype):
    w = torch.empty(shape, dtype=dtype)
    # 2 * cdf - 1 stays within about (-0.88, 0.96): erfinv_ is finite.
    torch.nn.init.trunc_normal_(w, mean=0.1, std=0.7, a=-1.0, b=1.5)
    return w


INITS = {
    "normal": lambda s, d: torch.empty(s, dtype=d).normal_(0.1, 0.8),
    "uniform": lambda s, d: torch.empty(s, dtype=d).uniform_(-0.5, 1.5),
    "bernoulli": lambda s, d: torch.empty(s, dtype=d).bernoulli_(0.3),
    "fill": lambda s, d: torch.empty(s, dtype=d).fill_(0.37),
    "trunc": _trunc,
}


def _boxes(shape):
    """The box set of tests/test_block_slice.py: every dim partial, the
    middle dim full, empty on one dim, the whole tensor, a single row and
    a single column. `partial`, `empty`, `row` and `col` of a 3-d shape
    are boxes of two levels."""
    r = len(shape)
    partial = [(1, n - 1) if n > 2 else (n - 1, n) for n in shape]
    whole = [(0, n) for n in shape]
    mid_full = list(partial)
    mid_full[r // 2 if r > 2 else r - 1] = whole[r // 2 if r > 2 else r - 1]
    empty = list(partial)
    empty[r - 2] = (2, 2)
    row = list(partial)
    row[0] = (shape[0] - 1, shape[0])
    col = list(partial)
    col[-1] = (3, 4)
    return {"partial": partial, "mid_full": mid_full, "empty": empty,
            "whole": whole, "row": row, "col": col}


def _index(box):
    return tuple(slice(lo, hi) for lo, hi in box)


def _block(t, box):
    return _C.materialize_tensor_block(
        t, [lo for lo, _ in box], [hi for _, hi in box]
    )


def _ranges(n):
    return sorted({(0, n), (0, 1), (n - 1, n), (1, n - 1), (n // 2, n)})


def _bits(t):
    """torch.equal is not implemented for fp8: compare the bytes."""
    return t.view(torch.uint8) if t.dtype == FP8 else t


def _check_slices(t, shape, label):
    """Every shard (both switch states) and block of `t` against the full
    replay, which runs last on the very same tape."""
    boxes = _boxes(shape)
    shards, blocks = {}, {}
    for fused in (True, False):
        # Explicitly on covers the float32 erfinv_ step too.
        _C.set_fused_init_chains(fused)
        for dim, n in enumerate(shape):
            for lo, hi in _ranges(n):
                shards[fused, dim, lo, hi] = _C.materialize_tensor_shard(
                    t, lo, hi, dim)
        for name, box in boxes.items():
            blocks[fused, name] = _block(t, box)
    full = _C.materialize_tensor(t).detach()
    assert not full.float().isnan().any()
    for (fused, dim, lo, hi), shard in shards.items():
        want = full.narrow(dim, lo, hi - lo)
        assert shard.dtype == full.dtype and shard.shape == want.shape
        assert shard.is_contiguous()
        assert torch.equal(_bits(shard), _bits(want)), (
            label, fused, dim, lo, hi)
    for (fused, name), block in blocks.items():
        want = full[_index(boxes[name])]
        assert block.dtype == full.dtype and block.shape == want.shape
        assert torch.equal(_bits(block), _bits(want)), (
            label, fused, name, boxes[name])
    return full


# ---- plans ------------------------------------------------------------------


def _lin(convert):
    torch.manual_seed(7)
    return deferred_init(lambda: convert(torch.nn.Linear(16, 8)))


@pytest.mark.parametrize(
    "convert, dst",
    [
        (lambda m: m.to(BF16), BF16),
        (lambda m: m.bfloat16(), BF16),
        (lambda m: m.half(), F16),
    ],
    ids=["to", "bfloat16", "half"],
)
def test_module_conversion_in_the_builder_plans(convert, dst) -> None:
    plain = _lin(lambda m: m)
    cast = _lin(convert)
    for name in ("weight", "bias"):
        want = _C.tensor_chain_plan(getattr(plain, name))
        got = _C.tensor_chain_plan(getattr(cast, name))
        assert want is not None and want["src_dtype"] is None
        assert want["kind"] == "uniform" and want["dtype"] == F32
        assert got is not None, name
        assert got["kind"] == "uniform"
        assert got["dtype"] == dst and got["src_dtype"] == F32
        assert getattr(cast, name).dtype == dst
        for key in ("p0", "p1", "seed", "offset", "sizes", "tail"):
            assert got[key] == want[key], (name, key)
        assert _C.tensor_init_plan(getattr(cast, name)) == {
            k: v for k, v in got.items() if k != "tail"}


def test_parameter_converted_before_wrapping_plans() -> None:
    torch.manual_seed(8)
    m = _module(
        w=lambda: torch.empty(12, 6).normal_(0.0, 0.02).to(BF16),
        ref=lambda: torch.empty(12, 6).normal_(0.0, 0.02),
    )
    plan = _C.tensor_chain_plan(m.w)
    ref = _C.tensor_chain_plan(m.ref)
    assert plan["kind"] == "normal" and (plan["p0"], plan["p1"]) == (0.0, 0.02)
    assert plan["dtype"] == BF16 and plan["src_dtype"] == F32
    assert plan["seed"] == ref["seed"]
    assert plan["offset"] > 0 and plan["offset"] != ref["offset"]
    assert ref.get("src_dtype") is None


def test_constant_heads_plan_as_plain_fills() -> None:
    m = _module(
        a=lambda: torch.empty(4, 4).fill_(0.37).to(BF16),
        b=lambda: torch.empty(4, 4, dtype=F16).fill_(1.0 / 3.0).to(BF16),
        z=lambda: torch.zeros(4, 4).to(F16),
        o=lambda: torch.ones(4, 4, dtype=BF16).to(F32),
    )
    a = _C.tensor_chain_plan(m.a)
    assert a["kind"] == "fill" and a["dtype"] == BF16
    assert a["src_dtype"] is None
    assert a["p0"] == float(torch.tensor(0.37, dtype=F32))
    b = _C.tensor_chain_plan(m.b)
    assert b["kind"] == "fill" and b["dtype"] == BF16
    third = torch.tensor(1.0 / 3.0, dtype=F32).to(F16)  # double->float->f16
    assert b["p0"] == float(third)
    # Rounding 1/3 straight to bf16 differs from going through f16 first.
    assert torch.tensor(b["p0"]).to(BF16) == third.to(BF16)
    z = _C.tensor_chain_plan(m.z)
    assert z["kind"] == "zero" and z["dtype"] == F16 and z["src_dtype"] is None
    o = _C.tensor_chain_plan(m.o)
    assert o["kind"] == "fill" and o["p0"] == 1.0 and o["dtype"] == F32
    for name in ("a", "b", "z", "o"):
        t = getattr(m, name)
        plan = _C.tensor_chain_plan(t)
        full = _C.materialize_tensor(t).detach()
        want = torch.zeros(4, 4, dtype=plan["dtype"])
        if plan["kind"] == "fill":
            want.fill_(plan["p0"])
        assert torch.equal(full, want), name


def test_same_dtype_to_plans_as_if_absent() -> None:
    torch.manual_seed(9)
    m = _module(
        w=lambda: torch.empty(6, 5).uniform_(-1.0, 2.0).to(F32),
        c=lambda: torch.empty(6, 5).uniform_(-1.0, 2.0).to(F32, copy=True),
        ref=lambda: torch.empty(6, 5).uniform_(-1.0, 2.0),
    )
    ref = _C.tensor_chain_plan(m.ref)
    for name in ("w", "c"):
        plan = _C.tensor_chain_plan(getattr(m, name))
        assert plan is not None and plan["src_dtype"] is None, name
        assert plan["dtype"] == F32
        for key in ("kind", "p0", "p1", "seed", "sizes", "tail"):
            assert plan[key] == ref[key]
        _check_slices(getattr(m, name), (6, 5), name)


def test_what_stays_unplannable() -> None:
    torch.manual_seed(10)
    m = _module(
        two=lambda: torch.empty(8, 4).uniform_().to(BF16).to(F32),
        after=lambda: torch.empty(8, 4).uniform_().to(BF16).mul_(2.0),
        refill=lambda: torch.empty(8, 4).uniform_().to(BF16).normal_(),
        f8=lambda: torch.empty(8, 4).uniform_().to(FP8),
        f64=lambda: torch.empty(8, 4, dtype=torch.float64).uniform_().to(F32),
        tail=lambda: torch.empty(8, 4).uniform_(-0.9, 0.95).erfinv_().to(BF16),
        tail16=lambda: torch.empty(8, 4, dtype=F16).uniform_(-0.9, 0.95)
        .erfinv_().to(BF16),
    )
    for name in ("two", "after", "refill", "f8", "f64"):
        assert _C.tensor_chain_plan(getattr(m, name)) is None, name
        assert _C.tensor_init_plan(getattr(m, name)) is None, name
    # The tail rules hold at the SOURCE dtype: float32 erfinv_ needs the
    # explicit switch, float16 erfinv_ does not.
    _C.reset_fused_init_chains()
    if not _C.fused_init_chains_explicit():
        assert _C.tensor_chain_plan(m.tail) is None
    plan16 = _C.tensor_chain_plan(m.tail16)
    if _C.fused_init_chains_enabled():
        assert plan16["tail"] == [("erfinv", 0.0, 0.0)]
        assert plan16["src_dtype"] == F16 and plan16["dtype"] == BF16
    _C.set_fused_init_chains(True)
    plan = _C.tensor_chain_plan(m.tail)
    assert plan["tail"] == [("erfinv", 0.0, 0.0)]
    assert plan["src_dtype"] == F32 and plan["dtype"] == BF16
    assert _C.tensor_init_plan(m.tail) is None


def test_other_kinds_of_to_are_not_simple_chains() -> None:
    torch.manual_seed(11)
    shape = (2, 3, 4, 5)
    m = _module(
        cl=lambda: torch.empty(shape).uniform_().to(
            BF16, memory_format=torch.channels_last),
        src_cl=lambda: torch.empty(shape)
        .to(memory_format=torch.channels_last).uniform_()
        .to(BF16, memory_format=torch.contiguous_format),
        ok=lambda: torch.empty(shape).uniform_().to(
            BF16, memory_format=torch.contiguous_format),
        like=lambda: torch.empty(shape).uniform_().to(
            torch.empty(1, dtype=F16)),
    )
    for name in ("cl", "src_cl"):
        t = getattr(m, name)
        assert _C.tensor_chain_plan(t) is None, name
        if t.is_contiguous():
            with pytest.raises(RuntimeError, match="slice materialization"):
                _C.materialize_tensor_shard(t, 0, 1, 0)
            shard = materialize_tensor_shard(t, 0, 1, 0)
            full = _C.materialize_tensor(t).detach()
            assert torch.equal(shard.detach(), full[0:1]), name
    assert _C.tensor_chain_plan(m.ok)["src_dtype"] == F32
    # to.other with a real tensor only lends its dtype.
    like = _C.tensor_chain_plan(m.like)
    assert like["dtype"] == F16 and like["src_dtype"] == F32
    _check_slices(m.ok, shape, "ok")
    _check_slices(m.like, shape, "like")


def test_module_to_on_an_already_converted_parameter() -> None:
    # Module.to(bf16) over a bf16 parameter records a no-op `to` and
    # `p.data = p`: still the tensor's own lineage, and no conversion.
    torch.manual_seed(12)
    m = deferred_init(
        lambda: torch.nn.Linear(24, 16, dtype=BF16).to(BF16))
    plan = _C.tensor_chain_plan(m.weight)
    assert plan["kind"] == "uniform" and plan["src_dtype"] is None
    assert plan["dtype"] == BF16
    _check_slices(m.weight, (16, 24), "noop")


# ---- slices -----------------------------------------------------------------


@pytest.mark.parametrize("init", sorted(INITS))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("shape", SHAPES)
def test_slices_and_blocks_match_the_full_replay(shape, pair, init) -> None:
    src, dst = pair
    torch.manual_seed(31)
    m = _module(w=lambda: INITS[init](shape, src).to(dst))
    full = _check_slices(m.w, shape, (init, src, dst))
    assert full.dtype == dst


@pytest.mark.parametrize("init", ["normal", "uniform", "fill", "trunc"])
@pytest.mark.parametrize("src", [F32, BF16])
def test_fp8_destination_takes_the_step_by_step_path(src, init) -> None:
    shape = (33, 9)
    torch.manual_seed(33)
    m = _module(w=lambda: INITS[init](shape, src).to(FP8))
    assert _C.tensor_chain_plan(m.w) is None or init == "fill"
    full = _check_slices(m.w, shape, (init, src))
    assert full.dtype == FP8


def test_module_to_slices_match() -> None:
    torch.manual_seed(34)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(24, 16)
            self.emb = torch.nn.Embedding(33, 9)
            self.register_buffer("scale", torch.ones(16, 24))

    m = deferred_init(lambda: M().half())
    assert _C.tensor_chain_plan(m.emb.weight)["kind"] == "normal"
    _check_slices(m.lin.weight, (16, 24), "lin")
    _check_slices(m.emb.weight, (33, 9), "emb")
    _check_slices(m.scale, (16, 24), "scale")


def test_casts_in_the_middle_shard_without_a_plan() -> None:
    torch.manual_seed(35)
    shape = (33, 9)
    m = _module(
        after=lambda: torch.empty(shape).normal_().to(BF16).mul_(1.7),
        two=lambda: torch.empty(shape).uniform_(-2.0, 2.0).to(BF16).to(F32),
        again=lambda: torch.empty(shape).uniform_().to(F16).normal_(0.0, 2.0),
        chain=lambda: torch.empty(shape, dtype=BF16).uniform_(-0.9, 0.95)
        .erfinv_().to(F32).mul_(0.7).add_(0.1).to(F16),
    )
    for name in ("after", "two", "chain"):
        assert _C.tensor_chain_plan(getattr(m, name)) is None, name
    for name in ("after", "two", "again", "chain"):
        full = _check_slices(getattr(m, name), shape, name)
        assert full.dtype == getattr(m, name).dtype


def test_a_conversion_of_the_tensor_is_no_part_of_the_tensor() -> None:
    # `h = p.half()` is pulled into p's replay set when p is overwritten
    # afterwards (h must read the old value first). It is not a step of p.
    torch.manual_seed(36)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.empty(16, 24).uniform_())
            self.h = torch.nn.Parameter(self.p.half())
            with torch.no_grad():
                self.p.mul_(2.0)

    m = deferred_init(M)
    plan = _C.tensor_chain_plan(m.p)
    assert plan["dtype"] == F32 and plan["src_dtype"] is None
    assert plan["tail"] == [("mul", 2.0, 0.0)]
    hplan = _C.tensor_chain_plan(m.h)
    assert hplan["dtype"] == F16 and hplan["src_dtype"] == F32
    assert hplan["tail"] == []
    h_shard = _C.materialize_tensor_shard(m.h, 3, 9, 0)
    p_shard = _C.materialize_tensor_shard(m.p, 3, 9, 1)
    h = _C.materialize_tensor(m.h).detach()
    p = _C.materialize_tensor(m.p).detach()
    assert torch.equal(h_shard, h[3:9]) and torch.equal(p_shard, p[:, 3:9])
    assert not p.isnan().any() and not h.isnan().any()
    # h holds the value p had BEFORE the mul_ (doubling is exact).
    assert torch.equal((p / 2.0).half(), h)


class _Outputs(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.numels = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        outs = out if isinstance(out, (tuple, list)) else (out,)
        for o in outs:
            if isinstance(o, torch.Tensor):
                self.numels.append((func.name(), o.numel()))
        return out


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("init", ["normal", "trunc", "fill"])
def test_no_full_size_intermediate(init, fused) -> None:
    shape = (5, 16, 24)
    numel = 5 * 16 * 24
    torch.manual_seed(37)
    m = _module(
        w=lambda: INITS[init](shape, F32).to(BF16),
        f8=lambda: INITS[init](shape, F32).to(FP8),
    )
    _C.set_fused_init_chains(fused)
    calls = [
        lambda t: _C.materialize_tensor_shard(t, 1, 4, 0),
        lambda t: _C.materialize_tensor_shard(t, 2, 15, 1),
        lambda t: _C.materialize_tensor_shard(t, 0, 23, 2),
        lambda t: _block(t, [(1, 4), (2, 9), (3, 11)]),  # two levels
    ]
    for t in (m.w, m.f8):
        for call in calls:
            with _Outputs() as rec:
                out = call(t)
            assert 0 < out.numel() < numel
            assert rec.numels, "the slice ran no op at all"
            worst = max(rec.numels, key=lambda r: r[1])
            assert worst[1] <= out.numel(), worst


# ---- lineage guard ----------------------------------------------------------


@pytest.mark.parametrize("other_first", [True, False])
@pytest.mark.parametrize("convert", [False, True])
def test_data_assigned_from_another_tensor_is_not_a_chain(
    other_first, convert
) -> None:
    shape = (33, 9)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            if other_first:
                other = torch.empty(shape).normal_(0.0, 3.0)
            self.p = torch.nn.Parameter(torch.empty(shape).uniform_())
            if not other_first:
                other = torch.empty(shape).normal_(0.0, 3.0)
            self.p.data = other.to(BF16) if convert else other

    torch.manual_seed(38)
    m = deferred_init(M)
    assert _C.tensor_chain_plan(m.p) is None
    assert _C.tensor_init_plan(m.p) is None
    with pytest.raises(RuntimeError, match="slice materialization"):
        _C.materialize_tensor_shard(m.p, 0, 4, 0)
    with pytest.raises(RuntimeError, match="slice materialization"):
        _C.materialize_tensor_block(m.p, [1, 1], [5, 5])
    shard = materialize_tensor_shard(m.p, 3, 20, 0)
    col = materialize_tensor_shard(m.p, 2, 7, 1)
    block = materialize_tensor_block(m.p, [(1, 30), (2, 8)])
    full = _C.materialize_tensor(m.p).detach()
    assert full.dtype == (BF16 if convert else F32)
    assert full.float().std() > 2.0  # the normal_(0, 3), not the uniform_
    assert torch.equal(shard.detach(), full[3:20])
    assert torch.equal(col.detach(), full[:, 2:7])
    assert torch.equal(block.detach(), full[1:30, 2:8])


def test_data_assigned_from_the_tensors_own_conversion_is_a_chain() -> None:
    shape = (16, 24)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.empty(shape).normal_())
            self.p.data = self.p.data.to(BF16)

    torch.manual_seed(39)
    m = deferred_init(M)
    plan = _C.tensor_chain_plan(m.p)
    assert plan["kind"] == "normal" and plan["src_dtype"] == F32
    _check_slices(m.p, shape, "own")


# ---- module level -----------------------------------------------------------


def _unplanned(model):
    named = list(model.named_parameters()) + list(model.named_buffers())
    return {n for n, t in named if _C.tensor_chain_plan(t) is None}


def test_tiny_model_converted_in_the_builder_plans_like_dtype_arg() -> None:
    torch.manual_seed(40)
    native = deferred_init(build_model, TINY, dtype=BF16)
    torch.manual_seed(40)
    cast = deferred_init(lambda: build_model(TINY).to(BF16))
    assert _unplanned(cast) <= _unplanned(native)
    n_cast = 0
    for name, p in cast.named_parameters():
        assert p.dtype == BF16
        plan = _C.tensor_chain_plan(p)
        if plan is not None and plan["src_dtype"] is not None:
            assert plan["src_dtype"] == F32 and plan["dtype"] == BF16
            n_cast += 1
    assert n_cast > 0
    # Every parameter shards along dim 0, equal to the full replay.
    shards = {
        n: _C.materialize_tensor_shard(p, 1, p.shape[0], 0)
        for n, p in cast.named_parameters()
    }
    for n, p in cast.named_parameters():
        full = _C.materialize_tensor(p).detach()
        assert torch.equal(shards[n], full[1:]), n


def test_tape_order_replay_still_equals_eager_construction() -> None:
    _C.set_native_init_cpu(False)
    torch.manual_seed(41)
    deferred = deferred_init(lambda: build_model(TINY).to(BF16))
    materialize_module(deferred)
    torch.manual_seed(41)
    eager = build_model(TINY).to(BF16)
    for (dn, dp), (en, ep) in zip(
        deferred.named_parameters(), eager.named_parameters()
    ):
        assert dn == en and dp.dtype == BF16
        assert torch.equal(dp, ep), dn
    for (dn, db), (en, eb) in zip(
        deferred.named_buffers(), eager.named_buffers()
    ):
        assert dn == en and torch.equal(db, eb), dn


# ---- the CPU reference ops --------------------------------------------------
# The CPU twins ARE the source-dtype op into a temporary followed by a
# conversion, so the two tests below compare an op with its own recipe:
# they pin argument order, routing, window geometry and that `copy_`
# converts like `.to()`, and are no independent check of the values. The
# independent check is on the GPU (tests/test_cast_chain_gpu.py), where
# the kernels compute the values in registers and must match this recipe.

_TAILS = {
    "none": ([], [], []),
    "mul_add": ([MUL, ADD], [1.1, -0.3], [0.0, 0.0]),
    "trunc": ([ERFINV, MUL, ADD, CLAMP], [0.0, 0.99, 0.1, -1.0],
              [0.0, 0.0, 0.0, 1.5]),
}
_DISTS = {"uniform": (0, -0.9, 0.95), "normal": (1, 0.2, 1.5),
          "bernoulli": (2, 0.3, 0.0)}


def _src_then_to(numel, src, dst, dist, p0, p1, tail):
    ref = torch.empty(numel, dtype=src)
    torch.ops.tdx.rng_chain_(ref, dist, p0, p1, *tail, seed=SEED,
                             offset=OFFSET)
    assert not ref.isnan().any()
    return ref.to(dst)


@pytest.mark.parametrize("dist", sorted(_DISTS))
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_cpu_cast_op_equals_the_source_op_then_to(pair, dist) -> None:
    src, dst = pair
    code, p0, p1 = _DISTS[dist]
    for tail_name, tail in _TAILS.items():
        if tail_name == "trunc" and dist != "uniform":
            continue
        for numel in (1, 3, 4, 5, 7, 8, 9, 13, 2053):
            want = _src_then_to(numel, src, dst, code, p0, p1, tail)
            out = torch.empty(numel, dtype=dst)
            torch.ops.tdx.rng_chain_cast_(out, src, code, p0, p1, *tail,
                                          seed=SEED, offset=OFFSET)
            assert torch.equal(out, want), (tail_name, numel)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_cpu_cast_window_op_is_a_slice_of_the_whole(pair) -> None:
    src, dst = pair
    rows, cols = 7, 48
    tail = _TAILS["mul_add"]
    whole = _src_then_to(rows * cols, src, dst, 1, 0.2, 1.5, tail)
    whole = whole.view(rows, cols)
    # g_off % 8 in {0, 4, 3}; odd and even block lengths.
    for lo, hi in [(0, 48), (8, 40), (4, 44), (4, 9), (3, 20), (16, 17)]:
        g_off = lo
        assert g_off % 8 in (0, 4, 3)
        out = torch.empty(rows, hi - lo, dtype=dst)
        torch.ops.tdx.rng_chain_cast_shard_win_(
            out, src, rows, hi - lo, cols, g_off, 1, 0.2, 1.5, *tail,
            rows * cols, seed=SEED, offset=OFFSET)
        assert torch.equal(out, whole[:, lo:hi]), (lo, hi)
    # Flat ranges (n_blocks == 1) starting inside a unit.
    flat = whole.reshape(-1)
    for start, end in [(0, 13), (4, 29), (3, 336), (8, 9), (12, 12)]:
        out = torch.empty(end - start, dtype=dst)
        torch.ops.tdx.rng_chain_cast_shard_win_(
            out, src, 1, end - start, end - start, start, 1, 0.2, 1.5,
            *tail, rows * cols, seed=SEED, offset=OFFSET)
        assert torch.equal(out, flat[start:end]), (start, end)


def test_cast_ops_reject_what_they_do_not_cover() -> None:
    out = torch.empty(8, dtype=BF16)
    with pytest.raises(RuntimeError, match="two different dtypes"):
        torch.ops.tdx.rng_chain_cast_(out, BF16, 0, 0.0, 1.0, [], [], [],
                                      seed=1, offset=4)
    with pytest.raises(RuntimeError, match="two different dtypes"):
        torch.ops.tdx.rng_chain_cast_(out, torch.float64, 0, 0.0, 1.0, [],
                                      [], [], seed=1, offset=4)
    with pytest.raises(RuntimeError, match="shard numel"):
        torch.ops.tdx.rng_chain_cast_shard_win_(
            out, F32, 2, 5, 8, 0, 0, 0.0, 1.0, [], [], [], 16, seed=1,
            offset=4)


def test_routing_of_converted_chains() -> None:
    names = []

    class _Trace(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            names.append(func.name())
            return func(*args, **(kwargs or {}))

    def traced(fn):
        names.clear()
        with _Trace():
            fn()
        return [n for n in names if not n.startswith("aten::empty")]

    _C.set_fused_init_chains(True)
    torch.manual_seed(42)
    shape = (6, 16, 24)
    m = _module(
        n=lambda: torch.empty(shape).normal_().to(BF16),
        w=lambda: _trunc(shape, F32).to(BF16),
        d=lambda: torch.empty(shape).uniform_().div_(2.0).to(BF16),
        f8=lambda: torch.empty(shape).normal_().to(FP8),
    )
    one = "tdx::rng_chain_cast_shard_win_"
    for t in (m.n, m.w):
        for dim in range(3):
            assert traced(
                lambda: _C.materialize_tensor_shard(t, 1, 5, dim)) == [one]
    # Two levels: the box op at the source dtype, then the conversion.
    two = [(1, 4), (2, 9), (3, 11)]
    assert traced(lambda: _block(m.n, two)) == ["tdx::rng_box_", "tdx::copy_"]
    assert traced(lambda: _block(m.w, two)) == ["tdx::rng_box_", "tdx::copy_"]
    # div_ is outside the fusable set; fp8 is outside the cast kernels.
    assert traced(lambda: _C.materialize_tensor_shard(m.d, 1, 5, 1)) == [
        "tdx::uniform_shard_win_", "aten::div_.Tensor", "tdx::copy_"]
    got = traced(lambda: _C.materialize_tensor_shard(m.f8, 1, 5, 1))
    assert got[0] == "tdx::normal_shard_win_" and "tdx::copy_" not in got
    assert any(n.startswith("aten::to") or n.startswith("aten::_to_copy")
               for n in got)
    # Switched off: step by step, still shard-sized.
    _C.set_fused_init_chains(False)
    got = traced(lambda: _C.materialize_tensor_shard(m.w, 1, 5, 1))
    assert got[0] == "tdx::uniform_shard_win_" and got[-1] == "tdx::copy_"
    assert len(got) == 6
