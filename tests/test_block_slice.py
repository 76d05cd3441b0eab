# N-d block materialization (materialize_tensor_block / tdx::rng_box_):
# planner routing, the CPU reference op and the public fallback —
# everything that can be checked without a GPU. A full materialization of
# the same tape is the oracle throughout: a block must equal full[box]
# bit for bit.

import itertools
import os
import random

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from torchdistx_amd import _C, deferred_init
from torchdistx_amd.parallel import (
    materialize_tensor_block,
    materialize_tensor_shard,
)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(16, 24), (33, 9), (5, 3, 17), (3, 4, 5, 6, 7)]

# TailOp codes (csrc/core/deferred_init.h).
ERFINV, MUL, ADD, SUB, CLAMP, CLAMP_MIN, CLAMP_MAX, NEG, ABS = range(9)


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
                setattr(self, name, torch.nn.Parameter(fn()))

    return deferred_init(M)


def _trunc(shape, dtype):
    w = torch.empty(shape, dtype=dtype)
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
    """The boxes every (shape, dtype, init) case covers: every dim
    partial, the middle dim full, empty on one dim, the whole tensor, a
    single row and a single column."""
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
    return {
        "partial": partial,
        "mid_full": mid_full,
        "empty": empty,
        "whole": whole,
        "row": row,
        "col": col,
    }


def _index(box):
    return tuple(slice(lo, hi) for lo, hi in box)


def _block(t, box):
    return _C.materialize_tensor_block(
        t, [lo for lo, _ in box], [hi for _, hi in box]
    )


@pytest.mark.parametrize("init", sorted(INITS))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_blocks_match_the_full_tensor(shape, dtype, init) -> None:
    torch.manual_seed(31)
    m = _module(w=lambda: INITS[init](shape, dtype))
    boxes = _boxes(shape)
    got = {}
    # Explicitly on covers the float32 erfinv_ step too.
    for fused in (True, False):
        _C.set_fused_init_chains(fused)
        for name, box in boxes.items():
            got[fused, name] = _block(m.w, box)
    full = _C.materialize_tensor(m.w).detach()
    assert full.dtype == dtype and not full.isnan().any()
    for (fused, name), block in got.items():
        want = full[_index(boxes[name])]
        assert block.shape == want.shape, (fused, name)
        assert block.is_contiguous()
        assert torch.equal(block, want), (fused, name, boxes[name])


class _Trace(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(func.name())
        return func(*args, **(kwargs or {}))


def _traced(fn):
    with _Trace() as tr:
        fn()
    return [n for n in tr.names if not n.startswith("aten::empty")]


def test_routing_of_boxes_to_ops() -> None:
    _C.set_fused_init_chains(True)
    torch.manual_seed(32)
    shape = (6, 16, 24)
    m = _module(
        w=lambda: _trunc(shape, torch.float32),
        n=lambda: torch.empty(shape).normal_(),
        d=lambda: torch.empty(shape).uniform_().div_(2.0),
        f=lambda: torch.empty(shape).fill_(2.0),
        z=lambda: torch.zeros(shape),
        m2=lambda: _trunc((16, 24), torch.float32),
    )

    def block(t, *box):
        return lambda: _block(t, list(box))

    two = ((1, 4), (2, 9), (3, 11))  # two strided levels over the runs
    # Two or more levels: exactly one box launch, tail included.
    assert _traced(block(m.w, *two)) == ["tdx::rng_box_"]
    assert _traced(block(m.n, *two)) == ["tdx::rng_box_"]
    # div_ is outside the fusable set: the box op, then step by step.
    assert _traced(block(m.d, *two)) == ["tdx::rng_box_", "aten::div_.Tensor"]
    _C.set_fused_init_chains(False)
    names = _traced(block(m.w, *two))
    assert names[0] == "tdx::rng_box_" and len(names) == 5
    _C.set_fused_init_chains(True)
    # Fill and zero steps fill the shard.
    assert _traced(block(m.f, *two)) == ["aten::fill_.Scalar"]
    assert _traced(block(m.z, *two)) == ["aten::zero_"]

    # One-dim boxes launch what materialize_tensor_shard launches.
    whole = [(0, n) for n in shape]
    for dim, (lo, hi) in enumerate(two):
        box = list(whole)
        box[dim] = (lo, hi)
        for t in (m.w, m.n, m.d):
            assert _traced(block(t, *box)) == _traced(
                lambda: _C.materialize_tensor_shard(t, lo, hi, dim))
    assert _traced(block(m.w, whole[0], whole[1], (3, 11))) == [
        "tdx::rng_chain_shard_win_"]
    assert _traced(block(m.d, whole[0], (2, 9), whole[2]))[0] == (
        "tdx::uniform_shard_win_")
    assert _traced(block(m.d, (1, 4), whole[1], whole[2]))[0] == (
        "tdx::uniform_shard_")
    # One level is a window whatever the number of dims behind it: a full
    # middle dim folds away, and so does the row/column block of a matrix.
    assert _traced(block(m.n, (1, 4), whole[1], (3, 11))) == [
        "tdx::normal_shard_win_"]
    assert _traced(block(m.m2, (2, 5), (3, 11))) == [
        "tdx::rng_chain_shard_win_"]
    # materialize_tensor_shard itself is untouched by all this.
    assert _traced(lambda: _C.materialize_tensor_shard(m.w, 3, 11, 2)) == [
        "tdx::rng_chain_shard_win_"]


def test_cpu_box_op_matches_the_window_op_and_the_full_op() -> None:
    seed, offset = 77, 12
    for dtype in DTYPES:
        full = torch.empty(6, 10, 12, dtype=dtype)
        torch.ops.tdx.uniform_(full, -1.0, 1.0, seed=seed, offset=offset)
        out = torch.empty(4, 7, 8, dtype=dtype)
        torch.ops.tdx.rng_box_(out, [4, 7], [120, 12], 8, 120 + 24 + 3, 0,
                               -1.0, 1.0, [MUL, ADD], [0.5, 0.25], [0.0, 0.0],
                               720, seed, offset)
        ref = full[1:5, 2:9, 3:11].contiguous()
        ref.mul_(0.5).add_(0.25)
        assert torch.equal(out, ref)
        # One level: the numbers of the window op, and its bits.
        win = torch.empty(6, 10, 5, dtype=dtype)
        torch.ops.tdx.uniform_shard_win_(win, 60, 5, 12, 4, -1.0, 1.0,
                                         seed=seed, offset=offset)
        box = torch.empty(6, 10, 5, dtype=dtype)
        torch.ops.tdx.rng_box_(box, [60], [12], 5, 4, 0, -1.0, 1.0, [], [],
                               [], 720, seed, offset)
        assert torch.equal(box, win)
        assert torch.equal(box, full[:, :, 4:9])


def test_box_op_validation() -> None:
    def call(shard=None, extents=(4, 7), strides=(120, 12), run_len=8,
             g_off=147, dist=0, p0=0.0, p1=1.0, ops=(), s0=(), s1=(),
             full_numel=720):
        shard = torch.empty(4, 7, 8) if shard is None else shard
        return torch.ops.tdx.rng_box_(
            shard, list(extents), list(strides), run_len, g_off, dist, p0,
            p1, list(ops), list(s0), list(s1), full_numel, 5, 8)

    call()  # the baseline is valid
    bad = [
        dict(extents=(), strides=()),  # 0 levels
        dict(extents=(1, 1, 1, 4, 7), strides=(720, 720, 720, 120, 12)),
        dict(extents=(4, 7), strides=(120,)),  # unequal lengths
        dict(extents=(-4, -7)),
        dict(run_len=-8),
        dict(g_off=-1),
        dict(strides=(120, 7)),  # innermost stride < run_len
        dict(strides=(80, 12)),  # outer stride < extent * stride inside
        dict(run_len=7),  # numel mismatch
        dict(full_numel=586),  # the box ends at element 587
        dict(g_off=281),  # ... and at 721 from here
        dict(shard=torch.empty(4, 7, 16)[:, :, ::2]),  # not contiguous
        dict(shard=torch.empty(4, 7, 8, dtype=torch.float64)),
        dict(dist=3),
        dict(dist=1, p1=-1.0),
        dict(dist=2, p0=1.5),
        dict(ops=[99], s0=[0.0], s1=[0.0]),
        dict(ops=[NEG] * 9, s0=[0.0] * 9, s1=[0.0] * 9),
        dict(ops=[NEG], s0=[], s1=[]),
    ]
    call(full_numel=587)
    call(g_off=280)
    for kwargs in bad:
        with pytest.raises(RuntimeError):
            call(**kwargs)
            pytest.fail(f"accepted {kwargs}")
    # An empty box launches nothing and leaves the shard alone.
    out = torch.empty(0, 7, 8)
    assert call(shard=out, extents=(0, 7)) is out


def test_block_argument_errors() -> None:
    torch.manual_seed(33)
    m = _module(w=lambda: torch.empty(6, 8).normal_())
    with pytest.raises(RuntimeError):
        _C.materialize_tensor_block(m.w, [0], [6])
    with pytest.raises(RuntimeError, match="invalid slice range"):
        _C.materialize_tensor_block(m.w, [0, 5], [6, 3])
    with pytest.raises(RuntimeError, match="invalid slice range"):
        _C.materialize_tensor_block(m.w, [0, 0], [7, 8])
    with pytest.raises(ValueError):
        _C.materialize_tensor_block(torch.empty(6, 8), [0, 0], [6, 8])
    with pytest.raises(ValueError):
        materialize_tensor_block(m.w, [(0, 6)])


def test_zero_dim_tensor_and_none_ranges() -> None:
    torch.manual_seed(34)
    m = _module(s=lambda: torch.empty(()).normal_(),
                w=lambda: torch.empty(6, 8, 10).normal_())
    scalar = _C.materialize_tensor_block(m.s, [], [])
    block = materialize_tensor_block(m.w, [(1, 4), None, (2, 9)])
    assert block.requires_grad and block.is_leaf
    full_s = _C.materialize_tensor(m.s).detach()
    full_w = _C.materialize_tensor(m.w).detach()
    assert torch.equal(scalar, full_s)
    assert torch.equal(block.detach(), full_w[1:4, :, 2:9])


def test_more_than_four_levels_falls_back() -> None:
    shape = (3,) * 6
    torch.manual_seed(35)
    m = _module(w=lambda: torch.empty(shape).normal_())
    with pytest.raises(RuntimeError, match="slice materialization"):
        _C.materialize_tensor_block(m.w, [1] * 6, [3] * 6)
    block = materialize_tensor_block(m.w, [(1, 3)] * 6)
    full = _C.materialize_tensor(m.w).detach()
    assert torch.equal(block.detach(), full[(slice(1, 3),) * 6])
    assert block.is_contiguous()


def test_fallback_for_unsupported_tapes() -> None:
    torch.manual_seed(36)
    gen = torch.Generator().manual_seed(5)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.g = torch.nn.Parameter(
                torch.empty(8, 12).normal_(generator=gen))
            pos = torch.arange(8, dtype=torch.float32)
            self.register_buffer(
                "cache", torch.outer(pos, torch.ones(12)).cos())

    m = deferred_init(M)
    for t in (m.g, m.cache):
        with pytest.raises(RuntimeError, match="slice materialization"):
            _C.materialize_tensor_block(t, [2, 3], [6, 11])
    got_g = materialize_tensor_block(m.g, [(2, 6), (3, 11)])
    got_c = materialize_tensor_block(m.cache, [(2, 6), (3, 11)])
    assert got_g.requires_grad and not got_c.requires_grad
    full_g = _C.materialize_tensor(m.g).detach()
    full_c = _C.materialize_tensor(m.cache)
    assert torch.equal(got_g.detach(), full_g[2:6, 3:11])
    assert torch.equal(got_c, full_c[2:6, 3:11])
    assert got_g.is_contiguous() and got_c.is_contiguous()
    # The fallback copies: the block does not keep the full tensor alive.
    assert got_c.untyped_storage().nbytes() == got_c.numel() * 4


def test_block_composes_with_single_dim_slices() -> None:
    # The route the docs used to recommend gives the same bits.
    torch.manual_seed(37)
    m = _module(w=lambda: _trunc((4, 12, 16), torch.bfloat16))
    block = materialize_tensor_block(m.w, [(1, 3), (0, 6), (8, 16)])
    composed = materialize_tensor_shard(m.w, 8, 16, 2)[1:3, 0:6].clone()
    assert torch.equal(block.detach(), composed.detach())


# ---- seeded fuzz, in the style of test_slice_fuzz.py -----------------------

_FUZZ_SHAPES = [
    (7,), (9, 8), (3, 5), (16, 17), (2, 3, 5), (4, 4, 4), (5, 1, 9),
    (3, 8, 16), (2, 3, 4, 5), (2, 2, 3, 2, 8), (3, 1, 2, 1, 3, 2),
]


def _fuzz_chain(rng, shape, dtype):
    kind = rng.choice(["uniform", "normal", "bernoulli", "fill", "zero"])
    t = torch.empty(shape, dtype=dtype)
    if kind == "uniform":
        a = rng.uniform(-2.0, 0.0)
        t.uniform_(a, a + rng.uniform(0.1, 3.0))
    elif kind == "normal":
        t.normal_(rng.uniform(-1.0, 1.0), rng.uniform(0.1, 2.0))
    elif kind == "bernoulli":
        t.bernoulli_(rng.uniform(0.0, 1.0))
    elif kind == "fill":
        t.fill_(rng.uniform(-3.0, 3.0))
    else:
        t.zero_()
    for _ in range(rng.randint(0, 3)):
        op = rng.choice(["mul", "add", "clamp", "abs", "erfinv", "neg", "div"])
        if op == "mul":
            t.mul_(rng.uniform(-2.0, 2.0))
        elif op == "add":
            t.add_(rng.uniform(-1.0, 1.0))
        elif op == "clamp":
            lo = rng.uniform(-1.0, 0.0)
            t.clamp_(min=lo, max=lo + rng.uniform(0.1, 2.0))
        elif op == "abs":
            t.abs_()
        elif op == "erfinv":
            t.clamp_(min=-0.999, max=0.999)
            t.erfinv_()
        elif op == "div":
            t.div_(rng.uniform(0.5, 2.0))
        else:
            t.neg_()
    if rng.random() < 0.3:
        t = t.detach()
    return t


def _fuzz_case(seed: int) -> None:
    rng = random.Random(seed)
    shape = rng.choice(_FUZZ_SHAPES)
    dtype = rng.choice(DTYPES)
    _C.set_fused_init_chains(rng.random() < 0.7)

    def build():
        class Holder(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.t = _fuzz_chain(rng2, shape, dtype)

        return Holder()

    rng2 = random.Random(seed + 1)
    torch.manual_seed(seed)
    full = _C.materialize_tensor(deferred_init(build).t)
    for _ in range(2):
        box = []
        for n in shape:
            mode = rng.random()
            if mode < 0.25:
                box.append((0, n))
            else:
                lo = rng.randint(0, n)
                box.append((lo, rng.randint(lo, n)))
        # Independent tape, same seed.
        rng2 = random.Random(seed + 1)
        torch.manual_seed(seed)
        holder = deferred_init(build)
        block = materialize_tensor_block(holder.t, box)
        want = full[_index(box)]
        assert block.shape == want.shape
        assert torch.equal(block, want), (seed, shape, dtype, box)


@pytest.mark.parametrize("chunk", range(10))
def test_block_fuzz_cpu(chunk: int) -> None:
    # 200 seeded (shape, box, dtype, init) cases, 20 per test.
    for seed in range(chunk * 20, chunk * 20 + 20):
        _fuzz_case(5000 + seed)


def test_every_box_of_a_small_tensor() -> None:
    # Exhaustive over a (3, 4, 5) bf16 tensor: 10 * 15 * 21 boxes.
    torch.manual_seed(38)
    m = _module(w=lambda: torch.empty(3, 4, 5, dtype=torch.bfloat16).normal_())
    full = None
    pairs = [
        [(lo, hi) for lo in range(n + 1) for hi in range(lo, n + 1)]
        for n in (3, 4, 5)
    ]
    blocks = {
        box: _block(m.w, box) for box in itertools.product(*pairs)
    }
    full = _C.materialize_tensor(m.w).detach()
    for box, block in blocks.items():
        assert torch.equal(block, full[_index(box)]), box
