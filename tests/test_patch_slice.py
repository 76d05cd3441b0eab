# Slice materialization of tensors whose init overwrites a contiguous
# sub-range (nn.Embedding(padding_idx=i), HF-style `weight.data[i].zero_()`,
# fused weights initialized by parts): the planner, the CPU reference of
# tdx::patch_box_ and the public fallbacks — everything that can be checked
# without a GPU. A full materialization of the same tape, indexed, is the
# oracle throughout, and equality is torch.equal.

import os
import random

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from tests import _patch_oracle as po
from torchdistx_amd import _C, deferred_init
from torchdistx_amd import parallel
from torchdistx_amd.models import TINY_PADDED, build_model

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(16, 24), (33, 9), (5, 3, 17)]


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


def _trunc(w):
    torch.nn.init.trunc_normal_(w, mean=0.1, std=0.7, a=-1.0, b=1.5)


BASES = {
    "normal": lambda w: w.normal_(0.1, 0.8),
    "uniform": lambda w: w.uniform_(-0.5, 1.5),
    "fill": lambda w: w.fill_(0.37),
    "trunc": _trunc,
}


def _row_zero(w):
    w[2].zero_()


def _rows_fill(w):
    w[1:4].fill_(0.37)


def _data_row_zero(w):
    w.data[w.shape[0] - 1].zero_()


def _inner_normal(w):
    # A stretch of one row; on the 3-d shape a stretch of w[i][j].
    if w.dim() == 3:
        w[3][1][2:15].normal_(0.1, 0.8)
    else:
        w[3, 2:7].normal_(0.1, 0.8)


def _by_parts(w):
    k = w.shape[0] // 3 + 1
    w[:k].normal_(0, 0.5)
    w[k:].uniform_()


def _flat_bernoulli(w):
    w.view(-1)[7:29].bernoulli_(0.3)


PATCHES = {
    "row_zero": _row_zero,
    "rows_fill": _rows_fill,
    "data_row_zero": _data_row_zero,
    "inner_normal": _inner_normal,
    "by_parts": _by_parts,
    "flat_bernoulli": _flat_bernoulli,
}


def _boxes(shape):
    """test_block_slice._boxes: every dim partial, the middle dim full,
    empty on one dim, the whole tensor, a single row and a single column."""
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
    # Boxes aimed at the patches above: one that ends before row 2 starts
    # (it misses `row_zero`), one inside rows 1..4 only.
    first_rows = list(whole)
    first_rows[0] = (0, 2)
    inside = list(partial)
    inside[0] = (2, 4)
    return {"partial": partial, "mid_full": mid_full, "empty": empty,
            "whole": whole, "row": row, "col": col,
            "first_rows": first_rows, "inside": inside}


def _ranges(n):
    """Single-dim shard ranges: every pair of cut points around the ends,
    the thirds and the middle of the dim, empty ranges included."""
    cuts = sorted({0, 1, 2, n // 3, n // 2, (2 * n) // 3, n - 2, n - 1, n}
                  & set(range(n + 1)))
    return [(a, b) for a in cuts for b in cuts if a <= b]


def _index(box):
    return tuple(slice(lo, hi) for lo, hi in box)


def _block(t, box):
    return _C.materialize_tensor_block(
        t, [lo for lo, _ in box], [hi for _, hi in box])


def _check_all_slices(t, shape, label=None):
    """Every shard range and every box of `t`, taken BEFORE the full
    materialization (which consumes the tape), against the full tensor."""
    shards = {}
    for dim, n in enumerate(shape):
        for a, b in _ranges(n):
            shards[dim, a, b] = _C.materialize_tensor_shard(t, a, b, dim)
    boxes = _boxes(shape)
    blocks = {name: _block(t, box) for name, box in boxes.items()}
    full = _C.materialize_tensor(t).detach()
    assert not full.isnan().any()
    for (dim, a, b), shard in shards.items():
        want = full.narrow(dim, a, b - a)
        assert shard.shape == want.shape and shard.dtype == full.dtype
        assert torch.equal(shard, want), (label, "shard", dim, a, b)
    for name, block in blocks.items():
        want = full[_index(boxes[name])]
        assert block.shape == want.shape and block.is_contiguous()
        assert torch.equal(block, want), (label, "block", name)
    return full


@pytest.mark.parametrize("patch", sorted(PATCHES))
@pytest.mark.parametrize("base", sorted(BASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_patched_tensors_slice_like_the_full_tensor(shape, dtype, base,
                                                    patch) -> None:
    def build():
        w = torch.empty(shape, dtype=dtype)
        BASES[base](w)
        PATCHES[patch](w)
        return w

    torch.manual_seed(41)
    m = _module(w=build)
    assert _C.tensor_chain_plan(m.w) is None
    assert _C.tensor_init_plan(m.w) is None
    plan = _C.tensor_patch_plan(m.w)
    if base == "trunc" and dtype == torch.float32:
        # erfinv_ on float32 fuses only on request: no plan, slices anyway.
        assert plan is None
    else:
        assert plan is not None and len(plan["patches"]) >= 1
    full = _check_all_slices(m.w, shape, (base, patch))
    if patch == "row_zero":
        assert (full[2] == 0).all() and (full[1] != 0).any()


def test_the_matrix_hits_every_edge() -> None:
    # (33, 9): rows start mid-group for every dtype (9 is no multiple of 4
    # or 8) and no patch length is a group multiple; some boxes miss the
    # patch, some cut it at both ends, one is empty.
    shape = (33, 9)
    boxes = _boxes(shape)
    g = po.global_indices(*po.box_geometry(shape, boxes["first_rows"]))
    assert g.max() < 2 * 9  # misses `row_zero` (elements 18..27)
    g = po.global_indices(*po.box_geometry(shape, boxes["partial"]))
    inside = (g >= 7) & (g < 29)  # `flat_bernoulli`
    assert inside.any() and not inside.all()
    g = po.global_indices(*po.box_geometry(shape, boxes["inside"]))
    inside = (g >= 9) & (g < 36)  # `rows_fill`: rows 1..4
    assert inside.all()  # the patch is cut at both ends
    assert g.min() > 9 and g.max() < 35
    assert po.global_indices(
        *po.box_geometry(shape, boxes["empty"])).numel() == 0
    assert (2 * 9) % 4 != 0 and 9 % 4 != 0 and (29 - 7) % 4 != 0


# ---- nn.Embedding(padding_idx=...) and HF-style _init_weights --------------

def _hf_init_weights(module):
    if isinstance(module, torch.nn.Embedding):
        module.weight.data.normal_(mean=0.0, std=0.02)
        if module.padding_idx is not None:
            module.weight.data[module.padding_idx].zero_()


def _embedding_builders():
    def stock(idx):
        return lambda: torch.nn.Embedding(50, 12, padding_idx=idx)

    def hf():
        emb = torch.nn.Embedding(50, 12, padding_idx=3)
        emb.apply(_hf_init_weights)
        return emb

    return {"padding_idx=3": stock(3), "padding_idx=-1": stock(-1), "hf": hf}


@pytest.mark.parametrize("cast", [None, "fused", "unfused"])
@pytest.mark.parametrize("name", sorted(_embedding_builders()))
def test_padded_embeddings(name, cast) -> None:
    builder = _embedding_builders()[name]
    if cast is not None:
        _C.set_fused_init_chains(cast == "fused")
        plain = builder
        builder = lambda: plain().to(torch.bfloat16)  # noqa: E731
    torch.manual_seed(42)
    emb = deferred_init(builder)
    pad = 49 if name == "padding_idx=-1" else 3
    plan = _C.tensor_patch_plan(emb.weight)
    assert _C.tensor_chain_plan(emb.weight) is None
    if cast != "unfused":
        assert plan is not None
        # Dead patches (the HF pass overwrites nn.Embedding's own) are gone.
        assert [(p["lo"], p["len"], p["kind"]) for p in plan["patches"]] == [
            (pad * 12, 12, "fill" if name != "hf" else "zero")]
        if cast is not None:
            assert plan["src_dtype"] == torch.float32
            assert plan["dtype"] == torch.bfloat16
    w = emb.weight
    # Row shards around the padded row, and column shards.
    rows = [(0, pad), (pad, pad + 1), (pad + 1, 50), (max(pad - 2, 0), pad + 1),
            (0, 50), (pad, pad), (0, 25), (25, 50)]
    cols = [(0, 12), (0, 5), (5, 12), (3, 4), (11, 12)]
    shards = [(0, a, b, _C.materialize_tensor_shard(w, a, b, 0))
              for a, b in rows]
    shards += [(1, a, b, _C.materialize_tensor_shard(w, a, b, 1))
               for a, b in cols]
    blocks = [(box, _block(w, box)) for box in
              ([(pad - 1, pad + 1), (2, 9)], [(0, pad), (0, 12)],
               [(pad, 50), (11, 12)])]
    full = _C.materialize_tensor(w).detach()
    assert full.dtype == (torch.float32 if cast is None else torch.bfloat16)
    assert (full[pad] == 0).all() and (full[pad - 1] != 0).any()
    for dim, a, b, shard in shards:
        assert shard.dtype == full.dtype
        assert torch.equal(shard, full.narrow(dim, a, b - a)), (dim, a, b)
    for box, block in blocks:
        assert torch.equal(block, full[_index(box)]), box


class _Trace(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []
        self.largest = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.names.append(func.name())
        if isinstance(out, torch.Tensor):
            self.largest = max(self.largest, out.numel())
        return out


def test_constant_patch_and_cast_routes() -> None:
    def build():
        return torch.nn.Embedding(50, 12, padding_idx=3).to(torch.bfloat16)

    torch.manual_seed(43)
    emb = deferred_init(build)
    _C.set_fused_init_chains(True)
    with _Trace() as tr:
        _C.materialize_tensor_shard(emb.weight, 0, 10, 1)
    ops = [n for n in tr.names if not n.startswith("aten::empty")]
    assert ops == ["tdx::rng_chain_cast_shard_win_", "tdx::patch_box_"]
    _C.set_fused_init_chains(False)
    with _Trace() as tr:
        _C.materialize_tensor_shard(emb.weight, 0, 10, 1)
    ops = [n for n in tr.names if not n.startswith("aten::empty")]
    assert ops == ["tdx::normal_shard_win_", "tdx::patch_box_", "tdx::copy_"]


def test_rng_patch_with_a_cast_takes_the_segment_path() -> None:
    def build():
        w = torch.empty(33, 9).uniform_(-1.0, 1.0)
        w[:13].normal_()
        return w.to(torch.bfloat16)

    for fused in (True, False):
        _C.set_fused_init_chains(fused)
        torch.manual_seed(44)
        m = _module(w=build)
        assert _C.tensor_patch_plan(m.w) is None
        assert _C.tensor_chain_plan(m.w) is None
        with _Trace() as tr:
            _C.materialize_tensor_shard(m.w, 2, 20)
        assert "tdx::patch_box_" in tr.names and "tdx::copy_" in tr.names
        full = _check_all_slices(m.w, (33, 9), fused)
        assert full.dtype == torch.bfloat16


# ---- order ----------------------------------------------------------------

@pytest.mark.parametrize("order", ["fill_then_normal", "normal_then_fill"])
def test_overlapping_patches_apply_in_tape_order(order) -> None:
    def build():
        w = torch.empty(33, 9, dtype=torch.bfloat16).uniform_()
        if order == "fill_then_normal":
            w[2:11].fill_(0.37)
            w[7:19].normal_(0.1, 0.8)
        else:
            w[7:19].normal_(0.1, 0.8)
            w[2:11].fill_(0.37)
        return w

    torch.manual_seed(45)
    m = _module(w=build)
    plan = _C.tensor_patch_plan(m.w)
    kinds = [p["kind"] for p in plan["patches"]]
    assert kinds == (["fill", "normal"] if order == "fill_then_normal"
                     else ["normal", "fill"])
    full = _check_all_slices(m.w, (33, 9), order)
    overlap = full[7:11]
    fill = torch.tensor(0.37, dtype=torch.bfloat16)
    if order == "fill_then_normal":
        assert (overlap != fill).any()
    else:
        assert (overlap == fill).all()


def test_a_whole_tensor_value_step_kills_earlier_patches() -> None:
    def patched():
        w = torch.empty(16, 24).uniform_()
        w[3].zero_()
        w[5:9].normal_()
        w.normal_(0.1, 0.8)
        return w

    def plain():
        w = torch.empty(16, 24).uniform_()
        torch.empty(24).zero_()  # keep the Philox slots aligned
        torch.empty(4, 24).normal_()
        w.normal_(0.1, 0.8)
        return w

    torch.manual_seed(46)
    a = _module(w=patched)
    torch.manual_seed(46)
    b = _module(w=plain)
    plan = _C.tensor_chain_plan(a.w)
    assert plan is not None and plan["kind"] == "normal"
    assert _C.tensor_patch_plan(a.w)["patches"] == []
    shard = _C.materialize_tensor_shard(a.w, 2, 9)
    full_a = _C.materialize_tensor(a.w).detach()
    full_b = _C.materialize_tensor(b.w).detach()
    assert torch.equal(full_a, full_b)
    assert torch.equal(shard, full_a[2:9])
    assert (full_a[3] != 0).any()


def test_whole_tensor_steps_through_a_view_stay_whole() -> None:
    def build():
        w = torch.empty(16, 24)
        w.view(-1).normal_(0.1, 0.8)
        return w

    def direct():
        return torch.empty(16, 24).normal_(0.1, 0.8)

    torch.manual_seed(47)
    a = _module(w=build)
    torch.manual_seed(47)
    b = _module(w=direct)
    plan = _C.tensor_chain_plan(a.w)
    assert plan is not None and plan == _C.tensor_chain_plan(b.w)
    shard = _C.materialize_tensor_shard(a.w, 3, 11, 1)
    full = _C.materialize_tensor(a.w).detach()
    assert torch.equal(shard, full[:, 3:11])
    assert torch.equal(full, _C.materialize_tensor(b.w).detach())


# ---- what still raises ------------------------------------------------------

def _sub_add(w):
    w[2].add_(1.0)


def _sub_mul(w):
    w[:5].mul_(0.5)


def _mul_after_patch(w):
    w[2].zero_()
    w.mul_(0.5)


def _transposed_row(w):
    w.t()[0].fill_(1.0)


def _strided_rows(w):
    w[::2].zero_()


def _column(w):
    w[:, 1].zero_()


def _generator_patch(w):
    w[2:5].normal_(generator=torch.Generator().manual_seed(5))


STILL_RAISING = {
    "sub_add": _sub_add,
    "sub_mul": _sub_mul,
    "mul_after_patch": _mul_after_patch,
    "transposed_row": _transposed_row,
    "strided_rows": _strided_rows,
    "column": _column,
    "generator_patch": _generator_patch,
}


@pytest.mark.parametrize("name", sorted(STILL_RAISING))
def test_unsupported_partial_writes_still_raise_and_fall_back(name) -> None:
    def build():
        w = torch.empty(16, 24).normal_()
        STILL_RAISING[name](w)
        return w

    torch.manual_seed(48)
    m = _module(w=build)
    with pytest.raises(RuntimeError, match="slice materialization"):
        _C.materialize_tensor_shard(m.w, 1, 9, 0)
    with pytest.raises(RuntimeError, match="slice materialization"):
        _C.materialize_tensor_block(m.w, [1, 2], [9, 20])
    assert _C.tensor_patch_plan(m.w) is None
    assert _C.tensor_chain_plan(m.w) is None
    shard = parallel.materialize_tensor_shard(m.w, 1, 9, 0)
    col = parallel.materialize_tensor_shard(m.w, 0, 7, 1)
    full = _C.materialize_tensor(m.w).detach()
    assert torch.equal(shard.detach(), full[1:9])
    assert torch.equal(col.detach(), full[:, 0:7])


# ---- the plan ---------------------------------------------------------------

def test_patch_plan_contents() -> None:
    def const():
        w = torch.empty(33, 9, dtype=torch.bfloat16).normal_(0.0, 0.02)
        w[4:6].fill_(0.37)
        return w

    def rng():
        w = torch.empty(33, 9).normal_(0.0, 0.02)
        w[3, 2:7].uniform_(-0.5, 1.5)
        return w

    def const_cast():
        w = torch.empty(33, 9, dtype=torch.float16).normal_(0.0, 0.02)
        w[4:6].fill_(0.37)
        return w.to(torch.bfloat16)

    torch.manual_seed(49)
    m = _module(c=const, r=rng, cc=const_cast)
    for t in (m.c, m.r, m.cc):
        assert _C.tensor_chain_plan(t) is None
        assert _C.tensor_init_plan(t) is None
    c = _C.tensor_patch_plan(m.c)
    assert c["kind"] == "normal" and c["sizes"] == [33, 9]
    assert c["dtype"] == torch.bfloat16 and c["src_dtype"] is None
    assert c["tail"] == [] and c["p1"] == 0.02
    assert c["patches"] == [{"lo": 36, "len": 18, "kind": "fill",
                             "p0": 0.37, "p1": 0.0, "seed": 0, "offset": 0}]
    r = _C.tensor_patch_plan(m.r)
    (p,) = r["patches"]
    assert (p["lo"], p["len"], p["kind"]) == (29, 5, "uniform")
    assert (p["p0"], p["p1"]) == (-0.5, 1.5)
    assert p["seed"] == r["seed"] and p["offset"] != r["offset"]
    cc = _C.tensor_patch_plan(m.cc)
    assert cc["src_dtype"] == torch.float16 and cc["dtype"] == torch.bfloat16
    # Rounded through the source dtype on the host.
    (p,) = cc["patches"]
    assert p["p0"] == float(torch.tensor(0.37, dtype=torch.float16))
    # A chain without patches plans as tensor_chain_plan does.
    torch.manual_seed(49)
    plain = _module(w=lambda: torch.empty(4, 4).normal_())
    plan = _C.tensor_patch_plan(plain.w)
    assert plan.pop("patches") == []
    assert plan == _C.tensor_chain_plan(plain.w)
    assert _C.tensor_patch_plan(torch.empty(3)) is None


# ---- the CPU op against a per-element oracle --------------------------------

_ORACLE_SHAPES = [(40,), (9, 8), (16, 17), (5, 3, 17), (4, 4, 4),
                  (2, 3, 4, 5), (2, 2, 3, 2, 8)]


def _random_box(rng, shape):
    box = []
    for n in shape:
        if rng.random() < 0.3:
            box.append((0, n))
        else:
            lo = rng.randint(0, n)
            box.append((lo, rng.randint(lo, n)))
    return box


@pytest.mark.parametrize("chunk", range(4))
def test_cpu_patch_op_matches_the_oracle(chunk) -> None:
    met = 0
    for seed in range(chunk * 12, chunk * 12 + 12):
        rng = random.Random(7000 + seed)
        shape = rng.choice(_ORACLE_SHAPES)
        dtype = rng.choice(DTYPES)
        numel = 1
        for n in shape:
            numel *= n
        geometry = po.box_geometry(shape, _random_box(rng, shape))
        lo = rng.randint(0, numel)
        length = rng.randint(0, numel - lo)
        dist = rng.randrange(5)
        p0 = rng.uniform(0.0, 1.0)
        p1 = p0 + rng.uniform(0.1, 2.0)
        shard_numel = geometry[2]
        for e in geometry[0]:
            shard_numel *= e
        shard = torch.full((shard_numel,), -7.0, dtype=dtype)  # sentinel
        want, n_inside = po.expected(shard, geometry, lo, length, dist, p0,
                                     p1, 11 + seed, 4 * seed)
        met += n_inside
        out = po.call(shard, geometry, numel, lo, length, dist, p0, p1,
                      11 + seed, 4 * seed)
        assert out is shard
        assert torch.equal(shard, want), (seed, shape, dtype, geometry, lo,
                                          length, dist)
        # Untouched elsewhere: exactly the elements outside the patch keep
        # the sentinel (no distribution here produces -7).
        assert int((shard == -7.0).sum()) == shard_numel - n_inside
    assert met > 0


def test_cpu_patch_op_validation() -> None:
    geometry = ([4, 7], [120, 12], 8, 147)  # ends at element 587

    def call(shard=None, geometry=geometry, full_numel=720, lo=100, length=300,
             dist=po.NORMAL, p0=0.0, p1=1.0, seed=5, offset=8):
        shard = (torch.full((4, 7, 8), -7.0) if shard is None else shard)
        before = shard.clone()
        try:
            return torch.ops.tdx.patch_box_(
                shard, geometry[0], geometry[1], geometry[2], geometry[3],
                full_numel, lo, length, dist, p0, p1, seed, offset)
        except RuntimeError:
            assert torch.equal(shard, before)  # rejected before any write
            raise

    call()  # the baseline is valid
    call(full_numel=587, lo=0, length=587)
    call(dist=po.FILL, seed=None, offset=None)
    call(dist=po.ZERO, seed=None, offset=None)
    bad = [
        dict(geometry=([], [], 8, 147)),
        dict(geometry=([4, 7], [120], 8, 147)),
        dict(geometry=([4, 7], [120, 7], 8, 147)),  # overlapping rows
        dict(geometry=([4, 7], [120, 12], 9, 147)),  # numel mismatch
        dict(full_numel=586),  # the box ends at element 587
        dict(lo=-1),
        dict(length=-1),
        dict(lo=500, length=221),  # ends at 721
        dict(lo=721, length=0),
        dict(dist=5),
        dict(dist=-1),
        dict(dist=po.NORMAL, p1=-1.0),
        dict(dist=po.BERNOULLI, p0=1.5),
        dict(dist=po.NORMAL, seed=None),
        dict(dist=po.UNIFORM, offset=None),
        dict(shard=torch.full((4, 7, 16), -7.0)[:, :, ::2]),
        dict(shard=torch.full((4, 7, 8), -7.0, dtype=torch.float64)),
    ]
    for kwargs in bad:
        with pytest.raises(RuntimeError):
            call(**kwargs)
            pytest.fail(f"accepted {kwargs}")
    # An empty shard and an empty patch launch nothing.
    empty = torch.empty(0, 7, 8)
    assert call(shard=empty, geometry=([0, 7], [120, 12], 8, 147)) is empty
    untouched = torch.full((4, 7, 8), -7.0)
    call(shard=untouched, length=0)
    call(shard=untouched, lo=0, length=147)  # ends where the box starts
    call(shard=untouched, lo=587, length=133)  # starts where it ends
    assert (untouched == -7.0).all()


# ---- the padded model config ------------------------------------------------

def test_padded_config_shards_reassemble_to_the_full_model() -> None:
    for init in ("fast", "stock"):
        cfg = TINY_PADDED if init == "fast" else type(TINY_PADDED)(
            **{**TINY_PADDED.__dict__, "init": "stock"})
        torch.manual_seed(50)
        m = deferred_init(build_model, cfg)
        assert _C.tensor_chain_plan(m.tok_emb.weight) is None
        assert len(_C.tensor_patch_plan(m.tok_emb.weight)["patches"]) == 1
        world = 4
        dim0 = [parallel.materialize_module_dim0_sharded(m, r, world)
                for r in range(world)]
        dims = {"tok_emb.weight": 1, "blocks.0.attn.wo.weight": 1,
                "blocks.0.attn.wq.weight": 0}
        tp = [parallel.materialize_module_tp_sharded(m, dims, r, world)
              for r in range(world)]
        with _Trace() as tr:
            _C.materialize_tensor_shard(m.tok_emb.weight, 0, 32)
        assert "tdx::patch_box_" in tr.names
        # No allocation larger than the shard for the embedding.
        assert tr.largest == 32 * cfg.dim
        with _Trace() as tr:
            _C.materialize_tensor_block(m.tok_emb.weight, [2, 8], [34, 40])
        assert tr.largest == 32 * 32
        full = {n: _C.materialize_tensor(t).detach() for n, t in
                list(m.named_parameters()) + list(m.named_buffers())}
        emb = full["tok_emb.weight"]
        assert (emb[cfg.padding_idx] == 0).all()
        assert (emb[cfg.padding_idx + 1] != 0).any()
        for name, want in full.items():
            got = torch.cat([s[name].detach() for s in dim0], 0)
            assert torch.equal(got, want), (init, name)
            if name in dims:
                got = torch.cat([s[name].detach() for s in tp], dims[name])
            else:
                got = tp[1][name].detach()
            assert torch.equal(got, want), (init, name)


def test_padded_embedding_example_compiles() -> None:
    import py_compile

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    py_compile.compile(
        os.path.join(root, "examples", "init_padded_embedding.py"),
        doraise=True)


def test_padding_idx_none_records_todays_tapes() -> None:
    from torchdistx_amd.models import TINY

    assert TINY.padding_idx is None
    torch.manual_seed(51)
    m = deferred_init(build_model, TINY)
    plan = _C.tensor_chain_plan(m.tok_emb.weight)
    assert plan is not None and plan["kind"] == "normal"
    assert _C.tensor_patch_plan(m.tok_emb.weight)["patches"] == []
