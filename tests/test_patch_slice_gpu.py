# GPU (MI355X) tests of tdx::patch_box_ and of slice materialization of
# tensors whose init overwrites a contiguous sub-range: the patch kernel
# must store, for any box and any patch, exactly what a full
# materialization followed by indexing holds — whole 16-byte groups and
# partial ones, every kind and dtype, on both index instantiations — and
# leave every other element alone.

import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from tests import _patch_oracle as po
from tests.test_block_slice_gpu import CASES

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    os.environ.setdefault("TDX_REQUIRE_NATIVE_INIT", "1")

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SENTINEL = -7.0  # no kind below produces it
SEED, OFFSET = 1234567, 40

# p0, p1 per kind; the fill value is not representable in any of the dtypes.
PARAMS = {po.UNIFORM: (-0.5, 1.5), po.NORMAL: (0.1, 0.8),
          po.BERNOULLI: (0.3, 0.0), po.FILL: (0.37, 0.0), po.ZERO: (0.0, 0.0)}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from torchdistx_amd import _kernels

    assert _kernels.available(), "torchdistx_amd._K must load on a GPU box"
    assert _kernels._K.has_patch_kernel()


_views = {}


def _view(n, dtype, dist):
    """The patch view, drawn once per (length, dtype, kind) with the GPU
    tdx:: op and shared by every geometry that uses it."""
    key = (n, dtype, dist)
    if key not in _views:
        _views[key] = po.draw_view(n, dtype, "cuda", dist, *PARAMS[dist],
                                   SEED, OFFSET)
    return _views[key]


def _check_box(shape, box, lo, length, dtypes=DTYPES, dists=range(5)):
    """patch_box_ over full[box] against "scatter the view into the full
    tensor, then index"."""
    numel = 1
    for n in shape:
        numel *= n
    geometry = po.box_geometry(shape, box)
    index = tuple(slice(a, b) for a, b in box)
    touched = None
    for dtype in dtypes:
        for dist in dists:
            full = torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
            full.view(-1)[lo:lo + length] = _view(length, dtype, dist)
            want = full[index]
            shard = torch.full(want.shape, SENTINEL, dtype=dtype,
                               device="cuda")
            out = po.call(shard, geometry, numel, lo, length, dist,
                          *PARAMS[dist], SEED, OFFSET)
            assert out is shard
            assert torch.equal(shard, want), (shape, box, lo, length, dtype,
                                              dist)
            touched = int((want != SENTINEL).sum())
    return touched


@pytest.mark.parametrize("run_len,col0", [(3, 5), (8, 8), (29, 7), (32, 8)])
def test_group_and_alignment_edges(run_len, col0) -> None:
    # Rows of 40 elements, runs shorter than a group, exactly one group,
    # odd, and aligned; patches that start on a group boundary of the
    # tensor, mid-group and on a group's last lane, of 1, 7, 8, 9 and 4099
    # elements (the long one spans a hundred rows and ends mid-group).
    shape = (600, 40)
    box = [(1, 590), (col0, col0 + run_len)]
    for patch_lo in (800, 803, 807):
        assert patch_lo % 8 in (0, 3, 7)
        for patch_len in (1, 7, 8, 9, 4099):
            _check_box(shape, box, patch_lo, patch_len)


@pytest.mark.parametrize("case", ["four_levels", "four_levels_aligned"])
def test_four_level_boxes(case) -> None:
    shape, box = CASES[case]
    extents, g_strides, run_len, g_off = po.box_geometry(shape, box)
    numel = 3 * 4 * 5 * 6 * 16
    last = g_off + sum((e - 1) * s for e, s in zip(extents, g_strides))
    # Partial first and last rows of the box.
    assert _check_box(shape, box, g_off + 3, last + 5 - (g_off + 3)) > 0
    # The whole tensor, and a patch that starts and ends between rows.
    assert _check_box(shape, box, 0, numel) > 0
    assert _check_box(shape, box, g_off + run_len, 3 * 96 + 2) > 0
    # Missing the box: before it, behind it, and in a gap between two rows.
    assert _check_box(shape, box, 0, g_off) == 0
    assert _check_box(shape, box, last + run_len, numel - last - run_len) == 0
    assert _check_box(shape, box, g_off + run_len, 16 - run_len) == 0


def test_patch_equal_to_the_box_and_empty_shards() -> None:
    # A flat box and exactly its elements; 8-aligned and not.
    assert _check_box((64,), [(8, 40)], 8, 32) == 32
    assert _check_box((64,), [(5, 42)], 5, 37) == 37
    # A row block of a matrix and exactly its elements.
    assert _check_box((12, 24), [(3, 7), (0, 24)], 72, 96) == 96
    # Empty shards launch nothing.
    assert _check_box((12, 24), [(3, 3), (0, 24)], 0, 288) == 0
    assert _check_box((12, 24), [(3, 7), (5, 5)], 0, 288) == 0
    # ... and so does an empty patch.
    assert _check_box((12, 24), [(3, 7), (0, 24)], 80, 0) == 0


def test_more_work_items_than_the_capped_grid_has_threads() -> None:
    # The grid is capped at 16384 blocks x 256 threads = 4.19M work items.
    # 5000 rows of 4096 f32 elements are 1025 (row, group) slots each,
    # 5.1M items: most threads take two. The patch covers all but the ends
    # of the first and last row; the runs start at column 8 of 4104, so a
    # row's view elements start mid-group for most rows. (82 MB tensors.)
    shape = (5000, 4104)
    box = [(0, 5000), (8, 4104)]
    lo = 4104 + 5
    hi = 4104 * 4999 + 77
    touched = _check_box(shape, box, lo, hi - lo, dtypes=[torch.float32],
                         dists=[po.NORMAL])
    assert touched > 16384 * 256 * 4
    _views.clear()


def _expected_by_ranges(shard, geometry, lo, length, dist, dtype):
    """Oracle for patches too long to draw: each row's view elements
    [k0, k1) come from the flat shard ops over that range."""
    extents, g_strides, run_len, g_off = geometry
    starts = po.global_indices(extents, g_strides, 1, g_off).tolist()
    want = shard.clone().view(-1)
    p0, p1 = PARAMS[dist]
    op = (torch.ops.tdx.uniform_shard_ if dist == po.UNIFORM
          else torch.ops.tdx.normal_shard_)
    n = 0
    for r, rs in enumerate(starts):
        a, b = max(rs, lo), min(rs + run_len, lo + length)
        if a >= b:
            continue
        piece = torch.empty(b - a, dtype=dtype, device="cuda")
        op(piece, a - lo, b - lo, p0, p1, seed=SEED, offset=OFFSET)
        at = r * run_len + (a - rs)
        want[at:at + (b - a)] = piece
        n += b - a
    return want.view(shard.shape), n


@pytest.mark.parametrize("where", ["offsets_past_2_33", "view_past_2_32"])
def test_offsets_beyond_32_bits(where) -> None:
    # A 5 x 7 x 29 shard far out in a 2^35-element tensor. First with the
    # box and the patch both above 2^33 (small view indices), then with the
    # patch starting at element 5 so the VIEW index itself exceeds 2^32.
    geometry = ([5, 7], [1 << 20, 64], 29, (1 << 33) + 3)
    full_numel = 1 << 35
    if where == "offsets_past_2_33":
        lo = (1 << 33) + (1 << 20) + 10
        length = 3 * (1 << 20) + 64 * 3
    else:
        lo = 5
        length = (1 << 33) + 2 * (1 << 20) + 64 * 4 + 9
        assert geometry[3] - lo > 1 << 32
    for dtype in DTYPES:
        for dist in (po.UNIFORM, po.NORMAL):
            shard = torch.full((5, 7, 29), SENTINEL, dtype=dtype,
                               device="cuda")
            want, n = _expected_by_ranges(shard, geometry, lo, length, dist,
                                          dtype)
            assert 0 < n < shard.numel()
            po.call(shard, geometry, full_numel, lo, length, dist,
                    *PARAMS[dist], SEED, OFFSET)
            assert torch.equal(shard, want), (where, dtype, dist)
            assert int((shard == SENTINEL).sum()) == shard.numel() - n


def test_more_than_2_to_the_31_rows_takes_the_64_bit_instantiation() -> None:
    # Every other element of a 2^32-element tensor: 2^31 + 64 rows of one
    # element each (4.3 GB of bf16), so the row index no longer fits the
    # multiply-shift division and the int64 instantiation runs. The patch
    # meets 50 rows next to row 2^31.
    rows = (1 << 31) + 64
    geometry = ([rows], [2], 1, 0)
    lo, length = 2 * (1 << 31) - 10, 100
    shard = torch.full((rows,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    po.call(shard, geometry, 2 * rows, lo, length, po.UNIFORM,
            *PARAMS[po.UNIFORM], SEED, OFFSET)
    view = _view(length, torch.bfloat16, po.UNIFORM)
    first = lo // 2
    assert torch.equal(shard[first:first + 50], view[0::2])
    assert int((shard != SENTINEL).sum()) == 50
    del shard
    torch.cuda.empty_cache()


def test_bad_arguments_raise_and_leave_the_shard_alone() -> None:
    geometry = ([4, 7], [120, 12], 8, 147)  # ends at element 587
    shard = torch.full((4, 7, 8), SENTINEL, device="cuda")

    def call(geometry=geometry, full_numel=720, lo=100, length=300,
             dist=po.NORMAL, p0=0.0, p1=1.0, seed=5, offset=8, shard=shard):
        return torch.ops.tdx.patch_box_(
            shard, geometry[0], geometry[1], geometry[2], geometry[3],
            full_numel, lo, length, dist, p0, p1, seed, offset)

    bad = [
        dict(geometry=([4, 7], [120, 7], 8, 147)),  # overlapping rows
        dict(geometry=([4, 7], [120, 12], 9, 147)),  # numel mismatch
        dict(geometry=([4, 7], [120], 8, 147)),
        dict(full_numel=586),  # the box ends at element 587
        dict(lo=-1),
        dict(length=-1),
        dict(lo=500, length=221),  # ends at 721
        dict(dist=5),
        dict(dist=po.NORMAL, p1=-1.0),
        dict(dist=po.BERNOULLI, p0=1.5),
        dict(dist=po.NORMAL, seed=None),
        dict(dist=po.UNIFORM, offset=None),
        dict(shard=torch.full((4, 7, 8), SENTINEL, device="cuda",
                              dtype=torch.float64)),
    ]
    for kwargs in bad:
        with pytest.raises(RuntimeError):
            call(**kwargs)
            pytest.fail(f"accepted {kwargs}")
    torch.cuda.synchronize()
    assert (shard == SENTINEL).all()
    call()  # the baseline is valid
    torch.cuda.synchronize()
    assert (shard != SENTINEL).any()


# ---- end to end -----------------------------------------------------------


class _Trace(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.names = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(func.name())
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("cast", [False, True], ids=["f32", "to_bf16"])
def test_padded_model_on_the_gpu(cast) -> None:
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import (
        _batched_fill,
        materialize_module,
        materialize_module_batched,
    )
    from torchdistx_amd.models import TINY_PADDED, build_model

    cfg = TINY_PADDED

    def build():
        m = build_model(cfg, device="cuda")
        return m.to(torch.bfloat16) if cast else m

    torch.manual_seed(70)
    m = deferred_init(build)
    w = m.tok_emb.weight
    assert _C.tensor_chain_plan(w) is None
    plan = _C.tensor_patch_plan(w)
    assert [(p["lo"], p["len"]) for p in plan["patches"]] == [
        (cfg.padding_idx * cfg.dim, cfg.dim)]
    n, d, pad = cfg.vocab_size, cfg.dim, cfg.padding_idx
    with _Trace() as tr:
        shards = {
            (dim, a, b): _C.materialize_tensor_shard(w, a, b, dim)
            for dim, a, b in [(0, 0, n // 8), (0, pad, pad + 1),
                              (0, pad + 1, n), (0, 1, n - 1), (1, 0, d // 8),
                              (1, 3, d - 5), (1, d - 1, d)]
        }
        boxes = [[(1, n - 1), (3, d - 5)], [(0, pad + 1), (8, 24)],
                 [(pad, pad + 1), (0, d)], [(pad + 1, n), (1, d)]]
        blocks = [(box, _C.materialize_tensor_block(
            w, [a for a, _ in box], [b for _, b in box])) for box in boxes]
    # The patch op, and no indexing of (or fill on) a full-sized tensor.
    assert "tdx::patch_box_" in tr.names
    assert not any(name.startswith(("aten::select", "aten::fill_",
                                    "aten::slice", "aten::zero_"))
                   for name in tr.names), tr.names

    full = {name: _C.materialize_tensor(t).detach()
            for name, t in m.named_parameters()}
    emb = full["tok_emb.weight"]
    assert emb.dtype == (torch.bfloat16 if cast else torch.float32)
    assert (emb[pad] == 0).all() and (emb[pad + 1] != 0).any()
    for (dim, a, b), shard in shards.items():
        assert torch.equal(shard, emb.narrow(dim, a, b - a)), (dim, a, b)
    for box, block in blocks:
        want = emb[tuple(slice(a, b) for a, b in box)]
        assert torch.equal(block, want), box

    # The batched planner on a twin: the embedding joins the batch, and
    # the result is bitwise the node-by-node replay above.
    torch.manual_seed(70)
    twin = deferred_init(build)
    entries = [
        (sub, key, p, True)
        for sub in twin.modules()
        for key, p in sub._parameters.items()
        if p is not None and _C.can_materialize(p)
    ]
    with _Trace() as tr:
        assert _batched_fill(entries) == []
    assert tr.names.count("tdx::patch_box_") == 1
    for name, p in twin.named_parameters():
        assert torch.equal(p.detach(), full[name]), name

    torch.manual_seed(70)
    a = deferred_init(build)
    torch.manual_seed(70)
    b = deferred_init(build)
    materialize_module_batched(a)
    materialize_module(b)
    for (name, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(pa.detach(), pb.detach()), name
    for (name, ba), (_, bb) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(ba, bb), name
    tokens = torch.randint(0, cfg.vocab_size, (2, 16), device="cuda")
    assert a.loss(tokens).isfinite().item()


def test_retargeting_follows_the_tail_rule() -> None:
    # Tapes recorded for the CPU, materialized straight onto the GPU: a
    # constant or uniform patch retargets with its tensor (same bits on
    # both devices), a normal patch sends the tensor to ordinary replay.
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import _batched_fill

    def build():
        m = torch.nn.Module()
        const = torch.empty(33, 9).uniform_(-1.0, 1.0)
        const[3].zero_()
        const[5, 2:7].uniform_(2.0, 3.0)
        m.const = torch.nn.Parameter(const)
        normal = torch.empty(33, 9).uniform_(-1.0, 1.0)
        normal[3].normal_()
        m.normal = torch.nn.Parameter(normal)
        return m

    torch.manual_seed(72)
    m = deferred_init(build)
    entries = [(m, key, p, True) for key, p in m._parameters.items()]
    fallback = _batched_fill(entries, device="cuda")
    assert [e[1] for e in fallback] == ["normal"]
    assert m.const.is_cuda
    torch.manual_seed(72)
    twin = deferred_init(build)
    native_cpu = _C.native_init_cpu_enabled()
    _C.set_native_init_cpu(True)
    try:
        want = _C.materialize_tensor(twin.const).detach()
    finally:
        _C.set_native_init_cpu(native_cpu)
    assert torch.equal(m.const.detach().cpu(), want)
    assert (want[3] == 0).all() and (want[5, 2:7] >= 2.0).all()


def test_rng_patches_by_parts_on_the_gpu() -> None:
    # A fused weight initialized by parts, and an RNG patch next to a cast:
    # shards, blocks and the batched planner against the full tensor.
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import _batched_fill

    def build():
        m = torch.nn.Module()
        qkv = torch.empty(96, 33, device="cuda", dtype=torch.bfloat16)
        qkv[:64].normal_(std=0.02)
        qkv[64:].normal_(std=0.5)
        m.qkv = torch.nn.Parameter(qkv)
        w = torch.empty(33, 9, device="cuda").uniform_(-1.0, 1.0)
        w[:13].normal_()
        m.cast = torch.nn.Parameter(w.to(torch.float16))
        return m

    torch.manual_seed(71)
    m = deferred_init(build)
    assert len(_C.tensor_patch_plan(m.qkv)["patches"]) == 2
    assert _C.tensor_patch_plan(m.cast) is None
    got = []
    for t in (m.qkv, m.cast):
        rows, cols = t.shape
        for dim, a, b in [(0, 0, rows // 3), (0, rows // 3, rows),
                          (0, 5, rows - 5), (1, 0, cols // 2),
                          (1, cols // 2, cols), (1, 1, 2)]:
            got.append((t, (slice(None),) * dim + (slice(a, b),),
                        _C.materialize_tensor_shard(t, a, b, dim)))
        box = (slice(3, rows - 2), slice(2, cols - 1))
        got.append((t, box, _C.materialize_tensor_block(
            t, [3, 2], [rows - 2, cols - 1])))
    full = {id(t): _C.materialize_tensor(t).detach() for t in (m.qkv, m.cast)}
    for t, index, piece in got:
        assert torch.equal(piece, full[id(t)][index]), index
    assert full[id(m.qkv)][:64].float().std() < 0.1
    assert full[id(m.qkv)][64:].float().std() > 0.3

    torch.manual_seed(71)
    twin = deferred_init(build)
    entries = [(twin, key, p, True) for key, p in twin._parameters.items()]
    fallback = _batched_fill(entries)
    assert [e[1] for e in fallback] == ["cast"]
    assert torch.equal(twin.qkv.detach(), full[id(m.qkv)])
