# GPU (MI355X) tests of N-d block materialization: the rng_box_ kernel
# must produce, for any box, bitwise the matching block of a full
# materialization of the same tape — on its group-indexed vector path, on
# its elementwise path, with and without a fused tail, and on the 64-bit
# index path.

import os

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    os.environ.setdefault("TDX_REQUIRE_NATIVE_INIT", "1")

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from torchdistx_amd import _kernels

    assert _kernels.available(), "torchdistx_amd._K must load on a GPU box"
    assert _kernels._K.has_box_kernel()


def _init(kind, shape, dtype):
    w = torch.empty(shape, dtype=dtype, device="cuda")
    if kind == "uniform":
        w.uniform_(-0.5, 1.5)
    elif kind == "normal":
        w.normal_(0.1, 0.8)
    elif kind == "bernoulli":
        w.bernoulli_(0.3)
    else:
        # erfinv_ on float32 fuses only on explicit request; the switch
        # stays at its default here, so that chain runs step by step
        # behind the box op while the 16-bit ones fuse.
        torch.nn.init.trunc_normal_(w, mean=0.1, std=0.7, a=-1.0, b=1.5)
    return w


def _deferred(kind, shape, dtype):
    from torchdistx_amd import deferred_init

    def build():
        m = torch.nn.Module()
        m.w = torch.nn.Parameter(_init(kind, shape, dtype))
        return m

    return deferred_init(build)


def _block(t, box):
    from torchdistx_amd import _C

    return _C.materialize_tensor_block(
        t, [lo for lo, _ in box], [hi for _, hi in box]
    )


def _index(box):
    return tuple(slice(lo, hi) for lo, hi in box)


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


# (shape, box): which path the kernel takes is a matter of the geometry —
# g_off, run_len and every stride must be multiples of the 16-byte group
# (4 x f32, 8 x bf16/f16) for the vector path.
CASES = {
    # run 32, g_off 1288, strides 1024 / 64: vector path for all dtypes.
    "aligned": ((6, 16, 64), [(1, 5), (4, 12), (8, 40)]),
    # g_off 1284 = 4 * 321: vector for f32, elementwise for 16-bit.
    "aligned_f32_only": ((6, 16, 64), [(1, 5), (4, 12), (4, 36)]),
    # Odd everything: elementwise for all dtypes.
    "odd": ((5, 7, 29), [(1, 4), (2, 6), (3, 20)]),
    # Every dim partial: four levels over runs of 8 (g_off 2532: vector for
    # f32 only) ...
    "four_levels": ((3, 4, 5, 6, 16),
                    [(1, 3), (1, 4), (1, 4), (2, 5), (4, 12)]),
    # ... and four levels on the vector path for every dtype.
    "four_levels_aligned": ((3, 4, 5, 6, 16),
                            [(1, 3), (1, 4), (1, 4), (2, 5), (8, 16)]),
    # Single row, single column, and a box that ends with the tensor.
    "row": ((6, 16, 64), [(2, 3), (4, 12), (8, 40)]),
    "col": ((6, 16, 64), [(1, 5), (4, 12), (63, 64)]),
    "to_the_end": ((5, 7, 29), [(2, 5), (3, 7), (11, 29)]),
}


@pytest.mark.parametrize("kind", ["uniform", "normal", "bernoulli", "trunc"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_blocks_are_bitwise_blocks_of_the_full_tensor(case, kind) -> None:
    from torchdistx_amd import _C

    shape, box = CASES[case]
    for dtype in DTYPES:
        torch.manual_seed(61)
        m = _deferred(kind, shape, dtype)
        names = _traced(lambda: _block(m.w, box))
        block = _block(m.w, box)
        full = _C.materialize_tensor(m.w).detach()
        assert not full.isnan().any()
        want = full[_index(box)]
        assert block.shape == want.shape and block.is_contiguous()
        assert torch.equal(block, want), (case, kind, dtype)
        if case != "row":  # a single row of a 3-d tensor is one level
            assert names[0] == "tdx::rng_box_", names
            fuses = kind != "trunc" or dtype != torch.float32
            assert len(names) == (1 if fuses else 5), names


def test_full_middle_dim_takes_the_window_op() -> None:
    from torchdistx_amd import _C

    box = [(1, 5), (0, 16), (8, 40)]
    for dtype in DTYPES:
        torch.manual_seed(62)
        m = _deferred("uniform", (6, 16, 64), dtype)
        assert _traced(lambda: _block(m.w, box)) == [
            "tdx::uniform_shard_win_"]
        block = _block(m.w, box)
        full = _C.materialize_tensor(m.w).detach()
        assert torch.equal(block, full[_index(box)])


def test_more_than_one_trip_of_the_grid_stride_loop() -> None:
    # 66.7M bf16 elements = 8.3M groups, twice the 16384 x 256 threads of
    # the largest grid: every thread takes two or three groups. Runs of
    # 4088 = 511 * 8 elements keep it on the vector path.
    from torchdistx_amd import _C

    shape = (4, 4096, 4096)
    box = [(0, 4), (8, 4088), (0, 4088)]
    torch.manual_seed(63)
    m = _deferred("normal", shape, torch.bfloat16)
    assert _traced(lambda: _block(m.w, box)) == ["tdx::rng_box_"]
    # The same box one column to the right takes the elementwise path.
    shifted = box[:2] + [(1, 4089)]
    blocks = [(b, _block(m.w, b)) for b in (box, shifted)]
    full = _C.materialize_tensor(m.w).detach()
    for b, block in blocks:
        assert torch.equal(block, full[_index(b)]), b


# See test_fused_chain_gpu.py: x + (2^-9 + 2^-23) makes the once-rounded
# and the twice-rounded f16 product differ on about half of all x.
F16_TIE_MAKER = 2.0 ** -9 + 2.0 ** -23


def test_f16_box_follows_the_full_tensors_last_block() -> None:
    # ATen's f16 mul_ rounds once in the last numel % 2048 elements of the
    # FULL tensor (13 * 11 * 47 = 6721 = 3 * 2048 + 577): the box starts
    # at element 2682 and ends at 6620, so it straddles element 6144 and
    # must switch rounding there — where the full tensor does, not where
    # a tensor of the box's own 2072 elements would (its last 24).
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import materialize_tensor

    def build():
        m = torch.nn.Module()
        w = torch.empty(13, 11, 47, device="cuda", dtype=torch.float16)
        w.uniform_(4.0, 8.0).add_(F16_TIE_MAKER).mul_(1.1)
        m.w = torch.nn.Parameter(w)
        return m

    torch.manual_seed(64)
    m = deferred_init(build)
    assert len(_C.tensor_chain_plan(m.w)["tail"]) == 2
    box = [(5, 13), (2, 9), (3, 40)]
    assert _traced(lambda: _block(m.w, box)) == ["tdx::rng_box_"]
    block = _block(m.w, box)
    full = materialize_tensor(m.w).detach()
    assert torch.equal(block, full[_index(box)])
    # Both sides of the full tensor's boundary are in the box.
    flat_pos = torch.arange(6721, device="cuda").view(13, 11, 47)[_index(box)]
    assert (flat_pos < 6144).any() and (flat_pos >= 6144).any()


def test_box_64bit_index_path() -> None:
    # Boxes above 2^31 elements take the int64 instantiation (plain
    # division); the aligned vector path and the elementwise path must
    # both stay bitwise blocks of the full tensor. (~10 GB HBM in all.)
    from torchdistx_amd import _C

    shape = (3, 26000, 36000)  # 2.81e9 elements, 5.6 GB of bf16
    torch.manual_seed(65)
    m = _deferred("normal", shape, torch.bfloat16)
    full = _C.materialize_tensor(m.w).detach()
    torch.manual_seed(65)
    part = _deferred("normal", shape, torch.bfloat16)
    box = [(0, 3), (0, 24000), (0, 30000)]  # 2.16e9 elements, aligned
    assert _traced(lambda: _block(part.w, [(0, 3), (0, 2), (0, 8)])) == [
        "tdx::rng_box_"]
    s = _block(part.w, box)
    assert s.numel() > 2**31
    assert torch.equal(s, full[_index(box)])
    del s
    box[2] = (1, 30001)  # unaligned: elementwise
    s2 = _block(part.w, box)
    assert s2.numel() > 2**31
    assert torch.equal(s2, full[_index(box)])
    del s2, full, part, m
    torch.cuda.empty_cache()


def test_box_op_rejects_bad_geometry_on_gpu() -> None:
    out = torch.empty(4, 7, 8, device="cuda")
    with pytest.raises(RuntimeError):  # ends at element 587
        torch.ops.tdx.rng_box_(out, [4, 7], [120, 12], 8, 147, 0, 0.0, 1.0,
                               [], [], [], 586, 5, 8)
    with pytest.raises(RuntimeError):  # numel mismatch
        torch.ops.tdx.rng_box_(out, [4, 7], [120, 12], 9, 147, 0, 0.0, 1.0,
                               [], [], [], 720, 5, 8)
    with pytest.raises(RuntimeError):  # overlapping rows
        torch.ops.tdx.rng_box_(out, [4, 7], [120, 7], 8, 147, 0, 0.0, 1.0,
                               [], [], [], 720, 5, 8)
    empty = torch.empty(0, 7, 8, device="cuda")
    assert torch.ops.tdx.rng_box_(empty, [0, 7], [120, 12], 8, 147, 0, 0.0,
                                  1.0, [], [], [], 720, 5, 8) is empty
