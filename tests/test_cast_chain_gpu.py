# GPU (MI355X) tests of the cast-chain kernels: an RNG value step, its
# pointwise tail and ONE dtype conversion in a single launch
# (tdx::rng_chain_cast_ / rng_chain_cast_shard_win_ and the second launch
# of the batched planner) must be bitwise what the separate kernels give —
# the RNG (or fused chain) op at the source dtype, then `.to(dst)`.

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    os.environ.setdefault("TDX_REQUIRE_NATIVE_INIT", "1")

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAIRS = [(s, d) for s in (F32, BF16, F16) for d in (F32, BF16, F16) if s != d]
_PAIR_IDS = [f"{s}-{d}".replace("torch.", "") for s, d in PAIRS]

# TailOp codes (csrc/core/deferred_init.h).
ERFINV, MUL, ADD, SUB, CLAMP, CLAMP_MIN, CLAMP_MAX, NEG, ABS = range(9)

SEED, OFFSET = 987654321, 12
STD_SQRT2 = 0.7 * math.sqrt(2.0)
NO_TAIL = ([], [], [])
MUL_ADD = ([MUL, ADD], [1.1, -0.3], [0.0, 0.0])
TRUNC = ([ERFINV, MUL, ADD, CLAMP], [0.0, STD_SQRT2, 0.1, -1.0],
         [0.0, 0.0, 0.0, 1.5])

# A partial unit inside the first (1, 3) and the second (5, 7) f32 group,
# an exact group and unit (4, 8), one past (9, 13), ATen's f16 block of
# 2048, the batched virtual block of 16384 (+4: half a unit), many blocks.
NUMELS = [1, 3, 4, 5, 7, 8, 9, 13, 2048, 2048 + 5, 16384, 16384 + 4,
          1_000_003]

DISTS = {"uniform": (0, -0.9, 0.95), "normal": (1, 0.2, 1.5),
         "bernoulli": (2, 0.3, 0.0)}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from torchdistx_amd import _C, _kernels

    assert _kernels.available(), "torchdistx_amd._K must load on a GPU box"
    assert _kernels._K.has_cast_chains()
    fused = _C.fused_init_chains_enabled()
    explicit = _C.fused_init_chains_explicit()
    yield
    if explicit or not fused:
        _C.set_fused_init_chains(fused)
    else:
        _C.reset_fused_init_chains()


def _source(numel, src, dist, p0, p1, tail, device="cuda"):
    """The oracle before its `.to(dst)`: the plain RNG op when there is no
    tail, tdx.rng_chain_ otherwise, at the source dtype."""
    ref = torch.empty(numel, device=device, dtype=src)
    if tail[0]:
        torch.ops.tdx.rng_chain_(ref, dist, p0, p1, *tail, seed=SEED,
                                 offset=OFFSET)
    elif dist == 0:
        torch.ops.tdx.uniform_(ref, p0, p1, seed=SEED, offset=OFFSET)
    elif dist == 1:
        torch.ops.tdx.normal_(ref, p0, p1, seed=SEED, offset=OFFSET)
    else:
        torch.ops.tdx.bernoulli_(ref, p0, seed=SEED, offset=OFFSET)
    assert not ref.isnan().any()
    return ref


def _cast(numel, src, dst, dist, p0, p1, tail, device="cuda"):
    out = torch.empty(numel, device=device, dtype=dst)
    torch.ops.tdx.rng_chain_cast_(out, src, dist, p0, p1, *tail, seed=SEED,
                                  offset=OFFSET)
    return out


# ---- whole-tensor op ----------------------------------------------------------


@pytest.mark.parametrize("dist", sorted(DISTS))
@pytest.mark.parametrize("pair", PAIRS, ids=_PAIR_IDS)
def test_cast_op_equals_source_op_then_to(pair, dist) -> None:
    src, dst = pair
    code, p0, p1 = DISTS[dist]
    for numel in NUMELS:
        want = _source(numel, src, code, p0, p1, NO_TAIL).to(dst)
        out = _cast(numel, src, dst, code, p0, p1, NO_TAIL)
        assert out.dtype == dst
        assert torch.equal(out, want), (numel,)


@pytest.mark.parametrize("dst", [BF16, F16])
def test_f32_mul_add_tail_is_not_contracted(dst) -> None:
    """mul -> add on an f32 source is the pair a contracting compiler
    would turn into one FMA; the unfused kernels round twice."""
    for code, p0, p1 in ((0, -3.0, 5.0), (1, 0.2, 1.5)):
        for numel in NUMELS:
            want = _source(numel, F32, code, p0, p1, MUL_ADD).to(dst)
            out = _cast(numel, F32, dst, code, p0, p1, MUL_ADD)
            assert torch.equal(out, want), (code, numel)
        # The oracle's oracle, once: rng_chain_ itself against ATen.
        ref = torch.empty(2053, device="cuda")
        torch.ops.tdx.uniform_(ref, -3.0, 5.0, seed=SEED, offset=OFFSET)
        ref.mul_(1.1).add_(-0.3)
        assert torch.equal(_cast(2053, F32, dst, 0, -3.0, 5.0, MUL_ADD),
                           ref.to(dst))


@pytest.mark.parametrize(
    "pair", [p for p in PAIRS if p[0] != F32],
    ids=[i for i, p in zip(_PAIR_IDS, PAIRS) if p[0] != F32])
def test_trunc_chain_at_a_16_bit_source(pair) -> None:
    src, dst = pair
    for numel in NUMELS:
        ref = torch.empty(numel, device="cuda", dtype=src)
        torch.ops.tdx.uniform_(ref, -0.9, 0.95, seed=SEED, offset=OFFSET)
        ref.erfinv_().mul_(STD_SQRT2).add_(0.1).clamp_(-1.0, 1.5)
        # |u| <= 0.95 keeps erfinv finite.
        assert not ref.isnan().any()
        out = _cast(numel, src, dst, 0, -0.9, 0.95, TRUNC)
        assert torch.equal(out, ref.to(dst)), (numel,)


# tests/test_fused_chain_gpu.py: x + F16_TIE_MAKER lies a quarter of an f32
# step above an f16 tie for f16 x in [4, 8).
F16_TIE_MAKER = 2.0 ** -9 + 2.0 ** -23


def test_f16_source_follows_atens_block_rounding() -> None:
    # ATen's f16 mul rounds the exact product once in the block that
    # handles the last numel % 2048 elements and twice elsewhere; the cast
    # kernel applies the tail at the SOURCE dtype, so it must place that
    # block by the full tensor's element count before converting.
    numel = 3 * 2048 + 579
    tail = ([MUL, ADD, SUB], [1.1, F16_TIE_MAKER, 0.3], [0.0] * 3)
    ref = torch.empty(numel, device="cuda", dtype=F16)
    torch.ops.tdx.uniform_(ref, 4.0, 8.0, seed=SEED, offset=OFFSET)
    ref.mul_(1.1).add_(F16_TIE_MAKER).sub_(0.3)
    for dst in (BF16, F32):
        out = _cast(numel, F16, dst, 0, 4.0, 8.0, tail)
        assert torch.equal(out, ref.to(dst)), dst
    # A window of it rounds as the FULL tensor does.
    lo, hi = 2 * 2048 + 8, numel
    win = torch.empty(hi - lo, device="cuda", dtype=BF16)
    torch.ops.tdx.rng_chain_cast_shard_win_(
        win, F16, 1, hi - lo, hi - lo, lo, 0, 4.0, 8.0, *tail, numel,
        seed=SEED, offset=OFFSET)
    assert torch.equal(win, ref[lo:hi].to(BF16))


# ---- windowed op --------------------------------------------------------------


def _window(whole, src, lo, hi, tail, out=None):
    rows, cols = whole.shape
    if out is None:
        out = torch.empty(rows, hi - lo, device="cuda", dtype=whole.dtype)
    torch.ops.tdx.rng_chain_cast_shard_win_(
        out, src, rows, hi - lo, cols, lo, 1, 0.2, 1.5, *tail, rows * cols,
        seed=SEED, offset=OFFSET)
    return out


@pytest.mark.parametrize("pair", PAIRS, ids=_PAIR_IDS)
def test_windows_are_slices_of_the_whole_tensor(pair) -> None:
    src, dst = pair
    tail = MUL_ADD
    geometries = {
        # (rows, cols): [(lo, hi)] along dim 1
        (64, 128): [
            (0, 128),   # everything, unit-aligned: vector path
            (8, 120),   # unit-aligned interior window: vector path
            (4, 124),   # g_off % 8 == 4: group- but not unit-aligned (f32)
            (4, 12),    # the same, one unit long
            (3, 100),   # odd offset
        ],
        (33, 9): [(0, 9), (1, 8), (8, 9)],   # odd block_len and stride
        (20, 36): [(0, 16), (8, 32)],        # g_stride % 8 == 4
        (3, 1000): [(0, 997), (16, 23)],     # blocks that are no unit multiple
    }
    for (rows, cols), windows in geometries.items():
        whole = _cast(rows * cols, src, dst, 1, 0.2, 1.5, tail)
        want = _source(rows * cols, src, 1, 0.2, 1.5, tail).to(dst)
        assert torch.equal(whole, want)
        whole = whole.view(rows, cols)
        for lo, hi in windows:
            got = _window(whole, src, lo, hi, tail)
            assert torch.equal(got, whole[:, lo:hi]), (rows, cols, lo, hi)
    # Flat ranges (n_blocks == 1, the dim-0 case): a partial last unit on
    # the vector path, and starts inside a unit.
    n = 4099
    flat = _cast(n, src, dst, 1, 0.2, 1.5, tail)
    for start, end in [(0, 4099), (8, 4099), (8, 21), (4, 4096), (4, 11),
                       (3, 4099), (4088, 4099), (16, 16)]:
        out = torch.empty(end - start, device="cuda", dtype=dst)
        torch.ops.tdx.rng_chain_cast_shard_win_(
            out, src, 1, end - start, end - start, start, 1, 0.2, 1.5,
            *tail, n, seed=SEED, offset=OFFSET)
        assert torch.equal(out, flat[start:end]), (start, end)


@pytest.mark.parametrize("pair", PAIRS, ids=_PAIR_IDS)
def test_misaligned_output_takes_the_elementwise_path(pair) -> None:
    src, dst = pair
    rows, cols = 16, 64
    whole = _cast(rows * cols, src, dst, 1, 0.2, 1.5, NO_TAIL).view(rows, cols)
    # A view one element into a larger buffer: not 16-byte aligned.
    buf = torch.full((rows * 48 + 1,), 7.0, device="cuda", dtype=dst)
    out = buf[1:].view(rows, 48)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    _window(whole, src, 8, 56, NO_TAIL, out=out)
    assert torch.equal(out, whole[:, 8:56])
    assert buf[0].item() == 7.0


def test_shard_past_2_to_the_31_elements() -> None:
    # 64-bit shard index path: bf16 -> f16 uniform, 2^31 + 8 elements.
    n = (1 << 31) + 8
    g_off = 8
    full_numel = n + 2 * g_off
    out = torch.empty(n, device="cuda", dtype=F16)
    torch.ops.tdx.rng_chain_cast_shard_win_(
        out, BF16, 1, n, n, g_off, 0, -1.0, 1.0, [], [], [], full_numel,
        seed=SEED, offset=OFFSET)
    ref = torch.empty(n, device="cuda", dtype=BF16)
    torch.ops.tdx.uniform_shard_(ref, g_off, g_off + n, -1.0, 1.0, seed=SEED,
                                 offset=OFFSET)
    ref = ref.to(F16)
    assert torch.equal(out, ref)
    assert out[-8:].float().abs().sum().item() > 0.0
    del out, ref
    torch.cuda.empty_cache()


# ---- cross-device -------------------------------------------------------------


@pytest.mark.parametrize("dist", ["uniform", "bernoulli"])
@pytest.mark.parametrize("pair", PAIRS, ids=_PAIR_IDS)
def test_gpu_op_equals_the_cpu_twin(pair, dist) -> None:
    # The project's device-independence claim covers uniform and bernoulli
    # (normals use each device's transcendentals).
    src, dst = pair
    code, p0, p1 = DISTS[dist]
    for numel in (13, 2053, 16384 + 4):
        gpu = _cast(numel, src, dst, code, p0, p1, NO_TAIL)
        cpu = _cast(numel, src, dst, code, p0, p1, NO_TAIL, device="cpu")
        assert torch.equal(gpu.cpu(), cpu), (numel,)


# ---- batched planner ----------------------------------------------------------


def _mixed_module():
    from torchdistx_amd import deferred_init

    def trunc(shape, dtype):
        w = torch.empty(shape, device="cuda", dtype=dtype)
        return torch.nn.init.trunc_normal_(w, mean=0.1, std=0.7, a=-1.0,
                                           b=1.5)

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            P = torch.nn.Parameter
            dev = "cuda"
            self.cast_n = P(torch.empty(257, 129, device=dev)
                            .normal_(0.0, 0.02).to(BF16))
            self.cast_u = P(torch.empty(1000, device=dev, dtype=BF16)
                            .uniform_(-1.0, 1.0).to(F32))
            self.cast_b = P(torch.empty(16384 + 4, device=dev)
                            .bernoulli_(0.3).to(F16))
            self.cast_big = P(torch.empty(3, 16384 + 13, device=dev,
                                          dtype=F16).normal_().to(F32))
            self.cast_trunc = P(trunc((300, 70), F16).to(BF16))
            self.cast_scaled = P(torch.empty(77, device=dev).normal_()
                                 .mul_(3).add_(0.5).to(BF16))
            self.plain = P(torch.empty(64, 40, device=dev).normal_(0.0, 0.3))
            self.plain_trunc = P(trunc((257, 129), BF16))
            self.fill = P(torch.empty(50, device=dev).fill_(0.37).to(BF16))
            self.zero = P(torch.zeros(9, 5, device=dev).to(F16))
            self.lin = torch.nn.Linear(40, 24, device=dev).bfloat16()
            tied = P(torch.empty(32, 16, device=dev).normal_().to(BF16))
            self.a = torch.nn.Linear(16, 32, bias=False, device=dev,
                                     dtype=BF16)
            self.b = torch.nn.Linear(16, 32, bias=False, device=dev,
                                     dtype=BF16)
            self.a.weight = tied
            self.b.weight = tied

    return deferred_init(M)


def test_batched_fill_takes_every_cast_parameter() -> None:
    from torchdistx_amd import _C
    from torchdistx_amd.deferred_init import (
        _batched_fill,
        materialize_module,
        materialize_module_batched,
    )

    _C.reset_fused_init_chains()
    torch.manual_seed(41)
    ref = _mixed_module()
    materialize_module(ref)  # node-by-node replay

    torch.manual_seed(41)
    bat = _mixed_module()
    assert bat.a.weight is bat.b.weight
    for name in ("cast_n", "cast_u", "cast_b", "cast_big", "cast_trunc",
                 "cast_scaled"):
        plan = _C.tensor_chain_plan(getattr(bat, name))
        assert plan is not None and plan["src_dtype"] is not None, name
    assert _C.tensor_chain_plan(bat.lin.weight)["src_dtype"] == F32
    assert _C.tensor_chain_plan(bat.plain)["src_dtype"] is None
    entries = [
        (sub, key, p, True)
        for sub in bat.modules()
        for key, p in sub._parameters.items()
        if p is not None and _C.can_materialize(p)
    ]
    assert _batched_fill(entries) == []
    torch.cuda.synchronize()

    torch.manual_seed(41)
    pub = _mixed_module()
    materialize_module_batched(pub)

    names = [n for n, _ in ref.named_parameters()]
    for other in (bat, pub):
        assert names == [n for n, _ in other.named_parameters()]
        for (name, p_ref), (_, p) in zip(
            ref.named_parameters(), other.named_parameters()
        ):
            assert not p_ref.isnan().any(), name
            assert p.dtype == p_ref.dtype and p.is_cuda, name
            assert p.requires_grad == p_ref.requires_grad
            assert torch.equal(p_ref, p), name
        assert other.a.weight is other.b.weight
        assert other.a.weight.dtype == BF16


def test_batched_call_without_src_dtypes_is_the_old_call() -> None:
    # None, a list of Nones and no argument at all are one and the same
    # launch; a src_dtype on a fill is refused.
    from torchdistx_amd import _kernels

    K = _kernels._K
    outs = []
    for extra in ((), ([[]], [[]], [[]], None), ([[]], [[]], [[]], [None])):
        t = torch.empty(16384 + 5, device="cuda", dtype=BF16)
        K.batched_init_([t], [1], [0.0], [1.0], [SEED], [OFFSET], *extra)
        outs.append(t)
    want = torch.empty(16384 + 5, device="cuda", dtype=BF16)
    torch.ops.tdx.normal_(want, 0.0, 1.0, seed=SEED, offset=OFFSET)
    for t in outs:
        assert torch.equal(t, want)
    both = [torch.empty(16384 + 5, device="cuda", dtype=BF16) for _ in "ab"]
    K.batched_init_(both, [1, 1], [0.0, 0.0], [1.0, 1.0], [SEED, SEED],
                    [OFFSET, OFFSET], [[], []], [[], []], [[], []],
                    [None, F32])
    assert torch.equal(both[0], want)
    assert torch.equal(both[1], _cast(16384 + 5, F32, BF16, 1, 0.0, 1.0,
                                      NO_TAIL))
    with pytest.raises(RuntimeError, match="only RNG plans"):
        K.batched_init_([both[0]], [3], [1.0], [0.0], [0], [0], [[]], [[]],
                        [[]], [F32])
    with pytest.raises(RuntimeError, match="two different"):
        K.batched_init_([both[0]], [1], [0.0], [1.0], [0], [4], [[]], [[]],
                        [[]], [BF16])
    # A refused batch fills nothing: the conversion part is checked before
    # the conversion-free part launches.
    both[0].fill_(7.0)
    with pytest.raises(RuntimeError, match="two different"):
        K.batched_init_(both, [1, 1], [0.0, 0.0], [1.0, 1.0], [SEED, SEED],
                        [OFFSET, OFFSET], [[], []], [[], []], [[], []],
                        [None, BF16])
    torch.cuda.synchronize()
    assert (both[0] == 7.0).all()


# ---- end to end -----------------------------------------------------------------


def test_tiny_model_converted_in_the_builder() -> None:
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import (
        _batched_fill,
        materialize_module,
    )
    from torchdistx_amd.models import TINY, build_model
    from torchdistx_amd.parallel import (
        materialize_tensor_block,
        materialize_tensor_shard,
    )

    def build():
        return build_model(TINY, device="cuda").to(BF16)

    torch.manual_seed(50)
    m = deferred_init(build)
    shards, blocks = {}, {}
    n_cast = 0
    for name, p in m.named_parameters():
        assert p.dtype == BF16
        plan = _C.tensor_chain_plan(p)
        n_cast += plan is not None and plan["src_dtype"] is not None
        for dim in range(min(p.dim(), 2)):
            n = p.shape[dim]
            for lo, hi in {(0, n // 2), (n // 2, n), (1, n - 1)}:
                # The raw binding: a parameter that is no simple chain
                # would raise here instead of falling back.
                shards[name, dim, lo, hi] = _C.materialize_tensor_shard(
                    p, lo, hi, dim)
        box = [(1, n - 1) if n > 2 else (0, n) for n in p.shape]
        blocks[name] = (box, _C.materialize_tensor_block(
            p, [lo for lo, _ in box], [hi for _, hi in box]))
    assert n_cast > 0
    for name, b in m.named_buffers():
        if b.dim() == 0:
            continue
        n = b.shape[0]
        shards[name, 0, 0, n // 2] = materialize_tensor_shard(b, 0, n // 2, 0)
    tensors = dict(m.named_parameters())
    tensors.update(dict(m.named_buffers()))
    full = {
        n: _C.materialize_tensor(t).detach() for n, t in tensors.items()
    }
    for (name, dim, lo, hi), shard in shards.items():
        want = full[name].narrow(dim, lo, hi - lo)
        assert shard.dtype == want.dtype
        assert torch.equal(shard.detach(), want), (name, dim, lo, hi)
    for name, (box, block) in blocks.items():
        want = full[name][tuple(slice(lo, hi) for lo, hi in box)]
        assert torch.equal(block, want), (name, box)
    assert not any(t.float().isnan().any() for t in full.values())

    # The batched planner on a twin: no cast parameter in the fallback,
    # bitwise the node-by-node replay above.
    torch.manual_seed(50)
    twin = deferred_init(build)
    entries = [
        (sub, key, p, True)
        for sub in twin.modules()
        for key, p in sub._parameters.items()
        if p is not None and _C.can_materialize(p)
    ]
    assert _batched_fill(entries) == []
    for name, p in twin.named_parameters():
        assert torch.equal(p.detach(), full[name]), name
    materialize_module(twin, buffers_only=True)
    tokens = torch.randint(0, TINY.vocab_size, (2, 16), device="cuda")
    assert twin.loss(tokens).isfinite().item()


# ---- memory ---------------------------------------------------------------------


def test_no_full_precision_copy_is_allocated() -> None:
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import materialize_module_batched

    rows, cols = 2048, 2048
    numel = rows * cols  # 2^22
    mib = 1 << 20

    def build():
        m = torch.nn.Module()
        m.w = torch.nn.Parameter(
            torch.empty(rows, cols, device="cuda").normal_(0.0, 0.02)
            .to(BF16))
        return m

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    torch.manual_seed(60)
    m = deferred_init(build)
    # A bf16 tensor is 2 bytes per element; the parent commit's replay held
    # the f32 source (4) next to it.
    peak, _ = peak_of(lambda: materialize_module_batched(m))
    print(f"batched: peak {peak} bytes for {numel} elements")
    assert m.w.dtype == BF16 and m.w.is_cuda
    assert peak < 2 * numel + mib

    torch.manual_seed(60)
    m2 = deferred_init(build)
    for fused in (True, False):
        _C.set_fused_init_chains(fused)
        peak, shard = peak_of(
            lambda: _C.materialize_tensor_shard(m2.w, 0, rows // 2, 0))
        print(f"shard (fused={fused}): peak {peak} bytes")
        # Unfused: half the tensor at f32 plus its bf16 conversion.
        assert peak < numel * (4 // 2 + 2 // 2) + mib
        if fused:
            assert peak < numel * (2 // 2) + mib
        assert torch.equal(shard, m.w.detach()[: rows // 2])
        del shard
