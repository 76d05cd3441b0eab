# GPU (MI355X) tests of the fused init-chain kernels: an RNG value step
# and its pointwise-scalar tail in one launch must be bitwise what the
# unfused replay (tdx RNG kernel, then one ATen kernel per tail op) gives
# — for whole tensors, any-dim slices and inside the batched launch.
#
# One step is not bitwise: erfinv_ on a float32 tensor. ATen's f32 erfinv
# kernel and the device library's erfinvf differ by 1-2 ulp on about half
# of all inputs (measured on gfx950: 493565 of 1000003 elements), while on
# bf16/fp16 tensors the two agree on every element. So float32 erfinv
# fuses only with the switch explicitly on, and is checked here for
# self-consistency and for accuracy against an fp64 evaluation instead.
# float16 mul_ has a twist of its own, see
# test_f16_arithmetic_follows_aten_block_rounding.

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    os.environ.setdefault("TDX_REQUIRE_NATIVE_INIT", "1")

DTYPES = [torch.float32, torch.bfloat16, torch.float16]

# TailOp codes (csrc/core/deferred_init.h).
ERFINV, MUL, ADD, SUB, CLAMP, CLAMP_MIN, CLAMP_MAX, NEG, ABS = range(9)

SEED, OFFSET = 987654321, 12
STD_SQRT2 = 0.7 * math.sqrt(2.0)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    from torchdistx_amd import _C, _kernels

    assert _kernels.available(), "torchdistx_amd._K must load on a GPU box"
    assert _kernels._K.has_fused_chains()
    fused = _C.fused_init_chains_enabled()
    explicit = _C.fused_init_chains_explicit()
    yield
    if explicit or not fused:
        _C.set_fused_init_chains(fused)
    else:
        _C.reset_fused_init_chains()


def _k_elems(dtype):
    return 4 if dtype == torch.float32 else 8


def _numels(dtype):
    k = _k_elems(dtype)
    return [1, k - 1, k, k + 1, 1_000_003]


def _chain(numel, dtype, dist, p0, p1, ops, s0, s1):
    out = torch.empty(numel, device="cuda", dtype=dtype)
    torch.ops.tdx.rng_chain_(out, dist, p0, p1, ops, s0, s1,
                             seed=SEED, offset=OFFSET)
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_trunc_normal_chain_bitwise(dtype) -> None:
    for numel in _numels(dtype):
        ref = torch.empty(numel, device="cuda", dtype=dtype)
        torch.ops.tdx.uniform_(ref, -0.9, 0.95, seed=SEED, offset=OFFSET)
        ref.erfinv_().mul_(STD_SQRT2).add_(0.1).clamp_(-1.0, 1.5)
        # |u| <= 0.95 keeps erfinv finite.
        assert not ref.isnan().any()
        out = _chain(numel, dtype, 0, -0.9, 0.95,
                     [ERFINV, MUL, ADD, CLAMP],
                     [0.0, STD_SQRT2, 0.1, -1.0], [0.0, 0.0, 0.0, 1.5])
        assert torch.equal(out, ref), (dtype, numel)


def test_f32_erfinv_chain_accuracy() -> None:
    # The unfused f32 chain is the reference for accuracy: against an fp64
    # evaluation of the same chain on the identical uniform draw, the
    # fused result's maximum error may be at most twice the unfused one's
    # (room for a different polynomial, not for a wrong one).
    numel = 1_000_003
    u = torch.empty(numel, device="cuda")
    torch.ops.tdx.uniform_(u, -0.9, 0.95, seed=SEED, offset=OFFSET)
    exact = u.double().erfinv_().mul_(STD_SQRT2).add_(0.1).clamp_(-1.0, 1.5)
    unfused = u.clone().erfinv_().mul_(STD_SQRT2).add_(0.1).clamp_(-1.0, 1.5)
    fused = _chain(numel, torch.float32, 0, -0.9, 0.95,
                   [ERFINV, MUL, ADD, CLAMP],
                   [0.0, STD_SQRT2, 0.1, -1.0], [0.0, 0.0, 0.0, 1.5])
    assert not unfused.isnan().any() and not fused.isnan().any()
    err_unfused = (unfused.double() - exact).abs().max().item()
    err_fused = (fused.double() - exact).abs().max().item()
    print(f"max abs error vs fp64: unfused {err_unfused:.3e}, "
          f"fused {err_fused:.3e}")
    assert err_unfused > 0.0
    assert err_fused <= 2.0 * err_unfused


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_op_chain_bitwise(dtype) -> None:
    """mul -> add on an f32 tensor is the pair a contracting compiler
    would turn into one FMA."""
    for numel in _numels(dtype):
        ref = torch.empty(numel, device="cuda", dtype=dtype)
        torch.ops.tdx.uniform_(ref, -3.0, 5.0, seed=SEED, offset=OFFSET)
        ref.mul_(1.1).add_(-0.3).neg_().abs_().clamp_min_(0.75)
        assert not ref.isnan().any()
        out = _chain(numel, dtype, 0, -3.0, 5.0,
                     [MUL, ADD, NEG, ABS, CLAMP_MIN],
                     [1.1, -0.3, 0.0, 0.0, 0.75], [0.0] * 5)
        assert torch.equal(out, ref), (dtype, numel)


# A tie-maker for f16 values in [4, 8), where f16 steps by 2^-8 and f32
# by 2^-21: x + (2^-9 + 2^-23) lies a quarter of an f32 step above an f16
# tie. Rounded to f32 first it becomes the tie (then to even: down for
# half of all x); rounded to f16 once it always goes up. So the two
# roundings differ on about half of all elements.
F16_TIE_MAKER = 2.0 ** -9 + 2.0 ** -23


@pytest.mark.parametrize(
    "numel", [579, 2048, 3 * 2048 + 579, (1 << 20) + 2047]
)
def test_f16_arithmetic_follows_aten_block_rounding(numel) -> None:
    # ATen's f16 mul/add/sub round the float result to f16 (two
    # roundings), except that mul rounds the exact product once in the
    # block of its elementwise kernel that handles the last numel % 2048
    # elements. The fused kernel follows that from the tensor's element
    # count: below one block every product rounds once, a whole number
    # of blocks never does; add/sub round twice everywhere.
    cases = [
        ([ADD], [F16_TIE_MAKER], lambda t: t.add_(F16_TIE_MAKER)),
        ([SUB], [-F16_TIE_MAKER], lambda t: t.sub_(-F16_TIE_MAKER)),
        ([MUL], [1.1], lambda t: t.mul_(1.1)),
        ([MUL, ADD, SUB], [1.1, F16_TIE_MAKER, 0.3],
         lambda t: t.mul_(1.1).add_(F16_TIE_MAKER).sub_(0.3)),
    ]
    for ops, s0, unfused in cases:
        ref = torch.empty(numel, device="cuda", dtype=torch.float16)
        torch.ops.tdx.uniform_(ref, 4.0, 8.0, seed=SEED, offset=OFFSET)
        unfused(ref)
        out = _chain(numel, torch.float16, 0, 4.0, 8.0, ops, s0,
                     [0.0] * len(ops))
        assert torch.equal(out, ref), (numel, ops)


def test_f16_slices_follow_the_full_tensors_blocks() -> None:
    # A slice's elements round as they do in the FULL tensor (6721 =
    # 3 * 2048 + 577 elements), not as ATen would round the slice alone.
    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import materialize_tensor

    def build():
        m = torch.nn.Module()
        w = torch.empty(13, 517, device="cuda", dtype=torch.float16)
        w.uniform_(4.0, 8.0).add_(F16_TIE_MAKER).mul_(1.1)
        m.w = torch.nn.Parameter(w)
        return m

    torch.manual_seed(51)
    m = deferred_init(build)
    assert len(_C.tensor_chain_plan(m.w)["tail"]) == 2
    cases = [(0, 0, 13), (0, 11, 13), (0, 3, 9), (1, 0, 8), (1, 500, 517)]
    shards = {
        c: _C.materialize_tensor_shard(m.w, c[1], c[2], c[0]) for c in cases
    }
    full = materialize_tensor(m.w).detach()  # unfused replay
    for dim, lo, hi in cases:
        assert torch.equal(
            shards[dim, lo, hi], full.narrow(dim, lo, hi - lo)
        ), (dim, lo, hi)


@pytest.mark.parametrize("dtype", DTYPES)
def test_normal_start_chain_bitwise(dtype) -> None:
    for numel in _numels(dtype):
        ref = torch.empty(numel, device="cuda", dtype=dtype)
        torch.ops.tdx.normal_(ref, 0.2, 1.5, seed=SEED, offset=OFFSET)
        ref.mul_(1.0 / 3.0).sub_(0.7).clamp_(-1.25, 0.5).clamp_max_(0.25)
        assert not ref.isnan().any()
        out = _chain(numel, dtype, 1, 0.2, 1.5,
                     [MUL, SUB, CLAMP, CLAMP_MAX],
                     [1.0 / 3.0, 0.7, -1.25, 0.25], [0.0, 0.0, 0.5, 0.0])
        assert torch.equal(out, ref), (dtype, numel)


def test_infinities_reach_the_clamp_bitwise() -> None:
    # 16-bit uniforms over [-1, 1) hit -1.0 exactly with probability 2^-16
    # per element, so erfinv yields -inf for some of 2^20 elements.
    numel = 1 << 20
    ref = torch.empty(numel, device="cuda", dtype=torch.bfloat16)
    torch.ops.tdx.uniform_(ref, -1.0, 1.0, seed=SEED, offset=OFFSET)
    assert (ref == -1.0).any()
    ref.erfinv_().mul_(0.5).clamp_(-1.0, 1.0)
    assert not ref.isnan().any()
    out = _chain(numel, torch.bfloat16, 0, -1.0, 1.0, [ERFINV, MUL, CLAMP],
                 [0.0, 0.5, -1.0], [0.0, 0.0, 1.0])
    assert torch.equal(out, ref)
    assert out.min().item() == -1.0


def _trunc_module(shape, dtype):
    from torchdistx_amd import deferred_init

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            w = torch.empty(shape, device="cuda", dtype=dtype)
            torch.nn.init.trunc_normal_(w, mean=0.1, std=0.7, a=-1.0, b=1.5)
            self.w = torch.nn.Parameter(w)

    return deferred_init(M)


_TAIL_CODE = {"erfinv": ERFINV, "mul": MUL, "add": ADD, "sub": SUB,
              "clamp": CLAMP, "clamp_min": CLAMP_MIN,
              "clamp_max": CLAMP_MAX, "neg": NEG, "abs": ABS}
_DIST = {"uniform": 0, "normal": 1, "bernoulli": 2}


def _fused_full(plan):
    """The whole tensor of a chain plan through tdx.rng_chain_."""
    out = torch.empty(plan["sizes"], device="cuda", dtype=plan["dtype"])
    torch.ops.tdx.rng_chain_(
        out, _DIST[plan["kind"]], plan["p0"], plan["p1"],
        [_TAIL_CODE[t[0]] for t in plan["tail"]],
        [t[1] for t in plan["tail"]], [t[2] for t in plan["tail"]],
        seed=plan["seed"], offset=plan["offset"])
    return out


def _ranges(n):
    ranges = {(0, 0), (0, n), (0, 1), (n - 1, n), (1, n - 1)}
    if n % 8 == 0 and n > 16:
        ranges.add((8, n - 8))  # group-aligned interior window
    return sorted(ranges)


# (64, 128) is group-aligned (vector path when the range is too);
# (33, 9) and (5, 3, 17) have odd geometry (elementwise path).
@pytest.mark.parametrize("shape", [(64, 128), (33, 9), (5, 3, 17)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_windows_match_unfused_full(shape, dtype) -> None:
    from torchdistx_amd import _C
    from torchdistx_amd.deferred_init import materialize_tensor

    _C.set_fused_init_chains(True)  # explicit: float32 erfinv fuses too
    torch.manual_seed(31)
    m = _trunc_module(shape, dtype)
    plan = _C.tensor_chain_plan(m.w)
    assert [t[0] for t in plan["tail"]] == ["erfinv", "mul", "add", "clamp"]
    cases = [
        (dim, lo, hi)
        for dim in range(len(shape))
        for lo, hi in _ranges(shape[dim])
    ]
    shards = {
        c: _C.materialize_tensor_shard(m.w, c[1], c[2], c[0]) for c in cases
    }
    if dtype == torch.float32:
        # erfinv on float32 is not bitwise vs ATen: the slices must be
        # bitwise sub-tensors of the FUSED whole-tensor op instead.
        full = _fused_full(plan)
    else:
        # Unfused full materialization: node-by-node replay.
        full = materialize_tensor(m.w).detach()
    assert not full.isnan().any()
    for dim, lo, hi in cases:
        assert torch.equal(
            shards[dim, lo, hi], full.narrow(dim, lo, hi - lo)
        ), (dim, lo, hi)


def _mixed_module():
    from torchdistx_amd import deferred_init

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for i, dtype in enumerate(DTYPES):
                w = torch.empty(130, 33, device="cuda", dtype=dtype)
                torch.nn.init.trunc_normal_(w, std=0.02)
                setattr(self, f"trunc{i}", torch.nn.Parameter(w))
            self.big = torch.nn.Parameter(
                torch.nn.init.trunc_normal_(
                    torch.empty(257, 129, device="cuda",
                                dtype=torch.bfloat16),
                    mean=0.1, std=0.7, a=-1.0, b=1.5))
            self.normal = torch.nn.Parameter(
                torch.empty(64, 40, device="cuda").normal_(0.0, 0.3))
            self.scaled = torch.nn.Parameter(
                torch.empty(77, device="cuda").normal_().mul_(3))
            self.fill = torch.nn.Parameter(
                torch.empty(50, device="cuda",
                            dtype=torch.float16).fill_(1.5))
            self.dep = torch.nn.Parameter(
                torch.zeros(9, 5, device="cuda")
                + torch.ones(9, 5, device="cuda"))
            tied = torch.nn.Parameter(
                torch.nn.init.trunc_normal_(
                    torch.empty(32, 16, device="cuda",
                                dtype=torch.bfloat16), std=0.5))
            self.a = torch.nn.Linear(16, 32, bias=False, device="cuda",
                                     dtype=torch.bfloat16)
            self.b = torch.nn.Linear(16, 32, bias=False, device="cuda",
                                     dtype=torch.bfloat16)
            self.a.weight = tied
            self.b.weight = tied

    return deferred_init(M)


def test_batched_fill_fuses_tails() -> None:
    from torchdistx_amd import _C
    from torchdistx_amd.deferred_init import (
        _batched_fill,
        materialize_module,
        materialize_tensor,
    )

    _C.set_fused_init_chains(True)  # explicit: float32 erfinv fuses too
    torch.manual_seed(41)
    ref = _mixed_module()
    # trunc0 is float32 with an erfinv step: its oracle is the fused
    # whole-tensor op (the batched kernel must agree with it bitwise).
    trunc0_full = _fused_full(_C.tensor_chain_plan(ref.trunc0))
    materialize_module(ref)  # unfused replay

    torch.manual_seed(41)
    bat = _mixed_module()
    assert bat.a.weight is bat.b.weight
    entries = [
        (sub, key, p, True)
        for sub in bat.modules()
        for key, p in sub._parameters.items()
        if p is not None and _C.can_materialize(p)
    ]
    fallback = _batched_fill(entries)
    # Only the cross-tensor dependency needs ordinary replay.
    assert [key for _, key, _, _ in fallback] == ["dep"]
    bat._parameters["dep"] = materialize_tensor(fallback[0][2])
    torch.cuda.synchronize()

    names = [n for n, _ in ref.named_parameters()]
    assert names == [n for n, _ in bat.named_parameters()]
    for (name, p_ref), (_, p_bat) in zip(
        ref.named_parameters(), bat.named_parameters()
    ):
        assert not p_ref.isnan().any(), name
        assert p_bat.dtype == p_ref.dtype and p_bat.is_cuda, name
        if name == "trunc0":
            assert torch.equal(trunc0_full, p_bat), name
            # erfinv values stay below 4, where a few ulp are ~1e-6;
            # the chain scales them by 0.02 * sqrt(2).
            assert torch.allclose(p_ref, p_bat, rtol=0, atol=1e-7), name
        else:
            assert torch.equal(p_ref, p_bat), name
    assert bat.a.weight is bat.b.weight
    assert bat.a.weight.data_ptr() == bat.b.weight.data_ptr()
    assert bat.a.weight.shape == (32, 16)


def test_switch_off_sends_tails_to_fallback() -> None:
    from torchdistx_amd import _C
    from torchdistx_amd.deferred_init import _batched_fill

    torch.manual_seed(42)
    f32 = _trunc_module((8, 8), torch.float32)
    bf16 = _trunc_module((8, 8), torch.bfloat16)
    # Default state: float32 erfinv is not fused, bf16 is.
    _C.reset_fused_init_chains()
    if _C.fused_init_chains_enabled() and not _C.fused_init_chains_explicit():
        assert len(_batched_fill([(f32, "w", f32.w, True)])) == 1
        bf16_default = _trunc_module((8, 8), torch.bfloat16)
        assert _batched_fill([(bf16_default, "w", bf16_default.w, True)]) == []
    _C.set_fused_init_chains(False)
    assert len(_batched_fill([(f32, "w", f32.w, True)])) == 1
    assert len(_batched_fill([(bf16, "w", bf16.w, True)])) == 1


def test_trunc_normal_distribution() -> None:
    # Same tolerances as the statistics tests in tests/test_gpu.py.
    from torchdistx_amd import deferred_init
    from torchdistx_amd.deferred_init import materialize_module_batched

    def build():
        m = torch.nn.Module()
        w = torch.empty(1 << 22, device="cuda")
        torch.nn.init.trunc_normal_(w, std=1.0, a=-2.0, b=2.0)
        m.w = torch.nn.Parameter(w)
        return m

    from torchdistx_amd import _C

    _C.set_fused_init_chains(True)  # float32 erfinv through the fused path
    torch.manual_seed(43)
    m = deferred_init(build)
    assert _C.tensor_chain_plan(m.w)["tail"]
    materialize_module_batched(m)
    f = m.w.detach().float()
    assert f.min().item() >= -2.0 and f.max().item() <= 2.0
    assert f.mean().item() == pytest.approx(0.0, abs=0.02)
    # Standard deviation of a normal truncated at +-2 sigma.
    assert f.std().item() == pytest.approx(0.8796, rel=0.02)
