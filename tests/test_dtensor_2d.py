# materialize_module_dtensor over a 2-D device mesh: 4 gloo processes on a
# (2, 2) mesh. Every rank materializes only its N-d block, and the
# resulting DTensors must be bitwise what distribute_tensor makes of a
# full materialization of the same tape.

import pytest
import torch

from tests._dist_utils import run_distributed

# name -> (shape, dtype, placements as ("S", dim) / "R" per mesh dim).
# Sizes 3 and 1 give uneven and empty chunks; "experts" is a stacked
# [E, out, in] weight whose block is a two-level box.
_SPECS = {
    "both": ((6, 10), torch.float32, (("S", 0), ("S", 1))),
    "nested": ((3, 8), torch.float32, (("S", 0), ("S", 0))),
    "tp_only": ((5, 3), torch.bfloat16, ("R", ("S", 1))),
    "dp_only": ((3, 4), torch.float16, (("S", 0), "R")),
    "experts": ((4, 6, 8), torch.bfloat16, (("S", 1), ("S", 2))),
    "tiny": ((1, 5), torch.float32, (("S", 0), ("S", 0))),
    "neg_dim": ((4, 3), torch.float32, (("S", -1), ("S", -2))),
    "default": ((7, 4), torch.float32, None),
    "scalar": ((), torch.float32, None),
    "replicated": ((4, 4), torch.float32, ("R", "R")),
}


def _build():
    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for name, (shape, dtype, _) in _SPECS.items():
                t = torch.empty(shape, dtype=dtype)
                if name == "experts":
                    torch.nn.init.trunc_normal_(t, std=0.5, a=-1.0, b=1.0)
                elif name == "dp_only":
                    t.uniform_(-1.0, 1.0)
                else:
                    t.normal_()
                setattr(self, name, torch.nn.Parameter(t))
            self.register_buffer("mask", torch.empty(3, 6).bernoulli_(0.5))

    return M()


def _placements(spec):
    from torch.distributed.tensor import Replicate, Shard

    return [Replicate() if p == "R" else Shard(p[1]) for p in spec]


def _worker(rank, world):
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import Replicate, Shard, distribute_tensor
    from torch.distributed.tensor.placement_types import _StridedShard

    from torchdistx_amd import _C, deferred_init
    from torchdistx_amd.deferred_init import materialize_module
    from torchdistx_amd.parallel import materialize_module_dtensor

    _C.set_native_init_cpu(True)
    try:
        mesh = init_device_mesh("cpu", (2, 2), mesh_dim_names=("dp", "tp"))
        shard_dims = {
            name: _placements(spec)
            for name, (_, _, spec) in _SPECS.items()
            if spec is not None
        }
        shard_dims["mask"] = 1  # an int: Shard(1) on mesh dim 0
        torch.manual_seed(41)
        m = deferred_init(_build)
        dts = materialize_module_dtensor(m, mesh, shard_dims=shard_dims)

        torch.manual_seed(41)
        ref = deferred_init(_build)
        materialize_module(ref)
        refs = dict(list(ref.named_parameters()) + list(ref.named_buffers()))

        out = {"names": sorted(dts)}
        for name, dt in dts.items():
            full = refs[name].detach()
            if name == "mask":
                want_pl = (Shard(1), Replicate())
            elif name == "scalar":
                want_pl = (Replicate(), Replicate())
            elif _SPECS[name][2] is None:
                want_pl = (Shard(0), Replicate())
            else:
                want_pl = tuple(
                    Shard(p.dim % full.dim()) if isinstance(p, Shard) else p
                    for p in shard_dims[name]
                )
            want_local = distribute_tensor(full, mesh, want_pl).to_local()
            local = dt.to_local()
            out[name] = {
                "placements": dt.placements == want_pl,
                "shape": tuple(dt.shape) == tuple(full.shape),
                "local_shape": tuple(local.shape) == tuple(want_local.shape),
                "local": torch.equal(local.detach(), want_local),
                "full": torch.equal(dt.full_tensor().detach(), full),
                "local_numel": local.numel(),
                "requires_grad": dt.requires_grad,
            }

        # Placement types other than Shard / Replicate are named and refused.
        torch.manual_seed(41)
        m2 = deferred_init(_build)
        for bad in (
            [_StridedShard(0, split_factor=2), Replicate()],
            [Shard(0)],  # one placement for a 2-d mesh
        ):
            try:
                materialize_module_dtensor(m2, mesh, shard_dims={"both": bad})
                out.setdefault("errors", []).append(None)
            except ValueError as e:
                out.setdefault("errors", []).append(str(e))

        # A 1-D mesh takes placement sequences too, and keeps its meaning
        # for everything it accepted before.
        flat = mesh["tp"]
        torch.manual_seed(41)
        m3 = deferred_init(_build)
        one = materialize_module_dtensor(
            m3, flat, shard_dims={"both": [Shard(1)], "nested": 1,
                                  "tiny": None, "scalar": None})
        out["one_d"] = {
            "both": one["both"].placements == (Shard(1),)
            and torch.equal(
                one["both"].to_local().detach(),
                distribute_tensor(refs["both"].detach(), flat,
                                  [Shard(1)]).to_local()),
            "nested": one["nested"].placements == (Shard(1),),
            "tiny": one["tiny"].placements == (Replicate(),),
            "default": one["default"].placements == (Shard(0),)
            and torch.equal(one["default"].full_tensor().detach(),
                            refs["default"].detach()),
        }
        return out
    finally:
        _C.set_native_init_cpu(False)


@pytest.fixture(scope="module")
def results():
    return run_distributed(_worker, 4)


def test_every_tensor_is_returned(results) -> None:
    for r in results:
        assert r["names"] == sorted(list(_SPECS) + ["mask"])


@pytest.mark.parametrize("name", list(_SPECS) + ["mask"])
def test_local_blocks_match_distribute_tensor(results, name) -> None:
    for rank, r in enumerate(results):
        got = r[name]
        for key in ("placements", "shape", "local_shape", "local", "full"):
            assert got[key], (rank, name, key)
        assert got["requires_grad"] == (name != "mask")


def test_uneven_and_empty_chunks(results) -> None:
    # (3, 8) under [Shard(0), Shard(0)]: rows split 2 + 1, then 1 + 1 and
    # 1 + 0 — the last rank holds an empty (0, 8) block.
    assert [r["nested"]["local_numel"] for r in results] == [8, 8, 8, 0]
    # (1, 5): only rank 0 holds anything.
    assert [r["tiny"]["local_numel"] for r in results] == [5, 0, 0, 0]
    # (5, 3) under [Replicate(), Shard(1)]: columns split 2 + 1.
    assert [r["tp_only"]["local_numel"] for r in results] == [10, 5, 10, 5]
    # Each rank keeps a quarter of the stacked expert weight.
    assert [r["experts"]["local_numel"] for r in results] == [48] * 4


def test_unsupported_placements_raise(results) -> None:
    for r in results:
        strided, short = r["errors"]
        assert strided is not None and "_StridedShard" in strided
        assert short is not None and "placements" in short


def test_one_d_mesh_keeps_its_meaning(results) -> None:
    for r in results:
        assert all(r["one_d"].values()), r["one_d"]
