#!/usr/bin/env python3
"""FSDP x TP initialization on a 2-D device mesh: every parameter comes up
directly as a DTensor over a (dp, tp) mesh, each rank generating exactly
the block it keeps — rows split over dp on top of the Megatron column /
row split over tp — with zero communication, bitwise-consistent with the
full model.

  torchrun --standalone --nproc-per-node 8 examples/init_2d_mesh.py

Also runs single-rank: `python examples/init_2d_mesh.py` (a 1 x 1 mesh).
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import time

import torch
import torch.distributed as dist
from torch.distributed.device_mesh import init_device_mesh
from torch.distributed.tensor import Replicate, Shard

from torchdistx_amd import deferred_init
from torchdistx_amd.models import LLAMA3_8B, TINY, build_model
from torchdistx_amd.parallel import materialize_module_dtensor


def placements_2d(model) -> dict:
    """Placements per (dp, tp) mesh dim. TP follows Megatron: wq/wk/wv and
    the FFN up/gate projections are column-parallel (tp shards dim 0 of
    the [out, in] weight), wo and the FFN down projection row-parallel
    (tp shards dim 1); embeddings split on the vocab dim. FSDP then
    shards dim 0 of whatever TP left on the rank — for column-parallel
    weights both mesh dims shard dim 0 and nest. Norms and other small
    tensors keep the default: Shard(0) over dp, replicated over tp."""
    out = {}
    for name, _ in model.named_parameters():
        if name.endswith(("wq.weight", "wk.weight", "wv.weight",
                          "w1.weight", "w3.weight")):
            out[name] = [Shard(0), Shard(0)]
        elif name.endswith(("wo.weight", "w2.weight")):
            out[name] = [Shard(0), Shard(1)]
        elif name in ("tok_emb.weight", "lm_head.weight"):
            out[name] = [Shard(0), Shard(0)]
    return out


def main():
    if "RANK" not in os.environ:  # plain `python ...` -> single-rank run
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("LOCAL_RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29574")
    backend = "nccl" if torch.cuda.is_available() else "gloo"
    dist.init_process_group(backend)
    rank = dist.get_rank()
    world = dist.get_world_size()
    device = "cuda" if torch.cuda.is_available() else "cpu"
    if device == "cuda":
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))

    # tp = 2 where the world allows it (8 ranks -> a 4 x 2 mesh).
    tp = 2 if world % 2 == 0 else 1
    mesh = init_device_mesh(device, (world // tp, tp),
                            mesh_dim_names=("dp", "tp"))

    # Llama-3-8B on GPU; the tiny config keeps a GPU-less rehearsal quick.
    cfg = LLAMA3_8B if device == "cuda" else TINY
    torch.manual_seed(0)  # all ranks pin the same Philox streams
    t0 = time.perf_counter()
    model = deferred_init(build_model, cfg, device=device,
                          dtype=torch.bfloat16)
    dts = materialize_module_dtensor(model, mesh,
                                     shard_dims=placements_2d(model))
    if device == "cuda":
        torch.cuda.synchronize()
    t1 = time.perf_counter()

    local = [dt.to_local() for dt in dts.values()]
    local_gb = sum(t.numel() * t.element_size() for t in local) / 1e9
    full_gb = sum(dt.numel() * dt.element_size() for dt in dts.values()) / 1e9
    n_2d = sum(
        1 for dt in dts.values()
        if not any(isinstance(p, Replicate) for p in dt.placements)
    )
    print(f"rank {rank}/{world} on a {world // tp} x {tp} mesh: "
          f"{len(dts)} DTensors ({n_2d} sharded on both mesh dims), "
          f"{local_gb:.2f} of {full_gb:.2f} GB local, "
          f"{(t1 - t0) * 1e3:.0f} ms")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
