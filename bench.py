#!/usr/bin/env python3
"""Flagship benchmark: deferred_init -> materialize wall-clock (the
BASELINE.json metric) on the named model configs.

One step = one full pipeline: record the module-construction tape under
deferred_init (CPU-side, C++ tape), then materialize every parameter and
buffer into HBM3E through the CDNA4 init kernels.

Default config: Llama-3-70B bf16, mode=replicate — every rank materializes
a full replica from the shared Philox streams with ZERO communication
(weak scaling: per-GPU work is fixed as N grows). On the xGMI fabric local
regeneration beats any broadcast by ~40x (see
torchdistx_amd/parallel/sharded_materialize.py), so this mode is both the
fastest way to replicate a model across a node and the honest flagship
number. --mode shard / broadcast measure the FSDP-style sharded path and
the RCCL-broadcast path.

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W
  torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...

Such a plain run only sets up, warms up, times the K steps and prints one
JSON result line. --dump-outputs DIR adds a dump of what the last timed
step materialized; --full is reserved for measurements beyond the headline
figure.
"""

import argparse
import json
import os
import resource
import sys
import time

import torch


def get_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--model", type=str, default=None,
                   help="config name (default: llama3-70b on GPU, tiny on "
                        "CPU); see torchdistx_amd.models.CONFIGS")
    p.add_argument("--mode", type=str, default="replicate",
                   choices=["replicate", "shard", "broadcast", "allgather", "slice"])
    p.add_argument("--dtype", type=str, default="bf16",
                   choices=["bf16", "fp32", "fp16"])
    p.add_argument("--init", type=str, default="fast",
                   choices=["fast", "stock"],
                   help="fast: one normal_ per weight; stock: PyTorch's "
                        "default kaiming resets (uniform_-dominated tape)")
    p.add_argument("--threads", type=int, default=1,
                   help="worker threads (one HIP stream each) for GPU "
                        "replicate-mode materialization; the pinned Philox "
                        "streams make the result bitwise independent of "
                        "replay order. Default 1: the 70B replicate step "
                        "is HBM-write-bound, so extra streams only add "
                        "allocator cross-stream overhead (measured t1 "
                        "53.3 ms vs t4 67.7 ms); the parallel path pays "
                        "off for many-small-tensor CPU/mixed workloads.")
    p.add_argument("--replay", type=str, default="pertensor",
                   choices=["pertensor", "batched"],
                   help="batched: collapse simple init chains and fill all "
                        "tensors in one kernel launch (bitwise-identical "
                        "to per-tensor replay)")
    p.add_argument("--selftest", action="store_true",
                   help="multi-rank preflight: validates communicator "
                        "creation, cross-rank bitwise equality of every "
                        "materialization mode, and shard coverage on the "
                        "tiny config, with the exact rank/env plumbing the "
                        "benchmark uses. Run it with the same launcher as "
                        "the benchmark (torchrun for N>1).")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step materialized (every parameter and buffer, or "
                        "this rank's slices in mode=slice) as "
                        "DIR/<name>.npy, float64 for float64/int64 tensors "
                        "and float32 for the rest. The 64 MB total is "
                        "split evenly over the tensors: one within its "
                        "share is written whole in its own shape, a larger "
                        "one as a 1-d fixed seeded sample of its elements "
                        "(about 21k per tensor for Llama-3-70B). *.npy "
                        "files already in DIR are removed first. "
                        "Inputs are seeded, so two "
                        "builds run with the same arguments can be compared "
                        "output for output. Ranks above 0 write under "
                        "DIR/rank<r>/.")
    p.add_argument("--full", action="store_true",
                   help="also run whatever the benchmark measures beyond "
                        "its headline figure. A plain run only sets up, "
                        "warms up, times the steps and prints the result "
                        "line; today there is nothing beyond that, so "
                        "--full changes nothing (the preflight stays "
                        "behind --selftest).")
    return p.parse_args()


# --dump-outputs writes at most this much array data (the limit is 64 MB;
# the rest is headroom for the .npy headers).
DUMP_BUDGET_BYTES = 60 << 20
# A sampled tensor always includes this many leading and trailing elements,
# where partial tiles and tail handling live.
DUMP_EDGE = 1024


def named_outputs(out):
    """(name, tensor) for everything a caller of the timed path receives:
    the slice dict of mode=slice, else the module's materialized parameters
    and buffers (mode=shard leaves the tensors other ranks own fake)."""
    from torchdistx_amd import is_fake

    if isinstance(out, dict):
        return sorted(out.items())
    named = list(out.named_parameters()) + list(out.named_buffers())
    return [(n, t) for n, t in named if not is_fake(t)]


def dump_outputs(out_dir, named, budget_bytes=DUMP_BUDGET_BYTES):
    """Write each tensor as out_dir/<name>.npy. The budget is split evenly:
    a tensor within its share is written whole in its own shape, a larger
    one as a sorted 1-d sample of its flattened elements, the edges plus
    indices drawn from a generator seeded by the tensor's name."""
    import zlib

    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    # Arrays of an earlier dump (another model or mode) must not mix in.
    for f in os.listdir(out_dir):
        if f.endswith(".npy"):
            os.remove(os.path.join(out_dir, f))
    share = budget_bytes // max(len(named), 1)
    for name, t in named:
        t = t.detach()
        wide = t.dtype in (torch.float64, torch.int64)
        out_dtype = torch.float64 if wide else torch.float32
        cap = share // out_dtype.itemsize
        if t.numel() > cap:
            n = t.numel()
            edge = min(DUMP_EDGE, cap // 4)
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            idx = torch.cat([
                torch.arange(edge),
                torch.randint(n, (cap - 2 * edge,), generator=g),
                torch.arange(n - edge, n),
            ]).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"),
                t.to(out_dtype).cpu().numpy())


def main():
    args = get_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))

    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(local_rank)
        device = f"cuda:{local_rank}"
    else:
        device = "cpu"

    distributed = world > 1
    if distributed:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl" if use_cuda else "gloo")
    else:
        dist = None

    # Fail loudly if materialization would silently fall back to stock ATen
    # kernels on a GPU box.
    if use_cuda:
        os.environ.setdefault("TDX_REQUIRE_NATIVE_INIT", "1")

    from torchdistx_amd import deferred_init, is_deferred, _kernels
    from torchdistx_amd.models import CONFIGS, build_model
    from torchdistx_amd.parallel import (
        materialize_module_dim0_sharded,
        materialize_module_distributed,
    )

    if use_cuda and not _kernels.available():
        print("FATAL: torchdistx_amd._K (CDNA4 kernels) not loaded on a GPU box",
              file=sys.stderr)
        sys.exit(1)

    if args.selftest:
        sys.exit(run_selftest(args, dist, device, rank, world, use_cuda))

    model_name = args.model or ("llama3-70b" if use_cuda else "tiny")
    if model_name not in CONFIGS:
        print(f"FATAL: unknown model {model_name!r}; available: "
              f"{sorted(CONFIGS)}", file=sys.stderr)
        sys.exit(2)
    cfg = CONFIGS[model_name]
    if args.init != cfg.init:
        import dataclasses

        cfg = dataclasses.replace(cfg, init=args.init)
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32,
             "fp16": torch.float16}[args.dtype]

    if use_cuda:
        # Fail fast with a clear message instead of an allocator OOM deep
        # inside materialization (e.g. llama3-405b needs >1 rank for any
        # non-replicated mode; replicate of it fits nowhere).
        per_rank = cfg.n_params * dtype.itemsize
        if args.mode in ("shard", "slice"):
            per_rank = -(-per_rank // world)  # this rank's share (ceil)
        hbm = torch.cuda.get_device_properties(0).total_memory
        if per_rank > hbm:  # Mixtral's 281 GB of 288 GB is fine; 812 GB is not
            print(
                f"FATAL: {model_name} mode={args.mode} needs "
                f"{per_rank / 1e9:.0f} GB per rank but the device has "
                f"{hbm / 1e9:.0f} GB; use more ranks or mode=slice/shard",
                file=sys.stderr,
            )
            sys.exit(1)

    def one_step(seed: int, keep: bool = False):
        torch.manual_seed(seed)
        module = deferred_init(build_model, cfg, device=device, dtype=dtype)
        if args.mode == "slice":
            # sub-tensor FSDP/TP-style init: this rank materializes its
            # contiguous dim-0 row-slice of every parameter.
            shards = materialize_module_dim0_sharded(module, rank, world)
            assert shards
            if keep:
                return shards
            del shards
        elif args.mode == "replicate" and use_cuda and args.replay == "batched":
            from torchdistx_amd.deferred_init import (
                materialize_module_batched,
            )

            materialize_module_batched(module)
            assert not is_deferred(module), "materialization incomplete"
        elif args.mode == "replicate" and use_cuda and args.threads > 1:
            from torchdistx_amd.deferred_init import (
                materialize_module_parallel,
            )

            materialize_module_parallel(module, num_threads=args.threads)
            assert not is_deferred(module), "materialization incomplete"
        else:
            materialize_module_distributed(module, mode=args.mode)
            if args.mode != "shard":
                assert not is_deferred(module), "materialization incomplete"
        # Reference-counting frees the module and its tape immediately (the
        # tape's ownership graph is acyclic by design); no gc.collect().
        if keep:
            return module
        del module

    def barrier_sync():
        if distributed:
            dist.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    for i in range(args.warmup):
        one_step(seed=1000 + i)
    barrier_sync()

    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = one_step(seed=2000 + i,
                        keep=bool(args.dump_outputs) and i == args.steps - 1)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        out_dir = args.dump_outputs
        if rank > 0:
            out_dir = os.path.join(out_dir, f"rank{rank}")
        dump_outputs(out_dir, named_outputs(last))
        # The kept step has not freed its module yet; every other step pays
        # for that inside the timed window, so this one is charged too.
        t_free = time.perf_counter()
        del last
        elapsed += time.perf_counter() - t_free

    # MAX over ranks.
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if use_cuda else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    ms_per_step = elapsed / args.steps * 1000.0
    n_params = cfg.n_params
    if args.mode == "replicate":
        # Whole-job aggregate: every rank materializes a full replica.
        total_params_per_step = n_params * world
        scaling = "weak"
    else:
        # One model materialized per step across all ranks.
        total_params_per_step = n_params
        scaling = "strong"
    value = total_params_per_step / (elapsed / args.steps)

    rss_gb = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6

    if rank == 0:
        print(json.dumps({
            "metric": "deferred_init_materialize_params_per_s",
            "value": value,
            "unit": "params/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic (random-init weights, no checkpoints)",
            "config": {
                "model": cfg.name,
                "n_params": n_params,
                "mode": args.mode,
                "init": args.init,
                "threads": args.threads,
                "replay": args.replay,
                "device": "cuda" if use_cuda else "cpu",
                "native_init_kernels": _kernels.available(),
                "peak_host_rss_gb": round(rss_gb, 2),
                "global_batch": None,
                "seq_len": None,
                "parallelism": f"{args.mode}{world}",
            },
        }))

    if distributed:
        dist.destroy_process_group()


def run_selftest(args, dist, device, rank, world, use_cuda) -> int:
    """Preflight for the multi-GPU benchmark paths: exercises every
    materialization mode on the tiny config with the exact env/rank
    plumbing the benchmark uses, and asserts cross-rank bitwise equality
    where the mode promises it. Cheap enough to run cold on a fresh node
    before the first real bench step."""
    import hashlib

    import torch.distributed  # noqa: F401  (dist may be None at world 1)

    from torchdistx_amd import deferred_init
    from torchdistx_amd.deferred_init import materialize_module
    from torchdistx_amd.models import CONFIGS, build_model
    from torchdistx_amd.parallel import (
        materialize_module_dim0_sharded,
        materialize_module_distributed,
    )

    cfg = CONFIGS["tiny"]
    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32,
             "fp16": torch.float16}[args.dtype]
    checks = []

    def digest(t):
        return hashlib.sha256(
            t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
        ).hexdigest()

    def model_digests(m):
        return {n: digest(p) for n, p in m.named_parameters()}

    def assert_all_ranks_equal(tag, digests):
        if world == 1:
            checks.append((tag, True, "world 1"))
            return
        gathered = [None] * world
        dist.all_gather_object(gathered, digests)
        ok = all(g == gathered[0] for g in gathered)
        checks.append((tag, ok, "" if ok else f"rank digests diverge: {tag}"))

    from contextlib import contextmanager

    from torchdistx_amd import _C

    @contextmanager
    def native_path():
        """The partition-invariant pinned-Philox path: default on GPU,
        opt-in on CPU. Partial (per-owner / per-slice) materializations
        are only order-independent on this path, so the distributed-mode
        bitwise checks run under it."""
        if use_cuda:
            yield
            return
        _C.set_native_init_cpu(True)
        try:
            yield
        finally:
            _C.set_native_init_cpu(False)

    # Local reference (every rank, same seed): the ground truth all
    # distributed modes must reproduce bitwise.
    torch.manual_seed(4242)
    ref = deferred_init(build_model, cfg, device=device, dtype=dtype)
    with native_path():
        materialize_module(ref)
    ref_digests = model_digests(ref)

    # 1. replicate: zero-comm bitwise replicas from the shared tape.
    torch.manual_seed(4242)
    m = deferred_init(build_model, cfg, device=device, dtype=dtype)
    with native_path():
        materialize_module_distributed(m, mode="replicate")
    ok = model_digests(m) == ref_digests
    checks.append(("replicate-matches-local", ok, "" if ok else "mismatch"))
    assert_all_ranks_equal("replicate-cross-rank", model_digests(m))

    # 2a. broadcast, same seed everywhere: result must equal the local
    # reference bitwise (no corruption in pack/transfer/unpack).
    if world > 1:
        torch.manual_seed(4242)
        m = deferred_init(build_model, cfg, device=device, dtype=dtype)
        with native_path():
            materialize_module_distributed(m, mode="broadcast")
        ok = model_digests(m) == ref_digests
        checks.append(
            ("broadcast-matches-local", ok, "" if ok else "mismatch")
        )

        # 2b. broadcast with rank-SKEWED seeds: every tensor must carry
        # its OWNER's bits on every rank — only the wire can make the
        # ranks converge, so this catches a broadcast that silently
        # degenerates to local materialization.
        torch.manual_seed(4242 + 7 * rank)
        m = deferred_init(build_model, cfg, device=device, dtype=dtype)
        with native_path():
            materialize_module_distributed(m, mode="broadcast")
        assert_all_ranks_equal("broadcast-skewed-cross-rank",
                               model_digests(m))

        # 3. shard: every tensor materialized on exactly its owner.
        from torchdistx_amd import _C

        torch.manual_seed(4242)
        m = deferred_init(build_model, cfg, device=device, dtype=dtype)
        with native_path():
            owner_map = materialize_module_distributed(m, mode="shard")
        n_entries = len(owner_map)
        still_fake = sum(
            1
            for t in list(m.parameters()) + list(m.buffers())
            if _C.can_materialize(t)
        )
        materialized_here = n_entries - still_fake
        expected_here = sum(1 for o in owner_map.values() if o == rank)
        counts = [None] * world
        dist.all_gather_object(counts, materialized_here)
        ok = materialized_here == expected_here and sum(counts) == n_entries
        checks.append(
            ("shard-coverage", ok,
             "" if ok else
             f"materialized {sum(counts)} of {n_entries} "
             f"(here {materialized_here}, expected {expected_here})")
        )

    # 4. slice: concatenating every rank's dim-0 slices reconstructs a
    # full NATIVE materialization bitwise. (On CPU the plain reference
    # uses the stock generator for eager parity, so a pinned-Philox
    # native reference is materialized here for the comparison; on GPU
    # the native kernels are the default path already.)
    torch.manual_seed(4242)
    native_ref = deferred_init(build_model, cfg, device=device, dtype=dtype)
    with native_path():
        materialize_module(native_ref)

    torch.manual_seed(4242)
    m = deferred_init(build_model, cfg, device=device, dtype=dtype)
    shards = materialize_module_dim0_sharded(m, rank, world)
    my = {n: s.detach().cpu() for n, s in shards.items()}
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, my)
    else:
        gathered = [my]
    ok = True
    detail = ""
    ref_params = dict(native_ref.named_parameters())
    ref_buffers = dict(native_ref.named_buffers())
    for name in my:
        full = torch.cat([g[name] for g in gathered], dim=0)
        want = ref_params.get(name, ref_buffers.get(name))
        if want is None or not torch.equal(
            full.view(want.shape), want.detach().cpu()
        ):
            ok = False
            detail = f"slice reassembly mismatch: {name}"
            break
    checks.append(("slice-reassembly", ok, detail))

    # 5. tp: concatenating every rank's dim-1 (row-parallel) slices of
    # each 2-d weight reconstructs the same native reference bitwise —
    # the windowed shard kernels' cross-rank contract.
    from torchdistx_amd.parallel import materialize_tensor_shard

    torch.manual_seed(4242)
    m2 = deferred_init(build_model, cfg, device=device, dtype=dtype)
    with native_path():
        my2 = {}
        for name, p in m2.named_parameters():
            if p.dim() != 2:
                continue
            n_cols = p.shape[1]
            a = rank * n_cols // world
            b = (rank + 1) * n_cols // world
            my2[name] = materialize_tensor_shard(p, a, b, dim=1).detach().cpu()
    if world > 1:
        gathered2 = [None] * world
        dist.all_gather_object(gathered2, my2)
    else:
        gathered2 = [my2]
    ok = True
    detail = ""
    for name in my2:
        full = torch.cat([g[name] for g in gathered2], dim=1)
        if not torch.equal(full, ref_params[name].detach().cpu()):
            ok = False
            detail = f"tp dim-1 reassembly mismatch: {name}"
            break
    checks.append(("tp-dim1-reassembly", ok, detail))

    failed = [c for c in checks if not c[1]]
    if rank == 0:
        print(json.dumps({
            "selftest": "pass" if not failed else "FAIL",
            "world": world,
            "device": "cuda" if use_cuda else "cpu",
            "backend": "nccl" if (use_cuda and world > 1) else
                       ("gloo" if world > 1 else None),
            "checks": [
                {"name": n, "ok": ok, "detail": d} for n, ok, d in checks
            ],
        }))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 1 if failed else 0


if __name__ == "__main__":
    main()
