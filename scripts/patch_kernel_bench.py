"""Measures slice materialization of tensors whose init overwrites a
contiguous sub-range (tdx::patch_box_) on one MI355X.

Workloads, bf16 on the GPU, the full tensor never needed by the new path:
  * a (128256, 16384) embedding with padding_idx=3 — normal_ on the whole
    table, then a zero fill of one row (a constant patch);
  * a (10240, 8192) fused QKV weight initialized by parts —
    w[:8192].normal_(std=0.02); w[8192:].normal_(std=0.5) (two RNG patches
    that together cover the tensor).
For each, one 1/8 row shard and one 1/8 column block, three ways:
  new      materialize_tensor_shard of the patched tensor (this build);
  parent   what the parent commit's fallback does for these tapes:
           materialize_tensor, then narrow().clone();
  plain    the same shard of the same tensor WITHOUT the patch (one
           whole-tensor normal_), the floor a patched shard can reach.

All variants run in one process, alternating, `--repeats` timed windows
each (a synchronise on both sides, `--iters` calls inside; the parent path
gets `--full-iters`, each on a fresh tape built outside the window, since a
full materialization consumes its tape). Medians and the min-max spread
are reported.

Usage: python scripts/patch_kernel_bench.py [--iters 200] [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torchdistx_amd  # noqa: F401  (registers tdx:: ops)
from torchdistx_amd import _C, deferred_init
from torchdistx_amd.parallel import materialize_tensor_shard

BF16 = torch.bfloat16


def emb_padded():
    return torch.nn.Embedding(128256, 16384, padding_idx=3, device="cuda",
                              dtype=BF16)


def emb_plain():
    return torch.nn.Embedding(128256, 16384, device="cuda", dtype=BF16)


def _holder(w):
    m = torch.nn.Module()
    m.weight = torch.nn.Parameter(w)
    return m


def qkv_parts():
    w = torch.empty(10240, 8192, device="cuda", dtype=BF16)
    w[:8192].normal_(std=0.02)
    w[8192:].normal_(std=0.5)
    return _holder(w)


def qkv_plain():
    return _holder(
        torch.empty(10240, 8192, device="cuda", dtype=BF16).normal_(std=0.02))


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--full-iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    assert _C.native_init_enabled()

    variants = []  # (name, fn, iters, shard bytes)
    for label, patched, plain in [("embedding+pad", emb_padded, emb_plain),
                                  ("qkv by parts", qkv_parts, qkv_plain)]:
        torch.manual_seed(7)
        new_t = deferred_init(patched).weight
        torch.manual_seed(7)
        plain_t = deferred_init(plain).weight
        rows, cols = new_t.shape
        for dim, n in ((0, rows), (1, cols)):
            a, b = 0, n // 8
            nbytes = new_t.numel() // n * (b - a) * 2

            def new(t=new_t, a=a, b=b, dim=dim):
                with torch.no_grad():
                    return _C.materialize_tensor_shard(t, a, b, dim)

            def base(t=plain_t, a=a, b=b, dim=dim):
                with torch.no_grad():
                    return _C.materialize_tensor_shard(t, a, b, dim)

            fresh = []

            def parent(a=a, b=b, dim=dim, fresh=fresh):
                t = fresh.pop()
                with torch.no_grad():
                    return _C.materialize_tensor(t).narrow(
                        dim, a, b - a).clone()

            def refill(patched=patched, fresh=fresh, k=opts.full_iters):
                while len(fresh) < k:
                    torch.manual_seed(7)
                    fresh.append(deferred_init(patched).weight)

            # Same bits from both routes, at the size that is timed.
            refill()
            want = parent()
            assert torch.equal(new(), want), (label, dim)
            assert torch.equal(
                materialize_tensor_shard(new_t, a, b, dim).detach(), want)
            del want
            tag = f"{label} dim {dim} [{a}:{b}]"
            variants.append((f"{tag} new", new, opts.iters, nbytes, None))
            variants.append((f"{tag} plain", base, opts.iters, nbytes, None))
            variants.append((f"{tag} parent", parent, opts.full_iters, nbytes,
                             refill))

    # Warm clocks and code objects: every variant, then half a second of
    # the first one.
    for _, fn, _, _, refill in variants:
        if refill is not None:
            refill()
        window(fn, 2)
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:
        for _ in range(20):
            variants[0][1]()
        torch.cuda.synchronize()

    times = {name: [] for name, *_ in variants}
    for _ in range(opts.repeats):
        for name, fn, iters, _, refill in variants:  # alternating
            if refill is not None:
                refill()
            times[name].append(window(fn, iters))

    print(f"iters/window {opts.iters} (parent rows {opts.full_iters}), "
          f"repeats {opts.repeats}")
    print(f"{'variant':<44} {'median us':>10} {'min us':>10} {'max us':>10} "
          f"{'shard MB':>9}")
    for name, _, _, nbytes, _ in variants:
        ts = times[name]
        print(f"{name:<44} {statistics.median(ts) * 1e6:10.1f} "
              f"{min(ts) * 1e6:10.1f} {max(ts) * 1e6:10.1f} "
              f"{nbytes / 1e6:9.1f}")


if __name__ == "__main__":
    main()
