"""Measures the N-d box kernel (tdx::rng_box_, block materialization for
2-D meshes) on one MI355X against the single-dim window kernel at the same
shard size, and against the route the docs recommended before it existed:
slice one dim natively, then narrow().clone() the others.

Workload: bf16 normal, virtual full tensor (4, 28672, 8192) — four stacked
Llama-3-70B FFN weights — box [1:3, 0:14336, 1024:2048] = 29.4M elements,
the byte count of win_kernel_bench.py's dim-1 1/8 slice. The full tensor is
never materialized.

All variants run in one process, alternating, `--repeats` timed windows
each (a synchronise on both sides, `--iters` calls inside); medians and
the min-max spread are reported. TDX_BOX_PLAIN_DIV=1 makes the untailed
32-bit normal box kernels divide with `/` instead of the multiply-shift
divisor, so both forms are timed side by side.

Usage: python scripts/box_kernel_bench.py [--iters 300] [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torchdistx_amd  # noqa: F401  (registers tdx:: ops)
from torchdistx_amd import deferred_init
from torchdistx_amd.parallel import (
    materialize_tensor_block,
    materialize_tensor_shard,
)

E, R, C = 4, 28672, 8192
FULL_NUMEL = E * R * C
SEED, OFFSET = 1, 4


def window_time(fn, iters):
    if getattr(fn, "plain", False):
        os.environ["TDX_BOX_PLAIN_DIV"] = "1"
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters
    finally:
        os.environ.pop("TDX_BOX_PLAIN_DIV", None)


def box_call(shard, lo_col, hi_col, plain=False):
    rows = R // 2
    args = (shard, [2, rows], [R * C, C], hi_col - lo_col,
            1 * R * C + lo_col, 1, 0.0, 1.0, [], [], [], FULL_NUMEL, SEED,
            OFFSET)

    def call():
        torch.ops.tdx.rng_box_(*args)

    call.plain = plain  # window_time sets the switch around the window
    return call


def win_call(shard, lo_col, hi_col):
    # The existing bench geometry: a dim-1 slice of one [R, C] weight.
    return lambda: torch.ops.tdx.normal_shard_win_(
        shard, R, hi_col - lo_col, C, lo_col, 0.0, 1.0, seed=SEED,
        offset=OFFSET)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--api-iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    opts = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"

    def build():
        m = torch.nn.Module()
        m.w = torch.nn.Parameter(
            torch.empty(E, R, C, dtype=torch.bfloat16, device="cuda").normal_())
        return m

    torch.manual_seed(7)
    deferred = deferred_init(build)
    ranges = [(1, 3), (0, R // 2), (1024, 2048)]

    def compose():
        with torch.no_grad():
            return materialize_tensor_shard(
                deferred.w, 1024, 2048, 2)[1:3, 0:R // 2].clone()

    def api_box():
        with torch.no_grad():
            return materialize_tensor_block(deferred.w, ranges)

    # Same bits from every route, at the size that is timed.
    want = compose().detach()
    assert torch.equal(api_box().detach(), want)
    assert want.numel() == 2 * (R // 2) * 1024
    del want

    bf = torch.empty(2, R // 2, 1024, dtype=torch.bfloat16, device="cuda")
    bf_odd = torch.empty(2, R // 2, 1023, dtype=torch.bfloat16, device="cuda")
    f32 = torch.empty(2, R // 2, 1024, dtype=torch.float32, device="cuda")
    wbf = torch.empty(R, 1024, dtype=torch.bfloat16, device="cuda")
    wbf_odd = torch.empty(R, 1023, dtype=torch.bfloat16, device="cuda")
    wf32 = torch.empty(R, 1024, dtype=torch.float32, device="cuda")

    box_call(bf, 1024, 2048)()
    a = bf.clone()
    window_time(box_call(bf, 1024, 2048, plain=True), 1)
    assert torch.equal(a, bf), "plain-division kernel differs"
    del a

    # (name, call, bytes per call, iterations per window)
    n, it, ait = bf.numel(), opts.iters, opts.api_iters
    variants = [
        ("rng_box_ bf16 aligned (multiply-shift)",
         box_call(bf, 1024, 2048), n * 2, it),
        ("rng_box_ bf16 aligned (plain /)",
         box_call(bf, 1024, 2048, plain=True), n * 2, it),
        ("normal_shard_win_ bf16 aligned, same numel",
         win_call(wbf, 1024, 2048), n * 2, it),
        ("rng_box_ bf16 odd width 1025:2048",
         box_call(bf_odd, 1025, 2048), bf_odd.numel() * 2, it),
        ("rng_box_ bf16 odd width (plain /)",
         box_call(bf_odd, 1025, 2048, plain=True), bf_odd.numel() * 2, it),
        ("normal_shard_win_ bf16 odd width",
         win_call(wbf_odd, 1025, 2048), wbf_odd.numel() * 2, it),
        ("rng_box_ f32 aligned (multiply-shift)",
         box_call(f32, 1024, 2048), n * 4, it),
        ("rng_box_ f32 aligned (plain /)",
         box_call(f32, 1024, 2048, plain=True), n * 4, it),
        ("normal_shard_win_ f32 aligned, same numel",
         win_call(wf32, 1024, 2048), n * 4, it),
        ("materialize_tensor_block (API, allocates)", api_box, n * 2, ait),
        ("compose: shard dim 2, then [1:3, 0:14336].clone()",
         compose, n * 2, ait),
    ]

    # Warm clocks and code objects: every variant, then half a second of
    # the main kernel.
    for _, fn, _, _ in variants:
        window_time(fn, 5)
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:
        for _ in range(50):
            variants[0][1]()
        torch.cuda.synchronize()

    times = {name: [] for name, _, _, _ in variants}
    for _ in range(opts.repeats):
        for name, fn, _, iters in variants:  # alternating
            times[name].append(window_time(fn, iters))

    print(f"iters/window {it} (API rows {ait}), repeats {opts.repeats}, "
          f"box {n} elements")
    print(f"{'variant':<52} {'median us':>10} {'min us':>9} {'max us':>9} "
          f"{'TB/s':>6}")
    for name, _, nbytes, _ in variants:
        ts = times[name]
        med = statistics.median(ts)
        print(f"{name:<52} {med * 1e6:10.1f} {min(ts) * 1e6:9.1f} "
              f"{max(ts) * 1e6:9.1f} {nbytes / med / 1e12:6.2f}")


if __name__ == "__main__":
    main()
