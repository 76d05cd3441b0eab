"""Measures the cast-chain kernel against the two launches it replaces, on
one MI355X, per (source -> destination) dtype pair and distribution:

  (i)  two launches: tdx.uniform_ / tdx.normal_ into a tensor of the
       source dtype, then `.to(dst)` — what node-by-node replay runs for
       `empty(..).normal_().to(bf16)` or `Module.to(dtype)` in a builder:
       a write, a read and a write, plus a transient source-dtype tensor;
  (ii) one launch: tdx.rng_chain_cast_ straight into the destination.

The two outputs are checked bitwise equal first. The variants alternate
inside one process, each warmed up and timed with device events over a
window of at least MIN_WINDOW_S; the comparison runs REPEATS times and
the medians are reported with the spread. Peak device memory of each
variant (above what was allocated before it) is recorded too.

Usage: python scripts/cast_chain_bench.py [--out FILE] [--sizes 20,26,30]

Writes a markdown report (default profiles/cast_chain_bench.md; text
after the end marker in an existing report is kept). Exits non-zero
without a GPU. No time threshold is applied: the report states what was
measured.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# (src, dst, dist code, name)
CASES = [
    (F32, BF16, 0, "uniform"),
    (F32, BF16, 1, "normal"),
    (BF16, F32, 0, "uniform"),
    (BF16, F16, 0, "uniform"),
]
REPEATS = 3
MIN_WINDOW_S = 0.5
END_MARK = "<!-- end of cast_chain_bench.py output -->"
SEED, OFFSET = 20240607, 4
P = {0: (-1.0, 1.0), 1: (0.0, 0.02)}


def two_launches(numel, src, dst, dist):
    t = torch.empty(numel, device="cuda", dtype=src)
    if dist == 0:
        torch.ops.tdx.uniform_(t, *P[0], seed=SEED, offset=OFFSET)
    else:
        torch.ops.tdx.normal_(t, *P[1], seed=SEED, offset=OFFSET)
    return t.to(dst)


def one_launch(numel, src, dst, dist):
    out = torch.empty(numel, device="cuda", dtype=dst)
    torch.ops.tdx.rng_chain_cast_(out, src, dist, *P[dist], [], [], [],
                                  seed=SEED, offset=OFFSET)
    return out


def event_ms(fn, args, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn(*args)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def timed(fn, args):
    """Mean ms per call over a window of at least MIN_WINDOW_S. The
    allocations are part of both variants and come from the caching
    allocator after the warm-up."""
    for _ in range(5):
        fn(*args)
    torch.cuda.synchronize()
    probe = event_ms(fn, args, 5)
    iters = max(10, int(math.ceil(MIN_WINDOW_S * 1e3 / probe)))
    return event_ms(fn, args, iters)


def peak_bytes(fn, args):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*args)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def name(dtype):
    return str(dtype).replace("torch.", "")


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument(
        "--out", default=os.path.join(ROOT, "profiles",
                                      "cast_chain_bench.md"))
    parser.add_argument("--sizes", default="20,26,30",
                        help="log2 element counts, comma separated")
    args = parser.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

    if not torch.cuda.is_available():
        print("cast_chain_bench: needs a ROCm GPU", file=sys.stderr)
        return 1
    import torchdistx_amd  # noqa: F401  (registers tdx:: ops)
    from torchdistx_amd import _kernels

    if not (_kernels.available() and _kernels._K.has_cast_chains()):
        print("cast_chain_bench: torchdistx_amd._K with cast chains did "
              "not load", file=sys.stderr)
        return 1

    lines = [
        "# Cast-chain kernel vs RNG kernel + `.to()`",
        "",
        f"`scripts/cast_chain_bench.py` on {torch.cuda.get_device_name(0)}, "
        f"torch {torch.__version__}. (i) = tdx RNG op at the source dtype, "
        "then `.to(dst)`; (ii) = `tdx.rng_chain_cast_`. Times are medians "
        f"of {REPEATS} repeats of the mean ms per call over a >= "
        f"{MIN_WINDOW_S} s device-event window (allocation included in "
        "both), the variants alternating within each repeat; spread = "
        "(max - min) / min over the repeats. Store rate = destination "
        "bytes / time of (ii). Peak = device memory above the starting "
        "level during one call.",
        "",
        "| pair | dist | elements | (i) ms | (ii) ms | (i)/(ii) | spread "
        "(i) / (ii) | (ii) store TB/s | peak (i) MiB | peak (ii) MiB |",
        "|---|---|---|---|---|---|---|---|---|---|",
    ]
    for src, dst, dist, dist_name in CASES:
        for log2 in sizes:
            numel = 1 << log2
            call = (numel, src, dst, dist)
            a = two_launches(*call)
            b = one_launch(*call)
            equal = torch.equal(a, b)
            del a, b
            if not equal:
                print(f"cast_chain_bench: outputs differ for {call}",
                      file=sys.stderr)
                return 2
            two_ms, one_ms = [], []
            for _ in range(REPEATS):
                two_ms.append(timed(two_launches, call))
                one_ms.append(timed(one_launch, call))
            peak_two = peak_bytes(two_launches, call)
            peak_one = peak_bytes(one_launch, call)
            t2 = statistics.median(two_ms)
            t1 = statistics.median(one_ms)
            spread2 = (max(two_ms) - min(two_ms)) / min(two_ms) * 100
            spread1 = (max(one_ms) - min(one_ms)) / min(one_ms) * 100
            dst_bytes = numel * torch.empty((), dtype=dst).element_size()
            row = (f"| {name(src)} -> {name(dst)} | {dist_name} | 2^{log2} "
                   f"| {t2:.4f} | {t1:.4f} | {t2 / t1:.2f} | "
                   f"{spread2:.1f} % / {spread1:.1f} % | "
                   f"{dst_bytes / t1 / 1e9:.2f} | {peak_two / 2**20:.1f} | "
                   f"{peak_one / 2**20:.1f} |")
            print(row, flush=True)
            lines.append(row)
            torch.cuda.empty_cache()
    lines += ["", END_MARK]

    kept = ""
    if os.path.exists(args.out):
        with open(args.out) as fh:
            old = fh.read()
        if END_MARK in old:
            kept = old.split(END_MARK, 1)[1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + (kept if kept else "\n"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
