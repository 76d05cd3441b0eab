"""Measures the fused init-chain kernel against the unfused chain on one
MI355X, for bf16 tensors of Llama-3-70B weight shapes:

  (i)  unfused: tdx.uniform_, then ATen erfinv_, mul_, add_, clamp_ —
       five launches, one write and four read-modify-writes;
  (ii) fused:   tdx.rng_chain_ — one launch, one write.

(The trunc_normal_ chain. A plain tdx.uniform_ is timed too, as the
store-bound yardstick: how far (ii) falls below it is erfinv's VALU
cost.) The two outputs are checked bitwise equal first. The variants
alternate inside one process, each warmed up and timed with device
events over a window of at least a second, and the whole comparison
runs three times to show the spread.

Usage: python scripts/chain_kernel_bench.py [--out FILE]

Writes a markdown report (default profiles/fused_chain_bench.md; text
after the end marker in an existing report is kept). Exits non-zero
without a GPU.
"""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

SHAPES = [(8192, 28672), (128256, 8192)]
REPEATS = 3
MIN_WINDOW_S = 1.0
END_MARK = "<!-- end of chain_kernel_bench.py output -->"

# trunc_normal_(mean=0, std=0.02, a=-2, b=2): the bounds are 100 sigma
# out, so the uniform runs over (2*Phi(-100)-1, 2*Phi(100)-1) = (-1, 1).
LO, HI = -1.0, 1.0
SCALE, MEAN, A, B = 0.02 * math.sqrt(2.0), 0.0, -2.0, 2.0
ERFINV, MUL, ADD, CLAMP = 0, 1, 2, 4
SEED, OFFSET = 20240607, 4


def unfused(t):
    torch.ops.tdx.uniform_(t, LO, HI, seed=SEED, offset=OFFSET)
    t.erfinv_().mul_(SCALE).add_(MEAN).clamp_(A, B)


def fused(t):
    torch.ops.tdx.rng_chain_(
        t, 0, LO, HI, [ERFINV, MUL, ADD, CLAMP], [0.0, SCALE, MEAN, A],
        [0.0, 0.0, 0.0, B], seed=SEED, offset=OFFSET)


def plain_uniform(t):
    torch.ops.tdx.uniform_(t, LO, HI, seed=SEED, offset=OFFSET)


def event_ms(fn, t, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn(t)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def timed(fn, t):
    """Mean ms per call over a window of at least MIN_WINDOW_S."""
    for _ in range(5):
        fn(t)
    torch.cuda.synchronize()
    probe = event_ms(fn, t, 5)
    iters = max(10, int(math.ceil(MIN_WINDOW_S * 1e3 / probe)))
    return event_ms(fn, t, iters), iters


def main() -> int:
    parser = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    parser.add_argument(
        "--out", default=os.path.join(ROOT, "profiles",
                                      "fused_chain_bench.md"))
    args = parser.parse_args()

    if not torch.cuda.is_available():
        print("chain_kernel_bench: needs a ROCm GPU", file=sys.stderr)
        return 1
    import torchdistx_amd  # noqa: F401  (registers tdx:: ops)
    from torchdistx_amd import _kernels

    if not (_kernels.available() and _kernels._K.has_fused_chains()):
        print("chain_kernel_bench: torchdistx_amd._K with fused chains "
              "did not load", file=sys.stderr)
        return 1

    lines = [
        "# Fused init-chain kernel vs the unfused chain",
        "",
        f"`scripts/chain_kernel_bench.py` on {torch.cuda.get_device_name(0)}"
        f", torch {torch.__version__}. bf16, trunc_normal_ chain "
        "(uniform_ -> erfinv_ -> mul_ -> add_ -> clamp_). Times are mean "
        "ms per materialization over a >= 1 s device-event window; the "
        "variants alternate within each repeat.",
        "",
        "| shape | repeat | (i) unfused ms | (ii) fused ms | (i)/(ii) | "
        "(ii) store TB/s | plain uniform_ ms | plain TB/s |",
        "|---|---|---|---|---|---|---|---|",
    ]
    verdicts = []
    for shape in SHAPES:
        t = torch.empty(shape, device="cuda", dtype=torch.bfloat16)
        nbytes = t.numel() * t.element_size()
        unfused(t)
        want = t.clone()
        t.zero_()
        fused(t)
        equal = torch.equal(t, want)
        del want
        if not equal:
            print(f"chain_kernel_bench: fused != unfused at {shape}",
                  file=sys.stderr)
            return 2
        ratios, un_ms, fu_ms = [], [], []
        for rep in range(REPEATS):
            u, _ = timed(unfused, t)
            f, _ = timed(fused, t)
            p, _ = timed(plain_uniform, t)
            un_ms.append(u)
            fu_ms.append(f)
            ratios.append(u / f)
            row = (f"| {shape[0]}x{shape[1]} | {rep + 1} | {u:.3f} | "
                   f"{f:.3f} | {u / f:.2f} | {nbytes / f / 1e9:.2f} | "
                   f"{p:.3f} | {nbytes / p / 1e9:.2f} |")
            print(row, flush=True)
            lines.append(row)
        # Faster by more than the run-to-run spread: the slowest fused
        # repeat still beats the fastest unfused one.
        ok = max(fu_ms) < min(un_ms)
        spread_u = (max(un_ms) - min(un_ms)) / min(un_ms)
        spread_f = (max(fu_ms) - min(fu_ms)) / min(fu_ms)
        verdicts.append(
            f"- {shape[0]}x{shape[1]}: outputs bitwise equal; fused is "
            f"{min(ratios):.2f}x-{max(ratios):.2f}x faster; spread over "
            f"repeats {spread_u * 100:.1f} % (unfused), "
            f"{spread_f * 100:.1f} % (fused); "
            + ("faster beyond the spread." if ok
               else "NOT faster beyond the spread."))
        del t
        torch.cuda.empty_cache()
    lines += [""] + verdicts + ["", END_MARK]
    for v in verdicts:
        print(v)

    kept = ""
    if os.path.exists(args.out):
        with open(args.out) as fh:
            old = fh.read()
        if END_MARK in old:
            kept = old.split(END_MARK, 1)[1]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + (kept if kept else "\n"))
    return 0 if all("NOT faster" not in v for v in verdicts) else 3


if __name__ == "__main__":
    sys.exit(main())
