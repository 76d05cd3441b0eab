"""A/B of one SlowMo outer step on GPU: SlowMomentumOptimizer with
use_fused=True (csrc/hip/slowmo.hip: pack kernel, all-reduce of one flat
buffer, outer-step kernel) against use_fused=False (stock averager plus
five tensor ops per parameter), on the Llama-3-8B parameter list in bf16
and in fp32, single-rank process group.

slowmo_freq=1 makes every step after the first an averaging step with an
outer update; the base optimizer's step is empty, so a step is the outer
step alone (gradients are set, because the averager takes the parameters
that have one). One optimizer over one set of tensors serves
both variants (the flag is switched between windows), windows alternate,
and each figure is the median of `--repeats` windows of `--steps` steps,
timed from the host around a device synchronise.

  python scripts/slowmo_bench.py                 # the tables
  python scripts/slowmo_bench.py --count eager=2,fused=0 --dtypes bf16
      # for a kernel trace: after set-up, exactly that many untimed steps
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import socket
import time

import torch
import torch.distributed as dist

from torchdistx_amd.models import LLAMA3_8B, build_model
from torchdistx_amd.slowmo import SlowMomentumOptimizer

DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


class IdleSGD(torch.optim.SGD):
    """Param groups with a learning rate and no work of its own."""

    def step(self, closure=None):
        return None


def setup(dtype):
    with torch.device("meta"):
        shapes = [p.shape for p in build_model(LLAMA3_8B).parameters()]
    gen = torch.Generator(device="cuda").manual_seed(0)
    params = [
        torch.nn.Parameter(
            torch.randn(s, generator=gen, device="cuda", dtype=dtype) * 0.02)
        for s in shapes
    ]
    for p in params:  # the averager takes the parameters that have one
        p.grad = torch.zeros_like(p)
    opt = SlowMomentumOptimizer(IdleSGD(params, lr=0.1), slowmo_freq=1,
                                slowmo_factor=0.5, slowmo_lr=1.0)
    opt.step()  # the first call averages without an outer update
    return params, opt


def run(opt, fused, steps):
    opt.use_fused = fused
    for _ in range(steps):
        opt.step()


def bench(label, dtype, steps, repeats):
    params, opt = setup(dtype)
    numel = sum(p.numel() for p in params)
    for fused in (False, True):  # state, flat buffer, code objects
        run(opt, fused, 2)
    times = {False: [], True: []}
    for _ in range(repeats):
        for fused in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(opt, fused, steps)
            torch.cuda.synchronize()
            times[fused].append((time.perf_counter() - t0) / steps * 1e3)
    assert opt._fused_outer_steps == 2 + steps * repeats
    print(f"| {label} | {len(params)} | {numel / 1e9:.2f} G |", end="")
    for fused in (False, True):
        t = sorted(times[fused])
        print(f" {t[len(t) // 2]:.2f} ({t[0]:.2f} .. {t[-1]:.2f}) |", end="")
    med = {f: sorted(t)[len(t) // 2] for f, t in times.items()}
    # Minimum traffic of the fused step: pack reads p and writes flat; the
    # outer step reads flat, prev and m and writes m, prev and p.
    esz = params[0].element_size()
    bytes_fused = numel * (5 * esz + 8 + esz)
    print(f" {med[False] / med[True]:.2f}x |"
          f" {bytes_fused / (med[True] * 1e-3) / 1e12:.2f} TB/s |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--count", default=None,
                    help="eager=N,fused=M: run that many steps and exit")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_PORT", str(s.getsockname()[1]))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        if args.count is not None:
            counts = dict(kv.split("=") for kv in args.count.split(","))
            _, opt = setup(DTYPES[args.dtypes.split(",")[0]])
            run(opt, False, int(counts.get("eager", 0)))
            run(opt, True, int(counts.get("fused", 0)))
            torch.cuda.synchronize()
            return
        print("| dtype | tensors | elements | eager ms/step, median (min .. "
              "max) | fused ms/step, median (min .. max) | eager / fused |"
              " fused, minimum traffic over time |")
        print("|---|---|---|---|---|---|---|")
        for name in args.dtypes.split(","):
            bench(name, DTYPES[name], args.steps, args.repeats)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
