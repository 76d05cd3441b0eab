"""Step time of AnyPrecisionAdamW(capturable=True) on one GPU, next to the
existing step, in one process:

  1. the existing (non-capturable) fused step,
  2. the capturable step, eager,
  3. the capturable step as a graph replay (torch.cuda.graph),

for one tensor of 2^28 elements and for 512 tensors of 16384 elements, on
the flagship Kahan layout (fp32 momentum, bf16 variance, bf16 Kahan) and the
fp8 layout (e4m3fn momentum, e5m2 variance). Windows of the three alternate;
every figure is the median (min, max) of `--repeats` windows, wall clock
around a device synchronize after two warm-up steps. A window holds as many
steps as fill `--window` seconds at the step time a trial of `--steps` steps
gave (and at least `--steps`), so a 0.04 ms replay is timed over thousands
of steps, not ten. Everything is measured again in a second pass: the
distance between the passes is the run-to-run spread. Before timing, one
capturable step is compared with one existing step on the same inputs."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse
import time

import torch

from torchdistx_amd.optimizers import AnyPrecisionAdamW

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
LAYOUTS = {
    "flagship (f32 m, bf16 v, kahan)": (torch.float32, torch.bfloat16, True),
    "fp8 (e4m3 m, e5m2 v)": (E4M3, E5M2, False),
}
SHAPES = {"2^28 elements": [1 << 28], "512x16k": [16384] * 512}


def setup(sizes, layout, capturable):
    m_dt, v_dt, kahan = LAYOUTS[layout]
    gen = torch.Generator(device="cuda").manual_seed(2)
    params = [torch.nn.Parameter(torch.randn(
        k, device="cuda", generator=gen).to(torch.bfloat16)) for k in sizes]
    opt = AnyPrecisionAdamW(
        params, lr=1e-3, weight_decay=0.01, use_kahan_summation=kahan,
        momentum_dtype=m_dt, variance_dtype=v_dt,
        compensation_buffer_dtype=torch.bfloat16, use_fused=True,
        capturable=capturable)
    for p in params:
        p.grad = torch.randn(p.numel(), device="cuda",
                             generator=gen).to(torch.bfloat16)
    return params, opt


def same_update(a, b):
    """Largest difference of the parameters, in bf16 ulps of the larger
    value: the capturable step's scalars may differ from the host's by one
    fp32 ulp, which a bf16 parameter shows as at most one code."""
    worst = 0.0
    for p, q in zip(a, b):
        d = (p.detach().float() - q.detach().float()).abs()
        mag = torch.maximum(p.detach().float().abs(),
                            q.detach().float().abs()).clamp(min=1e-30)
        worst = max(worst, float((d / (mag * 2.0**-8)).max()))
    return worst


def window(fn, steps):
    """ms per call over one window of `steps` calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def windows(fns, steps, repeats, seconds):
    """Per fn: (median, min, max) ms per call and the steps per window."""
    per_window = [max(steps, int(seconds * 1e3 / window(fn, steps)) + 1)
                  for fn in fns]
    out = [[] for _ in fns]
    for _ in range(repeats):
        for times, fn, k in zip(out, fns, per_window):
            times.append(window(fn, k))
    return [(sorted(t)[len(t) // 2], min(t), max(t), k)
            for t, k in zip(out, per_window)]


def bench(shape, layout, steps, repeats, seconds):
    sizes = SHAPES[shape]
    pa, plain = setup(sizes, layout, False)
    pb, eager = setup(sizes, layout, True)
    pc, replayed = setup(sizes, layout, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for opt in (plain, eager, replayed):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    print(f"{shape}, {layout}: capturable vs existing after one step, "
          f"largest parameter difference {same_update(pa, pb):.2f} bf16 ulp")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.step()
    fns = [plain.step, eager.step, graph.replay]
    for fn in fns:
        fn()
    names = ("existing step", "capturable, eager", "capturable, replay")
    results = windows(fns, steps, repeats, seconds)
    for name, (med, lo, hi, k) in zip(names, results):
        print(f"{shape}, {layout}, {name}: median {med:8.3f} ms/step "
              f"(min {lo:.3f}, max {hi:.3f}; {k} steps per window)",
              flush=True)
    # Two warm-up steps, the trial, the windows.
    done = [2 + steps + repeats * k for _, _, _, k in results]
    assert plain._fused_steps == len(sizes) * done[0]
    assert eager._fused_steps == len(sizes) * done[1]
    assert all(replayed.state[p]["step"].item() == done[2] for p in pc[:2])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25,
                    help="least seconds of work per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for pass_ in ("first pass", "second pass"):
        print(f"--- {pass_}")
        for shape in SHAPES:
            for layout in LAYOUTS:
                bench(shape, layout, args.steps, args.repeats, args.window)


if __name__ == "__main__":
    main()
