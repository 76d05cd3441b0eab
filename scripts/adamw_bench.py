"""A/B of the AnyPrecisionAdamW step on GPU: eager op-sequence vs fused
CDNA4 kernel, on the flagship dtype layout (bf16 params/grad/variance/comp,
fp32 momentum, Kahan on).

Modes (arguments; default "step" and "clip"): "step" is the A/Bs of the
step kernels, "clip" compares clip_grad_norm_ followed by the fused step
with the fused max_grad_norm step and times the gradient norm kernels alone,
"sr" is the layout table alone (the stochastic-rounding rows next to the
layouts they are compared with), every row measured twice."""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import time

import torch

from torchdistx_amd.optimizers import AnyPrecisionAdamW

assert torch.cuda.is_available()
MODES = sys.argv[1:] or ["step", "clip"]
assert set(MODES) <= {"step", "clip", "sr"}, MODES
n = 1 << 28  # 268M params (~0.5 GB bf16)


def bench(use_fused, steps=10):
    torch.manual_seed(0)
    p = torch.nn.Parameter(torch.randn(n, device="cuda", dtype=torch.bfloat16))
    opt = AnyPrecisionAdamW(
        [p], lr=1e-3, weight_decay=0.01, use_kahan_summation=True,
        momentum_dtype=torch.float32, variance_dtype=torch.bfloat16,
        compensation_buffer_dtype=torch.bfloat16, use_fused=use_fused,
    )
    p.grad = torch.randn_like(p)
    opt.step()  # init state + warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    # bytes: p r/w (2+2) g r (2) m r/w (4+4) v r/w (2+2) c r/w (2+2) = 22 B/elem
    tbps = 22.0 * n / dt / 1e12
    return dt * 1e3, tbps


for name, fused in (("eager", False), ("fused", True)) * ("step" in MODES):
    ms, tb = bench(fused)
    print(f"{name}: {ms:8.2f} ms/step  effective {tb:5.2f} TB/s")


def bench_many_small(use_batched, n_tensors=512, numel=16384, steps=10):
    """Launch-overhead regime: hundreds of small params per step."""
    torch.manual_seed(1)
    params = [
        torch.nn.Parameter(
            torch.randn(numel, device="cuda", dtype=torch.bfloat16)
        )
        for _ in range(n_tensors)
    ]
    import torchdistx_amd.optimizers.anyprecision_optimizer as apo

    saved = apo._BATCH_MAX_NUMEL
    apo._BATCH_MAX_NUMEL = (1 << 20) if use_batched else 0
    try:
        opt = AnyPrecisionAdamW(
            params, lr=1e-3, weight_decay=0.01, use_kahan_summation=True,
            momentum_dtype=torch.float32, variance_dtype=torch.bfloat16,
            compensation_buffer_dtype=torch.bfloat16,
        )
        for p in params:
            p.grad = torch.randn_like(p)
        opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    finally:
        apo._BATCH_MAX_NUMEL = saved


for name, batched in ((("per-tensor fused", False), ("batched", True))
                      * ("step" in MODES)):
    ms = bench_many_small(batched)
    print(f"512x16k params, {name}: {ms:8.2f} ms/step")


# ---------------------------------------------------------------------------
# Block-scaled fp8 states (csrc/hip/anyprecision_adamw_q8.hip): bf16 p/g,
# e4m3fn momentum, e5m2 variance, without and with bf16 Kahan, next to the
# fused flagship layout measured the same way in the same process. Each
# figure is the median of `repeats` timings of `steps` steps.
# ---------------------------------------------------------------------------

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
SCALES = 8.0 / 256  # two fp32 scales read and written per 256 elements
CONFIGS = {
    # name: (momentum, variance, kahan, bytes per element[, stochastic
    # rounding of the bf16 parameter])
    "flagship fused (f32 m, bf16 v, kahan)": (
        torch.float32, torch.bfloat16, True, 22.0),
    "flagship fused (f32 m, bf16 v, no kahan)": (
        torch.float32, torch.bfloat16, False, 18.0),
    "q8 (e4m3 m, e5m2 v, no kahan)": (E4M3, E5M2, False, 10.0 + SCALES),
    "q8 (e4m3 m, e5m2 v, kahan)": (E4M3, E5M2, True, 14.0 + SCALES),
    # Stochastic rounding: no compensation buffer; any state layout takes
    # the multi-tensor kernel of anyprecision_adamw_q8.hip.
    "sr (f32 m, bf16 v)": (torch.float32, torch.bfloat16, False, 18.0, True),
    "sr q8 (e4m3 m, e5m2 v)": (E4M3, E5M2, False, 10.0 + SCALES, True),
}


def timed(opt, steps, repeats):
    opt.step()  # state + warm-up
    opt.step()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            opt.step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / steps * 1e3)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def bench_layout(sizes, config, steps=10, repeats=5):
    m_dt, v_dt, kahan, _, *sr = config
    torch.manual_seed(2)
    params = [
        torch.nn.Parameter(
            torch.randn(k, device="cuda", dtype=torch.bfloat16))
        for k in sizes
    ]
    opt = AnyPrecisionAdamW(
        params, lr=1e-3, weight_decay=0.01, use_kahan_summation=kahan,
        momentum_dtype=m_dt, variance_dtype=v_dt,
        compensation_buffer_dtype=torch.bfloat16, use_fused=True,
        **(dict(stochastic_rounding=True, stochastic_rounding_seed=4)
           if sr else {}),
    )
    for p in params:
        p.grad = torch.randn_like(p)
    result = timed(opt, steps, repeats)
    assert opt._fused_steps == len(params) * (2 + steps * repeats)
    return result


SHAPES = (("2^28 elements", [n]), ("512x16k", [16384] * 512))

for label, sizes in SHAPES * ("step" in MODES or "sr" in MODES):
    # The flagship layouts twice: the second pass is their run-to-run
    # spread under the same conditions.
    for name in (list(CONFIGS) + list(CONFIGS)[:2] if "step" in MODES
                 else list(CONFIGS) * 2):
        med, lo, hi = bench_layout(sizes, CONFIGS[name])
        tb = CONFIGS[name][3] * sum(sizes) / (med * 1e-3) / 1e12
        print(f"{label}, {name}: median {med:8.3f} ms/step "
              f"(min {lo:.3f}, max {hi:.3f})  effective {tb:5.2f} TB/s")


# ---------------------------------------------------------------------------
# Gradient clipping (csrc/hip/grad_norm.hip), flagship Kahan layout, bf16
# gradients of norm sqrt(numel) clipped to 1.0:
#   (a) torch.nn.utils.clip_grad_norm_, then the fused step;
#   (b) AnyPrecisionAdamW(max_grad_norm=1.0), fused.
# Windows of (a), (b) and (a) again alternate; the two (a) columns are the
# run-to-run spread. Then the norm call alone (both kernels and the table
# copy, timed from the host around a synchronise) against a device copy of
# the same tensor, which moves twice the bytes.
# ---------------------------------------------------------------------------


def windows(fns, steps=10, repeats=5):
    """Median, min and max ms/call of each fn; windows alternate."""
    for fn in fns:
        fn()
        fn()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for times, fn in zip(out, fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / steps * 1e3)
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in out]


def clip_setup(sizes, max_grad_norm):
    torch.manual_seed(3)
    params = [
        torch.nn.Parameter(
            torch.randn(k, device="cuda", dtype=torch.bfloat16))
        for k in sizes
    ]
    opt = AnyPrecisionAdamW(
        params, lr=1e-3, weight_decay=0.01, use_kahan_summation=True,
        momentum_dtype=torch.float32, variance_dtype=torch.bfloat16,
        compensation_buffer_dtype=torch.bfloat16, use_fused=True,
        max_grad_norm=max_grad_norm,
    )
    for p in params:
        p.grad = torch.randn_like(p)
    return params, opt


def bench_clip(label, sizes):
    from torchdistx_amd import _kernels

    pa, opt_a = clip_setup(sizes, None)
    pb, opt_b = clip_setup(sizes, 1.0)
    pc, opt_c = clip_setup(sizes, None)

    def torch_clip(params, opt):
        def fn():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        return fn

    names = ("(a) clip_grad_norm_ + fused step", "(b) max_grad_norm fused",
             "(a) again")
    results = windows(
        [torch_clip(pa, opt_a), opt_b.step, torch_clip(pc, opt_c)])
    for name, (med, lo, hi) in zip(names, results):
        print(f"{label}, {name}: median {med:8.3f} ms/step "
              f"(min {lo:.3f}, max {hi:.3f})")
    assert opt_b.grad_clip_coef < 1

    grads = [p.grad for p in pb]
    out = torch.empty(2, device="cuda")
    src = torch.cat([g.reshape(-1) for g in grads])
    dst = torch.empty_like(src)
    nbytes = src.numel() * src.element_size()
    (norm, _, _), (copy, _, _) = windows(
        [lambda: _kernels.grad_norm_clip_coef_(grads, 1.0, out),
         lambda: dst.copy_(src)], steps=20)
    print(f"{label}, norm call alone: median {norm:8.3f} ms, "
          f"{nbytes / (norm * 1e-3) / 1e12:5.2f} TB/s read; "
          f"device copy: {copy:8.3f} ms, "
          f"{2 * nbytes / (copy * 1e-3) / 1e12:5.2f} TB/s read+write")


for label, sizes in SHAPES * ("clip" in MODES):
    bench_clip(label, sizes)
