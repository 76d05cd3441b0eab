# fp64 reference and error-bound checker for the fused AnyPrecisionAdamW
# kernels (csrc/hip/anyprecision_adamw.hip), plus the shared input
# generator. A plain helper module: tests/test_adamw_reference.py proves
# the checker on the CPU, tests/test_adamw_fused_gpu.py applies it to the
# HIP kernels.
#
# Scalar contract: lr, beta1, beta2, eps, weight_decay, step_size,
# bias_correction2_sqrt and the three host-computed complements
# (1 - beta1, 1 - beta2, 1 - lr * weight_decay, each formed in double) are
# narrowed to fp32 once. From there the reference is exact (fp64)
# arithmetic on the inputs exactly as stored, so any deviation of a kernel
# is its fp32 rounding plus one rounding to the storage dtype:
#
#   |out - exact| <= 1/2 ulp_T(exact) + K * 2^-24 * mag
#
# with mag the sum of magnitudes entering that output and K a count of
# fp32 roundings (the longest chain, to p'/c', has about 12).

import collections
import dataclasses
import types

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16

# Count of fp32 roundings allowed on top of the storage rounding. Not a
# tuned tolerance: see the header.
K_ROUNDINGS = 32

# Largest K any checked output has needed so far in this process, per
# output name, with the label of the check that needed it; and the same
# over the checks that stayed inside their bound.
MAX_K_NEEDED = {}
MAX_K_WITHIN_BOUND = {}

# (precision bits incl. the hidden one, exponent of the smallest normal)
_FORMAT = {F32: (24, -126), BF16: (8, -126), F16: (11, -14)}

# Elements per reference chunk: bounds the fp64 temporaries of the large
# grid-wrap cases.
_CHUNK = 1 << 22


def narrow(x: float) -> float:
    """The fp32 value nearest to the double x, as a double."""
    return torch.tensor(x, dtype=torch.float64).to(F32).item()


@dataclasses.dataclass(frozen=True)
class Scalars:
    lr: float
    beta1: float
    beta2: float
    eps: float
    weight_decay: float
    step_size: float
    bias_correction2_sqrt: float

    @classmethod
    def for_step(cls, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0):
        # As AnyPrecisionAdamW.step forms them.
        beta1, beta2 = betas
        return cls(lr, beta1, beta2, eps, weight_decay,
                   lr / (1 - beta1**step), (1 - beta2**step) ** 0.5)

    def kernel_args(self):
        return (self.lr, self.beta1, self.beta2, self.eps,
                self.weight_decay, self.step_size,
                self.bias_correction2_sqrt)

    def narrowed(self):
        return types.SimpleNamespace(
            beta2=narrow(self.beta2),
            eps=narrow(self.eps),
            weight_decay=narrow(self.weight_decay),
            step_size=narrow(self.step_size),
            bias_correction2_sqrt=narrow(self.bias_correction2_sqrt),
            one_minus_beta1=narrow(1.0 - self.beta1),
            one_minus_beta2=narrow(1.0 - self.beta2),
            decay=narrow(1.0 - self.lr * self.weight_decay),
        )


Exact = collections.namedtuple("Exact", "p m v update p_decayed")


def reference_step(p, g, m, v, c, scalars):
    """Exact p', m', v', update and decayed p of one step, in fp64 on the
    inputs' device. c is the compensation buffer or None."""
    s = scalars.narrowed()
    p64, g64, m64, v64 = (t.to(torch.float64) for t in (p, g, m, v))
    p_decayed = p64 * s.decay if s.weight_decay != 0.0 else p64
    m_new = m64 + s.one_minus_beta1 * (g64 - m64)
    v_new = v64 * s.beta2 + g64 * g64 * s.one_minus_beta2
    denom = v_new.sqrt() / s.bias_correction2_sqrt + s.eps
    update = -s.step_size * (m_new / denom)
    p_new = p_decayed + update
    if c is not None:
        p_new = p_new + c.to(torch.float64)
    return Exact(p_new, m_new, v_new, update, p_decayed)


def ulp(exact, dtype):
    """Spacing of dtype at |exact| (fp64 tensor), floored at the subnormal
    spacing. Meaningless where exact is not finite."""
    bits, emin = _FORMAT[dtype]
    _, e = torch.frexp(exact.abs())  # |x| = f * 2^e, f in [0.5, 1)
    e = torch.where(exact == 0, torch.full_like(e, emin), e - 1)
    e = e.clamp_(min=emin) - (bits - 1)
    return torch.ldexp(torch.ones_like(exact), e)


def _check_one(name, out, exact, mag, k, where):
    """Returns (K needed, failure message or None) of one output."""
    out64 = out.to(torch.float64)
    if not torch.equal(out64.isnan(), exact.isnan()):
        return 0.0, f"{where}: {name}: nan mask differs from the reference"
    pinf = torch.equal(out64 == float("inf"), exact == float("inf"))
    ninf = torch.equal(out64 == -float("inf"), exact == -float("inf"))
    if not (pinf and ninf):
        return 0.0, f"{where}: {name}: inf mask differs from the reference"
    finite = exact.isfinite()
    zero = torch.zeros_like(exact)
    err = torch.where(finite, (out64 - exact).abs(), zero)
    half = torch.where(finite, 0.5 * ulp(exact, out.dtype), zero)
    unit = torch.where(finite, mag, zero) * 2.0**-24
    excess = err - half
    # mag == 0 leaves only the storage rounding: any excess needs K = inf.
    needed = torch.where(excess > 0, excess / unit, zero)
    if needed.numel() == 0:
        return 0.0, None
    worst = int(needed.argmax())
    k_needed = float(needed[worst])
    if k_needed <= k:
        return k_needed, None
    n_bad = int((needed > k).sum())
    return k_needed, (
        f"{where}: {name} ({out.dtype}): {n_bad} of {needed.numel()} "
        f"elements outside 1/2 ulp + {k} * 2^-24 * mag; worst at chunk "
        f"index {worst}: out={float(out64[worst])!r} "
        f"exact={float(exact[worst])!r} err={float(err[worst]):.3e} "
        f"half_ulp={float(half[worst]):.3e} mag={float(mag[worst]):.3e} "
        f"needs K={k_needed:.1f}")


def check_step(before, after, scalars, k=K_ROUNDINGS, where=""):
    """Asserts the bound for one step of one tensor.

    before = (p, g, m, v, c) as stored before the step (c None without
    Kahan), after = (p, m, v, c) as the code under test left them. Returns
    {output name: K needed} and folds it into MAX_K_NEEDED.
    """
    p0, g0, m0, v0, c0 = before
    p1, m1, v1, c1 = after
    assert (c0 is None) == (c1 is None)
    n = p0.numel()
    needed = collections.defaultdict(float)
    failures = []
    for lo in range(0, n, _CHUNK):
        sl = slice(lo, min(lo + _CHUNK, n))
        c0s = None if c0 is None else c0[sl]
        ex = reference_step(p0[sl], g0[sl], m0[sl], v0[sl], c0s, scalars)
        c_abs = 0.0 if c0 is None else c0s.to(torch.float64).abs()
        mag_p = ex.p_decayed.abs() + c_abs + ex.update.abs()
        checks = [
            ("exp_avg", m1[sl], ex.m,
             m0[sl].to(torch.float64).abs() + g0[sl].to(torch.float64).abs()),
            ("exp_avg_sq", v1[sl], ex.v, ex.v),
            ("param", p1[sl], ex.p, mag_p),
        ]
        if c0 is not None:
            # The compensation is a cancellation residual that flips when
            # p' rounds the other way at a tie, so it is checked against
            # the parameter the code under test itself stored.
            c_ref = ex.p - p1[sl].to(torch.float64)
            checks.append(("compensation", c1[sl], c_ref, mag_p))
        for name, out, exact, mag in checks:
            kn, msg = _check_one(name, out, exact, mag, k,
                                 f"{where}[{lo}:]")
            needed[name] = max(needed[name], kn)
            if msg is not None:
                failures.append(msg)
    for name, kn in needed.items():
        for record in (MAX_K_NEEDED,) + (
                (MAX_K_WITHIN_BOUND,) if kn <= k else ()):
            if kn >= record.get(name, (0.0, ""))[0]:
                record[name] = (kn, where)
    assert not failures, "\n".join(failures)
    return dict(needed)


# ---------------------------------------------------------------------------
# Dtype layouts (param, grad, exp_avg, exp_avg_sq, compensation or None)
# ---------------------------------------------------------------------------

_THREE = (F32, BF16, F16)
FLAGSHIP = (BF16, BF16, F32, BF16, BF16)
ALL_F32 = (F32, F32, F32, F32, None)

NO_KAHAN_LAYOUTS = [
    (pd, gd, md, vd, None)
    for pd in _THREE for gd in _THREE for md in _THREE for vd in _THREE
]
KAHAN_LAYOUTS = (
    [FLAGSHIP[:4] + (cd,) for cd in _THREE]
    + [(d, d, d, d, cd) for d in _THREE for cd in _THREE]
    + [
        (F32, BF16, F32, F32, BF16),
        (BF16, F32, BF16, F32, F32),
        (F16, BF16, F32, BF16, F32),
        (BF16, F16, F32, F16, BF16),
        (F32, F32, BF16, BF16, F16),
    ]
)
DTYPE_MATRIX = NO_KAHAN_LAYOUTS + KAHAN_LAYOUTS


def layout_id(layout):
    short = {F32: "f32", BF16: "bf16", F16: "f16", None: "nokahan"}
    return "-".join(short[d] for d in layout)


# ---------------------------------------------------------------------------
# Inputs: views into guarded buffers
# ---------------------------------------------------------------------------

# Guard elements on each side of every operand; a multiple of 8 so a view
# at offset 0 keeps the buffer's 16-byte alignment for every dtype.
GUARD = 64
OPERANDS = ("p", "g", "m", "v", "c")


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Case:
    """The five operands of one tensor's step as views into larger
    buffers whose guard elements carry a NaN sentinel, with a snapshot of
    everything before the step."""

    def __init__(self, n, layout, first_step, device, seed, misalign=(),
                 grad_overrides=None):
        gen = torch.Generator(device=device).manual_seed(seed)
        sigma = 1.0 if F16 in layout else 3.0

        def randn():
            return torch.randn(n, generator=gen, device=device,
                               dtype=torch.float32)

        p = randn() * torch.exp(sigma * randn())
        g = 1e-2 * randn() * torch.exp(sigma * randn())
        g[::7] = 0.0
        # (index, value) pairs written into the gradient before storing.
        for index, value in grad_overrides or ():
            g[index] = value
        c = 1e-3 * p * randn()
        if first_step:
            m = torch.zeros_like(p)
            v = torch.zeros_like(p)
        else:
            # Momentum and variance share one log-normal scale, as real
            # optimizer state does, so |m| / sqrt(v) stays O(1).
            scale = 1e-2 * torch.exp(sigma * randn())
            m = scale * randn()
            v = scale * scale * (0.5 + randn() ** 2)
        self.layout = layout
        self.n = n
        self.buffers = {}
        self.views = {}
        self.offsets = {}
        for name, dtype, val in zip(OPERANDS, layout, (p, g, m, v, c)):
            if dtype is None:
                self.views[name] = None
                continue
            off = GUARD + (1 if name in misalign else 0)
            buf = torch.full((off + n + GUARD,), float("nan"),
                             device=device, dtype=dtype)
            buf[off:off + n] = val.to(dtype)
            self.buffers[name] = buf
            self.offsets[name] = off
            self.views[name] = buf[off:off + n]
        self.snapshot = {k: b.clone() for k, b in self.buffers.items()}

    def operands(self):
        return tuple(self.views[k] for k in OPERANDS)

    def before(self):
        """(p, g, m, v, c) as stored before the step."""
        out = []
        for k in OPERANDS:
            if self.views[k] is None:
                out.append(None)
            else:
                off = self.offsets[k]
                out.append(self.snapshot[k][off:off + self.n])
        return tuple(out)

    def after(self):
        v = self.views
        return (v["p"], v["m"], v["v"], v["c"])

    def assert_guards_and_grad_intact(self, where=""):
        for k, buf in self.buffers.items():
            now, was = _bits(buf), _bits(self.snapshot[k])
            if k == "g":
                assert torch.equal(now, was), f"{where}: grad was written"
                continue
            off = self.offsets[k]
            assert torch.equal(now[:off], was[:off]), (
                f"{where}: guard before {k} was written")
            assert torch.equal(now[off + self.n:], was[off + self.n:]), (
                f"{where}: guard after {k} was written")

    def check(self, scalars, where="", k=K_ROUNDINGS):
        self.assert_guards_and_grad_intact(where)
        return check_step(self.before(), self.after(), scalars, k=k,
                          where=where)
