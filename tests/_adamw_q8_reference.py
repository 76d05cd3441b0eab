# fp64 reference, quantizer and bound checker for the block-scaled fp8
# AnyPrecisionAdamW step (csrc/hip/anyprecision_adamw_q8.hip), on top of
# tests/_adamw_reference.py. Stored fp8 inputs dequantize as code.double()
# * scale per block, reference_step gives the exact outputs; the bounds are
# those of docs/anyprecision_adamw.md, "What is checked".

import collections

import torch

from tests._adamw_reference import (
    _FORMAT, K_ROUNDINGS, MAX_K_NEEDED, _check_one, reference_step, ulp)

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
# (FMAX, exponent of FMAX = 1.75 * 2^top, precision bits, emin)
FP8 = {E4M3: (448.0, 8, 4, -6), E5M2: (57344.0, 15, 3, -14)}
_FORMAT.update({d: f[2:] for d, f in FP8.items()})  # for ulp(t, fp8 dtype)
QBLOCK = 256
MIN_EXP = -100
_CHUNK = 1 << 22  # a multiple of QBLOCK


def _blocks(x, fill=0.0):
    """x padded to whole quant blocks, as (n_blocks, QBLOCK)."""
    pad = -x.numel() % QBLOCK
    x = torch.nn.functional.pad(x, (0, pad), value=fill)
    return x.view(x.numel() // QBLOCK, QBLOCK)


def scale_exponent(absmax, dtype):
    """Smallest e with absmax * 2^-e <= FMAX, clamped at MIN_EXP; 0 for a
    zero absmax. absmax: finite non-negative fp64 tensor."""
    top = FP8[dtype][1]
    f, e = torch.frexp(absmax)  # absmax = 2f * 2^(e - 1), 2f in [1, 2)
    e = e - 1 - top + (2 * f > 1.75).to(e.dtype)
    e = e.clamp(min=MIN_EXP)
    return torch.where(absmax == 0, torch.zeros_like(e), e)


def per_element(scale, n):
    return scale.double().repeat_interleave(QBLOCK)[:n]


def dequantize(codes, scale):
    return codes.double() * per_element(scale, codes.numel())


def quantize(x, dtype, variance):
    """The format's quantizer on finite fp32 values: (codes, scales)."""
    x = x.double()
    e = scale_exponent(_blocks(x.abs()).amax(dim=1), dtype)
    scale = torch.ldexp(torch.ones_like(e, dtype=torch.float64), e)
    t = x / per_element(scale, x.numel())
    codes = t.to(torch.float32).to(dtype)
    if variance:
        bits = codes.view(torch.uint8)
        bits[(x > 0) & (bits == 0)] = 1
    return codes, scale.to(torch.float32)


def _check_fp8(name, codes, scale, exact, mag, k, where):
    """Returns (K needed, [failure messages]) of one fp8 state chunk."""
    fmax, _, bits, emin = FP8[codes.dtype]
    n = exact.numel()
    fails = []
    tol = k * 2.0**-24 * mag
    finite_block = _blocks(exact, 0.0).isfinite().all(dim=1)
    safe = torch.where(exact.isfinite(), exact.abs(), torch.zeros_like(exact))
    safe_tol = torch.where(exact.isfinite(), tol, torch.zeros_like(tol))
    e_lo = scale_exponent(_blocks((safe - safe_tol).clamp(min=0)).amax(dim=1),
                          codes.dtype)
    e_hi = scale_exponent(_blocks(safe + safe_tol).amax(dim=1), codes.dtype)
    e_lo = torch.where(finite_block, e_lo, torch.zeros_like(e_lo))
    e_hi = torch.where(finite_block, e_hi, torch.zeros_like(e_hi))
    f, e = torch.frexp(scale.double())
    bad = (f != 0.5) | (e - 1 < e_lo) | (e - 1 > e_hi)
    if bad.any():
        b = int(bad.nonzero()[0])
        fails.append(f"{where}: {name}_scale[{b}]={float(scale[b])!r}: "
                     f"exponent not in {int(e_lo[b])}..{int(e_hi[b])}")
    s = per_element(scale, n)
    out = codes.double() * s
    if not torch.equal(out.isfinite(), exact.isfinite()):
        fails.append(f"{where}: {name}: non-finite mask differs")
    tiny, zero = 2.0 ** (emin - (bits - 1)), torch.zeros_like(exact)
    t = torch.where(exact.isfinite(), exact / s, zero).clamp(-fmax, fmax)
    if name == "exp_avg_sq":
        t = torch.where((t > 0) & (t < tiny), torch.full_like(t, tiny), t)
    ok = exact.isfinite() & out.isfinite()
    err = torch.where(ok, (out - t * s).abs(), zero)
    half = torch.where(ok, 0.5 * ulp(t, codes.dtype) * s, zero)
    unit = torch.where(ok, mag, zero) * 2.0**-24
    excess = err - half
    needed = torch.where(excess > 0, excess / unit, zero)
    k_needed = float(needed.max()) if n else 0.0
    if k_needed > k:
        w = int(needed.argmax())
        fails.append(
            f"{where}: {name} ({codes.dtype}): worst at {w}: "
            f"out={float(out[w])!r} exact={float(exact[w])!r} "
            f"scale={float(s[w])!r} needs K={k_needed:.1f}")
    return k_needed, fails


def check_q8_step(before, after, scalars, k=K_ROUNDINGS, where=""):
    """before = (p, g, m, m_scale, v, v_scale, c), after = (p, m, m_scale,
    v, v_scale, c); a scale is None for a state that is not fp8, c is None
    without Kahan. Asserts every bound; returns {output: K needed}."""
    p0, g0, m0, ms0, v0, vs0, c0 = before
    p1, m1, ms1, v1, vs1, c1 = after
    n = p0.numel()
    needed = collections.defaultdict(float)
    failures = []
    for lo in range(0, n, _CHUNK):
        hi = min(lo + _CHUNK, n)
        sl, bl = slice(lo, hi), slice(lo // QBLOCK, -(-hi // QBLOCK))
        m0d = m0[sl] if ms0 is None else dequantize(m0[sl], ms0[bl])
        v0d = v0[sl] if vs0 is None else dequantize(v0[sl], vs0[bl])
        c0s = None if c0 is None else c0[sl]
        ex = reference_step(p0[sl], g0[sl], m0d, v0d, c0s, scalars)
        c_abs = 0.0 if c0 is None else c0s.double().abs()
        mag_p = ex.p_decayed.abs() + c_abs + ex.update.abs()
        tag = f"{where}[{lo}:]"
        results = [("param",) + _check_one("param", p1[sl], ex.p, mag_p, k,
                                           tag)]
        if c0 is not None:
            c_ref = ex.p - p1[sl].double()
            results.append(("compensation",) + _check_one(
                "compensation", c1[sl], c_ref, mag_p, k, tag))
        for name, out, scale, exact, mag in (
                ("exp_avg", m1, ms1, ex.m, m0d.double().abs()
                 + g0[sl].double().abs()),
                ("exp_avg_sq", v1, vs1, ex.v, ex.v)):
            if scale is None:
                results.append((name,) + _check_one(name, out[sl], exact,
                                                    mag, k, tag))
            else:
                kn, fails = _check_fp8(name, out[sl], scale[bl], exact, mag,
                                       k, tag)
                results.append((name + "(fp8)", kn, "\n".join(fails) or None))
        for name, kn, msg in results:
            needed[name] = max(needed[name], kn)
            if msg:
                failures.append(msg)
    for name, kn in needed.items():
        if kn >= MAX_K_NEEDED.get(name, (0.0, ""))[0]:
            MAX_K_NEEDED[name] = (kn, where)
    assert not failures, "\n".join(failures)
    return dict(needed)
