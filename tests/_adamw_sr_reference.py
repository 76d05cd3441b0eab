# Reference of the stochastic rounding of bf16 parameters in the fused
# AnyPrecisionAdamW step (docs/anyprecision_adamw.md, "Stochastic rounding"):
# a numpy Philox4x32-10 with the counter and key mapping of
# csrc/core/philox.h, the 16 random bits of every element, and the integer
# rounding recipe. A plain helper module.

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox10(seed, subsequence, offset):
    """(x, y, z, w) as uint64 arrays holding 32-bit words, for an array of
    64-bit offsets. Key = seed, counter = (offset lo, offset hi, subsequence
    lo, subsequence hi)."""
    offset = np.asarray(offset, dtype=np.uint64)
    full = np.full_like(offset, 0)
    x, y = offset & _LOW, offset >> _S32
    z = full + np.uint64(subsequence & 0xFFFFFFFF)
    w = full + np.uint64(subsequence >> 32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = _M0 * x, _M1 * z
        x, y, z, w = ((p1 >> _S32) ^ y ^ np.uint64(k0), p1 & _LOW,
                      (p0 >> _S32) ^ w ^ np.uint64(k1), p0 & _LOW)
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return x, y, z, w


def rand16(seed, step, ordinal, i):
    """The 16 random bits of the elements with indices i of the tensor with
    this ordinal at this step, as uint32."""
    i = np.asarray(i, dtype=np.uint64)
    words = np.stack(philox10(seed, (step << 32) | ordinal, i >> np.uint64(3)))
    word = words[((i & np.uint64(7)) >> np.uint64(1)).astype(np.intp),
                 np.arange(i.size)]
    return ((word >> (np.uint64(16) * (i & np.uint64(1))))
            & np.uint64(0xFFFF)).astype(np.uint32)


def sr_code(value, rand):
    """bf16 codes (uint16) of fp32 values under the integer recipe."""
    b = np.asarray(value, dtype=np.float32).view(np.uint32).astype(np.uint64)
    exp_ones = np.uint64(0x7F800000)
    b2 = b + np.asarray(rand, dtype=np.uint64)
    code = np.where((b2 & exp_ones) == exp_ones,
                    ((b >> np.uint64(16)) & np.uint64(0x8000))
                    | np.uint64(0x7F7F), b2 >> np.uint64(16))
    # inf and NaN convert as a plain store does: inf keeps its code, a NaN
    # stays a NaN (quiet bit set so that the kept half is not an inf's).
    nonfinite = (b & exp_ones) == exp_ones
    is_nan = nonfinite & ((b & np.uint64(0x7FFFFF)) != 0)
    plain = (b >> np.uint64(16)) | np.where(is_nan, np.uint64(0x40),
                                            np.uint64(0))
    return np.where(nonfinite, plain, code).astype(np.uint16)


def sr_bounds(exact, tol, rand):
    """The codes of float32(exact - tol) and float32(exact + tol): the
    recipe is monotone in the value, so a kernel whose fp32 result is
    within tol of exact stores a value between the two, inclusive. Returns
    them as float64 values (lo, hi)."""
    exact, tol = np.asarray(exact, np.float64), np.asarray(tol, np.float64)
    out = []
    for v in (exact - tol, exact + tol):
        with np.errstate(over="ignore"):
            code = sr_code(v.astype(np.float32), rand)
        out.append((code.astype(np.uint32) << np.uint32(16))
                   .view(np.float32).astype(np.float64))
    return out[0], out[1]
