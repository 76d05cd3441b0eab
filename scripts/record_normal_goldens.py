"""Records digests of tdx::normal_'s raw output bits on one MI355X.

The output, tests/data/normal_fill_goldens.json, pins the seeded normal
fill bit for bit: tests/test_normal_fill_goldens_gpu.py recomputes every
digest below and compares for equality. Record it on the commit whose bits
are to be kept, BEFORE changing the kernel.

Small cases store a sha256 over the tensor's bytes. The two coverage cases
(2^26 bf16 elements, 2^30 f32 elements) draw every 16-bit / 24-bit input
of the log/sqrt and the sin/cos stages many times over and store a 64-bit
order-sensitive checksum computed on the GPU.

Usage: python scripts/record_normal_goldens.py [OUT.json]
"""
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "tests", "data", "normal_fill_goldens.json")

SEED, OFFSET = 20240607, 4
# Both halves of the key and of the counter non-zero.
WIDE_SEED, WIDE_OFFSET = 0x5EADBEEF00012345, (1 << 32) + 12

DTYPES = {
    "bf16": torch.bfloat16,
    "f16": torch.float16,
    "f32": torch.float32,
}
_BITS = {
    torch.bfloat16: (torch.int16, 0xFFFF),
    torch.float16: (torch.int16, 0xFFFF),
    torch.float32: (torch.int32, 0xFFFFFFFF),
}

# n = 1, 7, 8, 9: below, at and just past one 16-byte group (the
# one-thread tail); 2051: a few blocks plus a tail; 256*8*3+5: grid-stride
# plus tail.
SMALL_NS = (1, 7, 8, 9, 2051, 256 * 8 * 3 + 5)


def small_cases():
    cases = []
    for name in DTYPES:
        for n in SMALL_NS:
            cases.append(dict(dtype=name, n=n, mean=0.0, std=1.0,
                              seed=SEED, offset=OFFSET))
        cases.append(dict(dtype=name, n=2051, mean=0.25, std=0.02,
                          seed=SEED, offset=OFFSET))
        cases.append(dict(dtype=name, n=2051, mean=0.0, std=1.0,
                          seed=WIDE_SEED, offset=WIDE_OFFSET))
    return cases


def coverage_cases():
    return [
        dict(dtype="bf16", n=1 << 26, mean=0.0, std=1.0,
             seed=SEED, offset=OFFSET),
        dict(dtype="f32", n=1 << 30, mean=0.0, std=1.0,
             seed=SEED, offset=OFFSET),
    ]


def case_id(case):
    return "{dtype}-n{n}-m{mean}-s{std}-seed{seed}-off{offset}".format(**case)


def fill(case):
    import torchdistx_amd  # noqa: F401  (registers tdx:: ops)

    t = torch.empty(case["n"], dtype=DTYPES[case["dtype"]], device="cuda")
    torch.ops.tdx.normal_(t, case["mean"], case["std"], seed=case["seed"],
                          offset=case["offset"])
    return t


def sha256_of(t):
    int_dtype, _ = _BITS[t.dtype]
    return hashlib.sha256(t.view(int_dtype).cpu().numpy().tobytes()).hexdigest()


_CHUNK = 1 << 24


def checksum_of(t):
    """sum((bits[i] + 1) * (2 * i + 1)) mod 2^64, with torch integer ops on
    the GPU (int64 arithmetic wraps)."""
    int_dtype, mask = _BITS[t.dtype]
    bits = t.view(int_dtype)
    odd = torch.arange(_CHUNK, dtype=torch.int64, device=t.device) * 2 + 1
    acc = torch.zeros((), dtype=torch.int64, device=t.device)
    for start in range(0, bits.numel(), _CHUNK):
        chunk = bits[start:start + _CHUNK].to(torch.int64)
        chunk.bitwise_and_(mask).add_(1)
        chunk.mul_(odd[:chunk.numel()] + 2 * start)
        acc += chunk.sum()
    return "%016x" % (acc.item() & 0xFFFFFFFFFFFFFFFF)


def compute_all():
    digests = {}
    for case in small_cases():
        digests[case_id(case)] = sha256_of(fill(case))
    for case in coverage_cases():
        t = fill(case)
        digests[case_id(case)] = checksum_of(t)
        del t
    return digests


def _commit():
    try:
        return subprocess.run(
            ["git", "-C", REPO, "rev-parse", "HEAD"], capture_output=True,
            text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return os.environ.get("TDX_GOLDENS_COMMIT", "unknown")


def main():
    assert torch.cuda.is_available(), "recording goldens needs the GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    record = {
        "commit": _commit(),
        "device": torch.cuda.get_device_name(0),
        "digests": compute_all(),
    }
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "with", len(record["digests"]), "digests")


if __name__ == "__main__":
    main()
