# Builds and runs tests/cc/test_philox_mulhilo.cc with plain g++: the host
# proofs behind the normal-fill kernels' VALU trims (one-product mulhilo32,
# three-input xor, folded angle constants checked for every 16-bit and
# 24-bit input, sqrt fix-up over Box-Muller's argument range).

import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_mulhilo_cc_units(tmp_path) -> None:
    header = os.path.join(REPO, "torchdistx_amd", "csrc", "core", "philox.h")
    if not os.path.exists(header):
        pytest.skip("C++ sources not present (wheel-installed run)")
    binary = tmp_path / "test_philox_mulhilo"
    # -ffp-contract=off: the float identities are about separately rounded
    # multiplies; no fused multiply-add may stand in for them.
    build = subprocess.run(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off",
         os.path.join(REPO, "tests", "cc", "test_philox_mulhilo.cc"),
         "-o", str(binary)],
        capture_output=True, text=True, timeout=120,
    )
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(binary)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all passed" in run.stdout
