# Builds and runs tests/cc/test_box_geometry.cc with plain g++, the way
# test_cc_units.py does for the Philox header: the box normalizer and the
# multiply-shift divisor are header-only and shared by the planner, the
# CPU reference op and the CDNA4 box kernel.

import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_box_geometry_cc_units(tmp_path) -> None:
    import pytest

    header = os.path.join(
        REPO, "torchdistx_amd", "csrc", "core", "box_geometry.h"
    )
    source = os.path.join(REPO, "tests", "cc", "test_box_geometry.cc")
    if not os.path.exists(os.path.dirname(header)):
        pytest.skip("C++ sources not present (wheel-installed run)")
    binary = tmp_path / "test_box_geometry"
    build = subprocess.run(
        ["g++", "-O2", "-std=c++17", source, "-o", str(binary)],
        capture_output=True, text=True, timeout=120,
    )
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(binary)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all passed" in run.stdout
