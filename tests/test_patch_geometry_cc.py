# Builds and runs tests/cc/test_patch_geometry.cc with plain g++, the way
# test_box_geometry_cc.py does for the box normalizer: rowsMeeting is
# header-only and shared by the CPU reference of tdx::patch_box_ and the
# CDNA4 patch kernel's launcher.

import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_patch_geometry_cc_units(tmp_path) -> None:
    import pytest

    header = os.path.join(
        REPO, "torchdistx_amd", "csrc", "core", "box_geometry.h"
    )
    source = os.path.join(REPO, "tests", "cc", "test_patch_geometry.cc")
    if not os.path.exists(os.path.dirname(header)):
        pytest.skip("C++ sources not present (wheel-installed run)")
    binary = tmp_path / "test_patch_geometry"
    build = subprocess.run(
        ["g++", "-O2", "-std=c++17", source, "-o", str(binary)],
        capture_output=True, text=True, timeout=120,
    )
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(binary)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all passed" in run.stdout
