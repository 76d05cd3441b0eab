# Pins tdx::normal_'s seeded output bit for bit to digests recorded on the
# MI355X (tests/data/normal_fill_goldens.json, written by
# scripts/record_normal_goldens.py on the commit named inside it). Any
# change to the normal-fill kernels must reproduce every digest: sha256
# over the raw bytes for the small shapes (sub-group sizes, one-thread
# tail, grid-stride plus tail; bf16, f16 and f32), and a 64-bit
# order-sensitive checksum for a 2^26-element bf16 fill and a
# 2^30-element f32 fill, which between them draw every 16-bit and every
# 24-bit input of the log/sqrt and sin/cos stages many times over.

import importlib.util
import json
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = os.path.join(REPO, "tests", "data", "normal_fill_goldens.json")

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(),
                       reason="normal-fill goldens are MI355X bits: no GPU"),
]


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_normal_goldens",
        os.path.join(REPO, "scripts", "record_normal_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _recorder()

with open(GOLDENS) as f:
    RECORD = json.load(f)


def test_goldens_file_names_its_origin() -> None:
    assert len(RECORD["commit"]) == 40
    assert RECORD["device"]
    expected = {rec.case_id(c)
                for c in rec.small_cases() + rec.coverage_cases()}
    assert set(RECORD["digests"]) == expected


@pytest.mark.parametrize("case", rec.small_cases(), ids=rec.case_id)
def test_small_fill_matches_golden(case) -> None:
    got = rec.sha256_of(rec.fill(case))
    assert got == RECORD["digests"][rec.case_id(case)]


@pytest.mark.parametrize("case", rec.coverage_cases(), ids=rec.case_id)
def test_coverage_fill_matches_golden(case) -> None:
    got = rec.checksum_of(rec.fill(case))
    assert got == RECORD["digests"][rec.case_id(case)]
