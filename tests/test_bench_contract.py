# Guards the driver contract of bench.py: one JSON line on stdout with the
# agreed fields, runnable without flags on a GPU-less machine.

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, env=None):
    result = subprocess.run(
        [sys.executable, "bench.py", "--model", "tiny", "--steps", "2",
         "--warmup", "1", *extra],
        capture_output=True,
        text=True,
        timeout=300,
        cwd=REPO,
        env=env,
    )
    assert result.returncode == 0, result.stderr
    lines = [l for l in result.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, f"expected exactly one JSON line: {lines}"
    return json.loads(lines[0])


def test_bench_json_contract() -> None:
    d = _run()
    for key in (
        "metric", "value", "unit", "n_gpus", "steps", "warmup",
        "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config",
    ):
        assert key in d, key
    assert d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] in ("weak", "strong")
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["model"] == "tiny"
    assert "synthetic" in d["data"]


def test_bench_modes_report_scaling() -> None:
    assert _run("--mode", "replicate")["scaling"] == "weak"
    assert _run("--mode", "slice")["scaling"] == "strong"


@pytest.mark.gpu
def test_bench_json_contract_gpu() -> None:
    # Same contract, exercised on the GPU path (native kernels required,
    # device-memory guard, cuda synchronize bracketing).
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    d = _run()
    assert d["config"]["device"] == "cuda"
    assert d["config"]["native_init_kernels"] is True
    assert d["value"] > 0


def test_bench_full_keeps_contract() -> None:
    # --full adds measurements beyond the headline figure (none today); the
    # result line keeps its meaning.
    d = _run("--full")
    assert d["metric"] == "deferred_init_materialize_params_per_s"
    assert d["steps"] == 2 and d["value"] > 0 and d["ms_per_step"] > 0


def _load_dump(path):
    import numpy as np

    return {f[:-len(".npy")]: np.load(os.path.join(path, f))
            for f in sorted(os.listdir(path))}


_NO_GPU = {"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""}


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _check_dump_matches_last_step(tmp_path, device) -> None:
    # The dump is what the last timed step (seed 2000 + steps - 1)
    # materialized, recomputed here independently, so it is also the same
    # from run to run.
    import numpy as np
    import torch

    from torchdistx_amd import deferred_init
    from torchdistx_amd.models import CONFIGS, build_model
    from torchdistx_amd.parallel import materialize_module_distributed

    env = dict(os.environ, **_NO_GPU) if device == "cpu" else None
    d = _run("--dump-outputs", str(tmp_path), env=env)
    assert d["config"]["device"] == device.split(":")[0]
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    a = _load_dump(str(tmp_path))

    torch.manual_seed(2001)
    m = deferred_init(build_model, CONFIGS["tiny"], device=device,
                      dtype=torch.bfloat16)
    materialize_module_distributed(m, mode="replicate")
    want = dict(list(m.named_parameters()) + list(m.named_buffers()))

    assert sorted(a) == sorted(want)
    for name, t in want.items():
        assert a[name].dtype in (np.float32, np.float64), name
        assert a[name].shape == tuple(t.shape), name
        assert np.array_equal(
            a[name], t.detach().to(torch.float32).cpu().numpy()
        ), name
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000


def test_bench_dump_outputs(tmp_path) -> None:
    # The CPU path, also where a GPU is present: the benchmark process is
    # kept off it.
    _check_dump_matches_last_step(tmp_path, "cpu")


@pytest.mark.gpu
def test_bench_dump_outputs_gpu(tmp_path) -> None:
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    _check_dump_matches_last_step(tmp_path, "cuda:0")


def test_bench_dump_samples_large_outputs(tmp_path) -> None:
    # Over budget, each tensor is reduced to a fixed sample: same indices on
    # every call, edges included, total within the budget.
    import numpy as np
    import torch

    bench = _load_bench()

    big = torch.arange(100_000, dtype=torch.float32).reshape(100, 1000)
    wide = torch.arange(50_000, dtype=torch.float64)
    small = torch.ones(3, 5, dtype=torch.bfloat16)
    ints = {
        "i16": torch.tensor([-3, 0, 7], dtype=torch.int16),
        "i32": torch.tensor([[1, -2], [3, 2**24]], dtype=torch.int32),
        "flag": torch.tensor([True, False, True]),
        "i64": torch.tensor([2**40 + 1, -5], dtype=torch.int64),
    }
    named = [("big", big), ("wide", wide), ("small", small), *ints.items()]
    budget = len(named) * 16_000
    bench.dump_outputs(str(tmp_path / "a"), named, budget_bytes=budget)
    bench.dump_outputs(str(tmp_path / "b"), named, budget_bytes=budget)
    a, b = _load_dump(str(tmp_path / "a")), _load_dump(str(tmp_path / "b"))

    assert sorted(a) == sorted(n for n, _ in named)
    assert sum(v.nbytes for v in a.values()) <= budget
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert a["small"].dtype == np.float32 and a["small"].shape == (3, 5)
    assert a["big"].dtype == np.float32 and a["big"].shape == (4000,)
    assert a["wide"].dtype == np.float64 and a["wide"].shape == (2000,)
    # Integer and bool tensors keep their shape and exact values: float64
    # for int64, float32 for the narrower types.
    for name, t in ints.items():
        want = np.float64 if t.dtype == torch.int64 else np.float32
        assert a[name].dtype == want and a[name].shape == tuple(t.shape)
        assert np.array_equal(a[name], t.numpy().astype(want)), name
    # arange data: a sampled value is its own flat index.
    for name, n in (("big", 100_000), ("wide", 50_000)):
        v = a[name]
        assert v[0] == 0 and v[-1] == n - 1
        assert np.all(np.diff(v) >= 0) and np.all(v == np.round(v))
        assert len(np.unique(v)) > len(v) // 2


def test_bench_dump_default_budget_and_stale_files(tmp_path) -> None:
    # With the default budget a set of outputs far over 64 MB lands within
    # it on disk, headers included, and arrays left in DIR by an earlier
    # dump do not survive into the next one.
    import torch

    bench = _load_bench()
    out = str(tmp_path)
    bench.dump_outputs(out, [("stale", torch.ones(4))])
    assert os.listdir(out) == ["stale.npy"]

    named = [(f"w{i}", torch.full((1024, 1024), float(i))) for i in range(24)]
    named += [(f"d{i}", torch.zeros(2 ** 20, dtype=torch.float64))
              for i in range(4)]
    named += [(f"norm{i}", torch.ones(512)) for i in range(700)]
    bench.dump_outputs(out, named)

    files = sorted(os.listdir(out))
    assert files == sorted(n + ".npy" for n, _ in named)
    on_disk = sum(os.path.getsize(os.path.join(out, f)) for f in files)
    assert on_disk <= 64 * 1000 * 1000
    a = _load_dump(out)
    assert a["w3"].ndim == 1 and (a["w3"] == 3.0).all()
    assert a["norm0"].shape == (512,)


def test_bench_selftest_world1() -> None:
    result = subprocess.run(
        [sys.executable, "bench.py", "--selftest"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert result.returncode == 0, result.stderr
    d = json.loads(result.stdout.strip().splitlines()[-1])
    assert d["selftest"] == "pass", d


def test_bench_selftest_world2_torchrun() -> None:
    # Rehearses the exact launcher + rank plumbing the driver uses for
    # multi-GPU benches, over gloo on CPU: communicator creation, every
    # materialization mode's cross-rank bitwise contract, shard coverage
    # and slice reassembly at world 2. The ranks are kept off any GPU: on
    # a one-GPU machine rank 1 would otherwise ask for a second device.
    env = dict(os.environ, **_NO_GPU)
    result = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29779", "bench.py", "--selftest"],
        capture_output=True, text=True, timeout=600, cwd=REPO, env=env,
    )
    assert result.returncode == 0, result.stderr[-2000:]
    line = [l for l in result.stdout.splitlines() if '"selftest"' in l][-1]
    d = json.loads(line)
    assert d["selftest"] == "pass", d
    names = {c["name"] for c in d["checks"]}
    assert "broadcast-skewed-cross-rank" in names
    assert "shard-coverage" in names


@pytest.mark.gpu
def test_bench_selftest_world2_torchrun_gpu() -> None:
    # The same selftest with each rank on a GPU of its own, over RCCL.
    import torch

    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n < 2:
        pytest.skip(f"needs 2 GPUs, found {n}")
    result = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29781", "bench.py", "--selftest"],
        capture_output=True, text=True, timeout=600, cwd=REPO,
    )
    assert result.returncode == 0, result.stderr[-2000:]
    line = [l for l in result.stdout.splitlines() if '"selftest"' in l][-1]
    d = json.loads(line)
    assert d["selftest"] == "pass", d
    assert d["device"] == "cuda" and d["backend"] == "nccl"
    names = {c["name"] for c in d["checks"]}
    assert "broadcast-skewed-cross-rank" in names
    assert "shard-coverage" in names
