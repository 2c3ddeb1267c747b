"""bench.py --dump-outputs without a GPU: what dump_outputs writes (whole fields, or the same seeded sample of x columns from every field
within the size limit), and the refusal of a multi-GPU run before any rank is started."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _fields(nx, ny, dtype, dye=False):
    rng = np.random.default_rng(7)
    f = {"v": rng.standard_normal((nx, ny, 2)).astype(dtype), "p": rng.standard_normal((nx, ny)).astype(dtype)}
    if dye:
        f["dye"] = rng.random((nx, ny, 3)).astype(dtype)
    return f


def test_small_fields_are_written_whole(tmp_path):
    bench = _bench_module()
    for dtype in (np.float32, np.float64):
        f = _fields(128, 64, dtype, dye=True)
        bench.dump_outputs(f, str(tmp_path / np.dtype(dtype).name))
        for k, a in f.items():
            got = np.load(tmp_path / np.dtype(dtype).name / (k + ".npy"))
            assert got.dtype == dtype and np.array_equal(got, a), k


def test_large_fields_keep_the_same_seeded_columns_within_the_limit(tmp_path):
    bench = _bench_module()
    assert bench.DUMP_LIMIT <= 64_000_000
    f = _fields(1000, 256, np.float32)
    limit = 1_000_000                              # (the whole fields: 3 MB)
    bench.dump_outputs(f, str(tmp_path / "a"), limit=limit)
    bench.dump_outputs(f, str(tmp_path / "b"), limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in f)
    assert total <= limit
    v, p = np.load(tmp_path / "a" / "v.npy"), np.load(tmp_path / "a" / "p.npy")
    assert v.shape[1:] == (256, 2) and p.shape[1:] == (256,) and v.shape[0] == p.shape[0] and 0 < p.shape[0] < 1000
    assert total > limit - sum(a[0].nbytes for a in f.values()) - 4096        # as many columns as fit
    # which columns: the same for every field, in order, and the same from run to run
    cols = [int(np.flatnonzero((f["p"] == row).all(axis=1))[0]) for row in p]
    assert cols == sorted(set(cols)) and np.array_equal(v, f["v"][cols])
    for k in f:
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))), k


def test_dump_outputs_refuses_a_multi_gpu_run(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path / "d")],
                         capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode != 0 and "--dump-outputs needs a single-GPU run" in out.stderr and out.stdout == ""
    assert not (tmp_path / "d").exists()
