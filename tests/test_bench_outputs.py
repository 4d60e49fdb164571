"""bench.py's `--dump-outputs` writer (`write_outputs`): float32 / float64 kept, integers and flags widened to float64, and above the
size cap a fixed, seeded sample of the rows of the long arrays (no GPU)."""
import importlib.util
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_outputs_are_written_whole_in_float32_or_float64(tmp_path):
    b = _bench()
    idx = np.array([3, -1, 7, 199999], dtype=np.int64)
    arrays = dict(T=np.eye(4), sim=np.array([0.9, -2.0, 0.85, 0.8], dtype=np.float32), idx=idx,
                  corres=np.array([[0, 3], [2, 7]], dtype=np.int32), inlier_mask=np.array([1, 0], dtype=np.uint8))
    names = b.write_outputs(tmp_path / "out", arrays)
    got = _load(tmp_path / "out")
    assert names == sorted(arrays) == sorted(got)
    assert got["T"].dtype == np.float64 and got["sim"].dtype == np.float32
    assert all(got[k].dtype == np.float64 for k in ("idx", "corres", "inlier_mask"))
    for k, a in arrays.items():
        np.testing.assert_array_equal(got[k], a)


def test_outputs_above_the_cap_keep_the_same_seeded_rows(tmp_path):
    b = _bench()
    n = 300_000
    rng = np.random.default_rng(5)
    arrays = dict(T=np.eye(4), idx=rng.integers(-1, 10 ** 6, n), sim=rng.random(n, dtype=np.float32),
                  corres=rng.integers(0, 10 ** 6, (n, 2)).astype(np.int32))
    cap = 2 * 10 ** 6      # the arrays widened to float64 hold 9.6 MB
    for run in ("a", "b"):
        b.write_outputs(tmp_path / run, arrays, max_bytes=cap)
    a1, a2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= cap
    assert sorted(a1) == ["T", "corres", "corres_rows", "idx", "idx_rows", "sim", "sim_rows"]
    np.testing.assert_array_equal(a1["T"], np.eye(4))               # the pose is kept whole: only long arrays are sampled
    for k in a1:
        np.testing.assert_array_equal(a1[k], a2[k])                  # the same sample in every run
    rows = a1["idx_rows"].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(a1["sim_rows"], a1["idx_rows"])   # arrays of the same length keep the same rows
    np.testing.assert_array_equal(a1["idx"], arrays["idx"][rows].astype(np.float64))
    np.testing.assert_array_equal(a1["corres"], arrays["corres"][rows].astype(np.float64))
