"""bench.py's command line and its --dump-outputs helpers (no GPU): --full and --dump-outputs parse and are off by
default, the env sample is everything while it fits the size limit and a fixed seeded subset beyond it, and the
files are float64 .npy."""
import sys

import numpy as np

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_sample_is_everything_or_a_fixed_subset():
    per_env = 8 * 9 * 23 * 8
    fit = bench.DUMP_MAX_BYTES // per_env
    assert np.array_equal(bench.dump_sample(4096, per_env, 0), np.arange(4096))
    assert np.array_equal(bench.dump_sample(fit, per_env, 0), np.arange(fit))
    s = bench.dump_sample(fit + 1000, per_env, 0)
    assert len(s) == fit and len(s) * per_env <= bench.DUMP_MAX_BYTES
    assert (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < fit + 1000
    assert np.array_equal(s, bench.dump_sample(fit + 1000, per_env, 0))


def test_dump_outputs_writes_float64_npy(tmp_path):
    out = tmp_path / "a" / "b"
    bench.dump_outputs(str(out), 0, {"ticks": np.arange(5, dtype=np.int32), "x": np.ones((2, 3), np.float32)})
    bench.dump_outputs(str(out), 1, {"ticks": np.arange(5, dtype=np.int32)})
    assert sorted(p.name for p in out.iterdir()) == ["ticks.npy", "ticks.rank1.npy", "x.npy"]
    t = np.load(out / "ticks.npy")
    assert t.dtype == np.float64 and np.array_equal(t, np.arange(5))
    assert np.load(out / "x.npy").dtype == np.float64


def test_dump_outputs_refuses_non_finite_values(tmp_path):
    import pytest
    with pytest.raises(SystemExit, match="non-finite"):
        bench.dump_outputs(str(tmp_path), 0, {"x": np.array([1.0, np.nan])})
    assert not (tmp_path / "x.npy").exists()
