"""CPU test (no GPU needed): bench.py --dump-outputs writes the headline point as float64 16-bit digits that give the 12 u64 limbs back
exactly, and --steps below 1 is refused before anything is set up."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dumped_point_round_trips_the_limbs(tmp_path):
    rng = np.random.default_rng(7)
    point = rng.integers(0, 1 << 63, size=12, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    point[3] = np.uint64(0xFFFFFFFFFFFFFFFF)
    _bench().dump_outputs(str(tmp_path / "out"), point)
    d = np.load(tmp_path / "out" / "msm_point.npy")
    assert d.dtype == np.float64 and d.shape == (3, 4, 4)
    digits = d.astype(np.uint64)
    assert (digits.astype(np.float64) == d).all() and int(digits.max()) <= 0xFFFF
    back = sum(digits[..., k] << np.uint64(16 * k) for k in range(4)).reshape(12)
    assert (back == point).all()


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
