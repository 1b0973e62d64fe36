"""bench.py --dump-outputs (CPU): the file it writes is float32, whole when
small, and a fixed sample of the rows, the same from call to call, when the
output is larger than the cap."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_whole_when_small(tmp_path):
    z = np.arange(40, dtype=np.float64).reshape(10, 4)
    bench.dump_outputs(str(tmp_path / "a" / "b"), "z", z, 10)
    got = np.load(tmp_path / "a" / "b" / "z.npy")
    assert got.dtype == np.float32 and np.array_equal(got, z.astype(np.float32))


def test_dump_sample_is_fixed(tmp_path):
    z = np.arange(4000, dtype=np.float32).reshape(1000, 4)
    bench.dump_outputs(str(tmp_path / "one"), "z", z, 64)
    bench.dump_outputs(str(tmp_path / "two"), "z", z, 64)
    a, b = np.load(tmp_path / "one" / "z.npy"), np.load(tmp_path / "two" / "z.npy")
    assert a.shape == (64, 4) and a.dtype == np.float32
    assert np.array_equal(a, b)
    rows = (a[:, 0] / 4).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, z[rows])  # distinct rows of z, ascending


def test_dump_cap_is_within_64_mb():
    assert bench.DUMP_MAX_ROWS * 16 <= 64 * 10**6
