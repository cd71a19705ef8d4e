"""bench.py --dump-outputs: the files of one dump stay within the 64 MB cap, headers included, and a sampled dump keeps the same rows of
every field.  bench.dump_outputs runs in a child process: importing bench.py sets the HIP runtime's queue count for the process."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 64 * 10 ** 6

# field j of row i holds i * n_fields + j: every value names its row and field
DUMP = """
import sys
import numpy as np
import bench
n_rows, n_fields = int(sys.argv[2]), int(sys.argv[3])
i = np.arange(n_rows, dtype=np.int64) * n_fields
rec = {"refpos": i.astype(np.int32)}
for j in range(1, n_fields):
    rec["f" + str(j)] = (i + j).astype(np.int32)
assert bench.DUMP_MAX_BYTES == int(sys.argv[4])
bench.dump_outputs(sys.argv[1], rec)
"""


def _dump(out_dir, n_rows, n_fields):
    subprocess.check_call([sys.executable, "-s", "-c", DUMP, str(out_dir), str(n_rows), str(n_fields), str(CAP)], cwd=ROOT)
    return {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}, sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))


def _check_rows(got, rows, n_fields):
    for name, a in got.items():
        if name == "_rows":
            continue
        j = 0 if name == "refpos" else int(name[1:])
        assert a.dtype == np.float64 and np.array_equal(a, rows * n_fields + j), name


def test_small_dump_is_whole_and_exact(tmp_path):
    got, total = _dump(tmp_path, 1000, 5)
    assert sorted(got) == ["f1", "f2", "f3", "f4", "refpos"] and total <= CAP
    _check_rows(got, np.arange(1000, dtype=np.float64), 5)


def test_oversized_dump_is_a_seeded_sample_within_the_cap(tmp_path):
    # 137 files (136 fields + _rows): the headers count too; 70 k rows x 136 fields of float64 = 76 MB unsampled
    n_rows, n_fields = 70000, 136
    got, total = _dump(tmp_path / "a", n_rows, n_fields)
    assert total <= CAP, total
    assert total > 0.95 * CAP, total                           # the sample uses the budget
    rows = got["_rows"]
    assert rows.dtype == np.float64 and len(rows) < n_rows and np.all(np.diff(rows) > 0) and rows[-1] < n_rows
    assert len(got) == n_fields + 1
    _check_rows(got, rows, n_fields)                           # the same rows in every field
    again, _ = _dump(tmp_path / "b", n_rows, n_fields)
    assert np.array_equal(again["_rows"], rows)                # fixed seed: the same sample every run


def test_few_wide_fields_over_the_cap(tmp_path):
    n_rows, n_fields = 9 * 10 ** 6, 1                          # 72 MB of one field
    got, total = _dump(tmp_path, n_rows, n_fields)
    assert total <= CAP, total
    _check_rows(got, got["_rows"], n_fields)
