"""bench.py --dump-outputs, host side: the files a dump consists of, their dtypes, and the seeded sample above the 64 MB budget"""
import os

import numpy as np

import bench


def _sketch(rs, sizes, counts=True):
    return [(rs.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32),
             rs.randint(1, 2 ** 16, size=n).astype(np.uint16) if counts else None) for n in sizes]


def test_dump_is_the_whole_sketch_below_the_budget(tmp_path):
    sk = _sketch(np.random.RandomState(1), (1000, 0, 77))
    rep = bench.dump_outputs(str(tmp_path), sk)
    assert not rep["sampled"] and rep["distinct_keys"] == 1077
    assert sorted(rep["files"]) == sorted(os.listdir(str(tmp_path)))
    assert np.load(str(tmp_path / "sketch_sizes.npy")).tolist() == [1000, 0, 77]
    for c, (ids, cnt) in enumerate(sk):
        got_ids = np.load(str(tmp_path / ("sketch_c%d_ids.npy" % c)))
        got_cnt = np.load(str(tmp_path / ("sketch_c%d_counts.npy" % c)))
        assert got_ids.dtype == np.float64 and got_cnt.dtype == np.float32
        assert np.array_equal(got_ids.astype(np.uint32), ids) and np.array_equal(got_cnt.astype(np.uint16), cnt)


def test_dump_without_counts(tmp_path):
    sk = _sketch(np.random.RandomState(2), (500,), counts=False)
    rep = bench.dump_outputs(str(tmp_path), sk)
    assert "sketch_c0_counts.npy" not in rep["files"] and not os.path.exists(str(tmp_path / "sketch_c0_counts.npy"))
    assert np.array_equal(np.load(str(tmp_path / "sketch_c0_ids.npy")).astype(np.uint32), sk[0][0])


def test_dump_above_the_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", (1 << 20) + 120_000)  # room for 6 000 sampled entries of 20 bytes
    sk = _sketch(np.random.RandomState(3), (9000, 3000))
    reps = [bench.dump_outputs(str(tmp_path / d), sk) for d in ("a", "b")]
    assert reps[0]["sampled"] and reps[0]["files"] == reps[1]["files"]
    total = 0
    for f in reps[0]["files"]:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)  # the same arguments give the same files
        total += a.nbytes
    assert total <= bench.DUMP_BUDGET
    assert np.load(str(tmp_path / "a" / "sketch_sizes.npy")).tolist() == [9000, 3000]
    for c, (ids, cnt) in enumerate(sk):
        at = np.load(str(tmp_path / "a" / ("sketch_c%d_positions.npy" % c))).astype(np.int64)
        assert len(at) == len(ids) // 2 and np.all(np.diff(at) > 0)
        assert np.array_equal(np.load(str(tmp_path / "a" / ("sketch_c%d_ids.npy" % c))).astype(np.uint32), ids[at])
        assert np.array_equal(np.load(str(tmp_path / "a" / ("sketch_c%d_counts.npy" % c))).astype(np.uint16), cnt[at])
