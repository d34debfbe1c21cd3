"""tests/golden/fullsize_digests.json (the compiled reference's -p 1 sketches of the bench workload, as digests) is what it says it
is, and the CPU oracle reproduces the reference byte for byte at 1 M and 4 M reads -- without a GPU.  The GPU side of the same pin is
tests/test_gpu_refdigest.py and tests/test_gpu_fullsize.py."""
import json
import os

import numpy as np
import pytest

import fullsize_ref as fr
from conftest import SHUF_SPECS

GOLDEN = os.path.dirname(fr.PATH)
SLOTS = {"L3K11": 33554393, "L3K10": 2097143}


def test_file_holds_the_six_entries():
    doc = json.load(open(fr.PATH))
    e = doc["entries"]
    assert sorted(e) == sorted(fr.NAMES)
    shas = json.load(open(os.path.join(GOLDEN, "manifest.json")))["shufs"]
    want = {"L3K11_1M": ("L3K11", 1_000_000), "L3K11_4M": ("L3K11", 4_000_000), "L3K11_16M": ("L3K11", 16_000_000),
            "config3": ("L3K11", 50_000_000), "config4": ("L3K11", 500_000_000), "L3K10_dense": ("L3K10", 30_000_000)}
    for name, (shuf, n) in want.items():
        x = e[name]
        assert (x["shuf"], x["reads"], x["seed"], x["read_len"], x["flags"]) == (shuf, n, 20261002, 150, ["-A", "-p", "1"]), name
        assert tuple(x["shuf_spec"]) == SHUF_SPECS[shuf] and x["slots"] == SLOTS[shuf], name
        assert x["shuf_sha256"] == shas[shuf]["sha256"], name
        for k in ("combco_sha256", "combco_a_sha256", "sketch_sha256", "multiset_sha256"):
            assert len(x[k]) == 64 and int(x[k], 16) >= 0, (name, k)
        assert 1 <= x["max_count"] <= 65535 and x["keys"] <= x["sum_counts"] and x["keys"] <= 0.6 * x["slots"], name
        # accepted occurrences: (151 - 2k) windows a read, 1/4096 of the inner substrings accepted; the 5-sigma window of
        # test_gpu_fullsize.py
        windows = 151 - 2 * SHUF_SPECS[shuf][0]
        mean = n * windows / 4096
        assert abs(x["sum_counts"] - mean) < 5 * mean ** 0.5, name
    assert e["config3"]["keys"] == 1573525 and e["config4"]["keys"] == 15692589
    assert 0.40 <= e["L3K10_dense"]["keys"] / e["L3K10_dense"]["slots"] <= 0.50


@pytest.mark.parametrize("name", ["L3K11_1M", "L3K11_4M"])
def test_cpu_oracle_reproduces_the_reference(shufs, oracle_for, name):
    """synth_rows_host -> Oracle.koc_from_rows equals the reference's files in all four digests: the oracle is pinned to the reference
    at 10 and 40 times its former largest case, and the committed digests agree with this suite's digest code.  (One core: about
    5 s at 1 M, 20 s at 4 M.)"""
    from metakssd_amd import capi
    x = fr.entries()[name]
    shuf = shufs(x["shuf"])
    rows = capi.synth_rows_host(x["seed"], 0, x["reads"], x["read_len"], 160)
    rc, want = oracle_for(shuf).koc_from_rows(rows, 160)
    assert rc == 0 and len(want) == 1
    fr.assert_equals_reference(x, want[0][0], want[0][1], "CPU oracle, pitch 160")
    assert int(want[0][1].max()) == x["max_count"] and int(want[0][1].astype(np.int64).sum()) == x["sum_counts"]
