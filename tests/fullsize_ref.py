"""tests/golden/fullsize_digests.json for the tests: the compiled reference's `dist -A -p 1` sketches of the bench read stream, kept
as digests (made by tests/golden/make_golden_fullsize.py), and the comparison every full-size test uses.  All comparisons are exact."""
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_digests.json")
NAMES = ("L3K11_1M", "L3K11_4M", "L3K11_16M", "config3", "config4", "L3K10_dense")


def entries():
    return json.load(open(PATH))["entries"]


def digests(ids, cnt):
    """the four digests of a one-component sketch as it lies in combco.0 (u32 ids) / combco.0.a (u16 counts)"""
    ids, cnt = np.ascontiguousarray(ids, dtype=np.uint32), np.ascontiguousarray(cnt, dtype=np.uint16)
    key = np.sort((ids.astype(np.uint64) << np.uint64(16)) | cnt.astype(np.uint64))
    return {"combco_sha256": hashlib.sha256(ids.tobytes()).hexdigest(), "combco_a_sha256": hashlib.sha256(cnt.tobytes()).hexdigest(),
            "sketch_sha256": hashlib.sha256(ids.tobytes() + cnt.tobytes()).hexdigest(),  # = bench.py's sketch_digest
            "multiset_sha256": hashlib.sha256(key.astype("<u8").tobytes()).hexdigest()}


def assert_equals_reference(entry, ids, cnt, route):
    """the sketch (ids, cnt) must be the reference's bytes.  The message says N, the route, keys got / expected, and whether the
    (id, count) multiset matched: if it did only the ORDER differs (ordinals / layout / dump), otherwise the CONTENT does
    (scan / resolve / insert)"""
    got = digests(ids, cnt)
    if all(got[k] == entry[k] for k in got) and int(ids.size) == entry["keys"]:
        return
    same_set = got["multiset_sha256"] == entry["multiset_sha256"]
    raise AssertionError(
        "N=%d, route %s: the sketch is not the reference's (-p 1): keys got %d, expected %d; sum of counts got %d, expected %d; multiset_sha256 %s "
        "-> %s; sketch_sha256 got %s, expected %s"
        % (entry["reads"], route, ids.size, entry["keys"], int(np.asarray(cnt, dtype=np.int64).sum()), entry["sum_counts"],
           "matched" if same_set else "differs",
           "only the ORDER differs (ordinals / layout / dump)" if same_set else "the CONTENT differs (scan / resolve / insert)",
           got["sketch_sha256"], entry["sketch_sha256"]))
