"""The seam inputs (tests/seam_cases.py) without a GPU: on the oracle's sketch of every case every planted key is present with exactly
its expected count, no two planted k-mers share a key, both strands occur, and both row orders hold a tile of 64 rows of kind a -- so
that the engine-against-oracle comparison of tests/test_gpu_seams.py cannot shrink to nothing.  The oracle itself is pinned here to
what the compiled reference wrote for five of the inputs (tests/golden/seams, made by tests/golden/make_golden_seams.py), and the
table beside the GPU module's pitch list is checked against a restatement of mk_launch_scan_ex.

L2K11 runs at pitches 272 and 152 only: its oracle table is 4.3 GB, seconds a case on the CPU."""
import hashlib
import os

import numpy as np
import pytest

import seam_cases as sc
import test_gpu_seams as gs

CPU_CASES = [c for c in gs.CASES if c[0] != "L2K11" or (c[1] in (272, 152) and c[2] == 0)]
CPU_CASES = [c for c in CPU_CASES if c[2] == 0]  # (a pointer offset is the same rows in another place)


@pytest.fixture(scope="module")
def oracles(oracle_for):
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = oracle_for(sc.get_shuf(geom))
        return made[geom]
    return get


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("geom,pitch,offset", CPU_CASES, ids=["%s-p%d" % c[:2] for c in CPU_CASES])
def test_planted_keys_have_their_expected_counts(oracles, geom, pitch, offset):
    case = sc.get_case(geom, pitch)
    assert case.nrows * pitch == case.rows.size and 400 <= case.nrows <= 8000
    assert len(case.anchors) >= 26 and case.anchors[0] == case.TL - 1 and case.anchors[-1] == pitch - 2
    rc, koc = oracles(geom).koc_from_rows(case.rows, pitch)
    assert rc == 0
    info = sc.check_conditions(case, koc)
    assert info["distinct_keys"] >= info["planted"]


def test_anchors_cover_every_seam():
    """up to pitch 528 every end column; beyond, both ends of the row and TL + 8 columns on both sides of every seam listed"""
    for pitch, row in ((p[0], p) for p in gs.PITCHES):
        for TL in (18, 20, 22):
            js = sc.anchors(pitch, TL)
            if pitch <= 528:
                assert js == list(range(TL - 1, pitch - 1))
                continue
            seams = sc.SEAMS.get(pitch, range(128, pitch, 128))
            assert all(s % row[7] == 0 for s in seams), "a listed seam that is no column-block bound"
            for s in seams:
                assert set(range(s - TL - 8, min(s + TL + 9, pitch - 1))) <= set(js)
            assert set(range(TL - 1, TL + 16)) <= set(js) and set(range(pitch - 18, pitch - 1)) <= set(js)
    assert sc.anchors(4096, 22, 4094)[-1] == 4093


@pytest.mark.parametrize("row", gs.PITCHES, ids=["p%d+%d" % r[:2] for r in gs.PITCHES])
def test_pitch_table_is_what_the_launch_selects(row):
    pitch, offset, vec, t6, t5, npieces, onepass, CB, ncb, last, tuned = row
    for subk, threads in ((6, t6), (5, t5)):
        assert sc.launch_plan(pitch, offset, subk) == {"CB": CB, "ncb": ncb, "last": last, "vec16": vec, "threads": threads,
                                                        "npieces": npieces, "onepass": onepass, "tuned": tuned}, (pitch, offset, subk)
    assert (ncb - 1) * CB + last == pitch and 0 < last <= CB <= 128


def test_pitch_table_covers_what_the_issue_lists():
    assert [r[0] for r in gs.PITCHES if r[2]] == [48, 80, 112, 144, 160, 176, 272, 304, 528, 1040, 4096]
    assert [(r[0], r[1]) for r in gs.PITCHES if not r[2] and r[10]] == [(152, 0), (168, 0), (200, 0), (248, 0), (160, 4)]
    assert [r[0] for r in gs.PITCHES if not r[10]] == [164, 308]
    assert len(gs.CASES) == 4 * len(gs.PITCHES)


# ---- the fixtures the compiled reference made -------------------------------------------------------------------------------------
def test_fixture_tree_equals_manifest():
    m = sc.manifest()
    assert sorted(m["cases"]) == sorted(sc.GOLDEN)
    want = {os.path.join(case, f): h for case, e in m["cases"].items() for f, h in e["files"].items()}
    have = {os.path.relpath(os.path.join(dp, f), sc.GOLD) for dp, _, fs in os.walk(sc.GOLD) for f in fs} - {"manifest.json"}
    assert have == set(want)
    for rel, h in want.items():
        assert hashlib.sha256(open(os.path.join(sc.GOLD, rel), "rb").read()).hexdigest() == h, "fixture changed: " + rel
        assert os.path.getsize(os.path.join(sc.GOLD, rel)) <= 256 << 10 and not rel.endswith(".a")
    for case, e in m["cases"].items():
        assert e["stat"]["koc"] == 1 and e["stat"]["infile_num"] == 1 and e["stat"]["ctx_ct"] == [e["keys"]]
        assert e["stat"]["comp_num"] == (16 if case.startswith("L2K11") else 1)


@pytest.mark.parametrize("name", sorted(sc.GOLDEN))
def test_oracle_reproduces_reference_fixture(oracles, name, tmp_path):
    geom, pitch, lmax = sc.GOLDEN[name]
    e = sc.manifest()["cases"][name]
    case = sc.get_case(geom, pitch, lmax)
    text = case.fastq()
    assert hashlib.sha256(text).hexdigest() == e["fastq_sha256"], "the input is no longer what the reference was run on"
    p = str(tmp_path / "x.shuf")
    sc.get_shuf(geom).write(p)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == sc.manifest()["shufs"][geom]
    assert max(len(s) for s in case.seqs) == (pitch - 1 if lmax is None else lmax) <= 4094
    ref = sc.fixture(name)
    rc, rows = oracles(geom).koc_from_rows(case.rows, pitch)
    assert rc == 0
    assert same(rows, ref), "the oracle on the rows differs from the reference's directory"
    rc, fq = oracles(geom).koc_from_fastq(text)
    assert rc == 0
    assert same(fq, ref), "the oracle on the FASTQ text differs from the reference's directory"
    info = sc.check_conditions(case, ref)  # on the REFERENCE's own sketch: every planted key with its count
    assert info["planted_counts"] == e["planted_counts"] and info["rows"] == e["rows"] and info["distinct_keys"] == e["keys"]
