"""mk_composite (the marker database resident on the device) and the resident route of `composite -q`.

Handle level: exact equality -- every integer and the row order -- with tests/composite_model.py (pinned to the reference's golden output by
tests/test_composite_model.py) AND with per-sample mk_setop_join, the path already pinned to the reference.  Command line: the default run,
--per-query and the oracle print the same bytes."""
import filecmp
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import composite_model as cm
import test_golden as tg

pytestmark = pytest.mark.gpu
shuf_files = tg.shuf_files
REF_CLI = os.path.join(tg.ROOT, "oracle", "_ref", "metakssd")


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def concat(lists, dtype):
    """per-sketch arrays -> (concatenation, positions)"""
    index = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = np.concatenate([np.asarray(x, dtype=dtype) for x in lists]) if lists else np.zeros(0, dtype)
    return flat.astype(dtype), index


def random_case(R, C, S, seed, universe, ref_len, qry_len):
    """ids from a small universe: many are shared by several sketches and samples; sketches may hold an id twice (drawn with
    replacement), samples get a few repeats with other counts"""
    rs = np.random.RandomState(seed)
    ref_comps, qry_comps = [], []
    for _ in range(C):
        refs = [rs.randint(0, universe, rs.randint(0, 2 * ref_len + 1)) for _ in range(R)]
        ref_comps.append(concat(refs, np.uint32))
        qs, qc = [], []
        for _ in range(S):
            ids = rs.permutation(universe)[:rs.randint(0, 2 * qry_len + 1)]
            if ids.size > 4:
                ids = np.concatenate([ids, ids[:3]])      # three ids once more, at the end
            cnt = np.minimum(rs.geometric(0.05, ids.size), 65535)
            qs.append(ids)
            qc.append(cnt)
        ids, index = concat(qs, np.uint32)
        qry_comps.append((ids, concat(qc, np.uint16)[0], index))
    return dict(R=R, S=S, ref=ref_comps, qry=qry_comps)


EXACT = (5, 6, 7, 8, 63, 64, 65, 129, 8193)


def edge_case():
    """the named edge cases in one database of three components (the third one empty):
      sketches 0..199   six private ids each + one id that all 200 hold (a row longer than a wave; 200 sketches tied on 7)
      sketches 200..208 exactly 5, 6, 7, 8, 63, 64, 65, 129, 8193 private ids, spread over components 0 and 1; ids 0 and 0xFFFFFFFF among them
      sketch   209      five ids, one of them twice: six hits only because both positions count
      sketch   210      empty
    samples: 0 holds everything (counts 1 and 65535 among them) and repeats one id of sketch 201 later with another count; 1 is empty;
    2 holds ids no sketch has; 3 holds half of sample 0"""
    rs = np.random.RandomState(7)
    nxt = [1000]
    R = 211
    refs = [[[] for _ in range(R)] for _ in range(3)]   # [component][sketch]

    def fresh(n):
        a = np.arange(nxt[0], nxt[0] + n, dtype=np.int64)
        nxt[0] += n
        return a

    shared = 999
    for r in range(200):
        refs[0][r] = list(fresh(6)) + [shared]
    for j, k in enumerate(EXACT):
        ids = fresh(k)
        if k == 64:
            ids[0], ids[1] = 0, 0xFFFFFFFF
        half = k // 2
        refs[0][200 + j] = list(ids[:half])
        refs[1][200 + j] = list(ids[half:])
    d = fresh(5)
    refs[1][209] = list(d) + [d[2]]
    ref_comps = [concat(refs[c], np.uint32) for c in range(3)]
    S = 4
    qry_comps = []
    for c in range(3):
        allids = np.unique(ref_comps[c][0]) if c < 2 else np.arange(50, 90)
        s0 = rs.permutation(allids)
        c0 = np.minimum(rs.geometric(0.02, s0.size), 65535)
        c0[:2] = (1, 65535)
        if c == 0:   # sketch 201's first id once more, later, with another count: only the first occurrence counts
            rep = refs[0][201][0]
            first = int(np.flatnonzero(s0 == rep)[0])
            c0[first] = 3
            s0 = np.concatenate([s0, [rep]])
            c0 = np.concatenate([c0, [60000]])
        s2 = np.arange(5_000_000, 5_000_300)
        s3 = s0[::2]
        ids, index = concat([s0, [], s2, s3], np.uint32)
        cnt = concat([c0, [], rs.randint(1, 9, s2.size), c0[::2] + 1], np.uint16)[0]
        qry_comps.append((ids, cnt, index))
    return dict(R=R, S=S, ref=ref_comps, qry=qry_comps)


CASES = {
    "1x1x1": lambda: random_case(1, 1, 1, 1, 40, 20, 30),
    "3x1x2": lambda: random_case(3, 1, 2, 2, 60, 30, 40),
    "300x4x5": lambda: random_case(300, 4, 5, 3, 3000, 40, 1200),
    "300x4x33": lambda: random_case(300, 4, 33, 4, 3000, 40, 1200),
    "70000x1x3": lambda: random_case(70000, 1, 3, 5, 60000, 8, 40000),
    "edge": edge_case,
}
_cache = {}


def case(name):
    """the data and the model's rows, computed once and shared"""
    if name not in _cache:
        d = CASES[name]()
        d["want"] = cm.composite_rows(d["R"], d["ref"], d["S"], d["qry"])
        _cache[name] = d
    return _cache[name]


def as_tuples(rows):
    return [[tuple(int(x) for x in r) for r in sample] for sample in rows]


@pytest.fixture(scope="module")
def handles():
    from metakssd_amd import capi
    made = {}

    def get(name, max_hits=None):
        """a handle with the case's database loaded (one per case, kept: loading is what the handle is for)"""
        if name not in made:
            h = capi.Composite(0)
            h.load(case(name)["R"], case(name)["ref"])
            made[name] = h
        made[name].set_option(capi.MK_COMPOSITE_OPT_MAX_HITS, max_hits if max_hits else 1 << 26)
        return made[name]
    yield get
    for h in made.values():
        h.close()


# ---- handle level -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_handle_equals_model(name, handles):
    d = case(name)
    got = as_tuples(handles(name).query(d["S"], d["qry"]))
    assert got == d["want"]
    assert sum(len(s) for s in got) > 0 or name == "1x1x1"


@pytest.mark.parametrize("name", sorted(CASES))
def test_handle_equals_per_sample_join(name, handles):
    """the per-query route's join (mk_setop_join, pinned to the reference by tests/test_gpu_setop.py) gives the same rows"""
    from metakssd_amd import capi
    d = case(name)
    got = as_tuples(handles(name).query(d["S"], d["qry"]))
    so = capi.SetOp(0)
    try:
        for s in range(d["S"]):
            rr, cc = [], []
            for (rids, rindex), (qids, qcnt, qindex) in zip(d["ref"], d["qry"]):
                a, b = int(qindex[s]), int(qindex[s + 1])
                counts, bout = so.join(qids[a:b], qcnt[a:b], rids, rindex)
                rr.append(np.repeat(np.arange(d["R"]), np.diff(bout.astype(np.int64))))
                cc.append(counts.astype(np.int64))
            assert got[s] == cm.rows_from_hits(np.concatenate(rr), np.concatenate(cc)), s
    finally:
        so.close()


def test_edge_case_is_what_it_says():
    d = case("edge")
    s0 = {r[0]: r for r in d["want"][0]}
    assert [s0[200 + j][1] for j, k in enumerate(EXACT) if k >= 6] == [k for k in EXACT if k >= 6] and 200 not in s0
    assert [r[0] for r in d["want"][0] if r[1] == 7] == list(range(200)) + [202]    # 201 sketches tied: by sketch number
    assert s0[209][1] == 6 and 210 not in s0
    assert d["want"][1] == [] and d["want"][2] == [] and len(d["want"][3]) > 0
    assert len(d["ref"][2][0]) == 0 and len(d["qry"][2][0]) > 0
    allc = np.concatenate([q[1] for q in d["qry"]])
    assert allc.min() == 1 and allc.max() == 65535
    assert s0[201][6] < 60000          # the repeat's count did not get in
    assert {0, 0xFFFFFFFF} <= set(int(x) for x in d["ref"][0][0]) | set(int(x) for x in d["ref"][1][0])


@pytest.mark.parametrize("max_hits", [1, 40000, 200000])
def test_cuts_do_not_change_the_result(max_hits, handles):
    """MK_COMPOSITE_OPT_MAX_HITS = 1: one sample per sub-range (each grows the buffer to what it needs); a sample has about 19 000
    hits here, so the other two put about two and about ten samples into a range"""
    d = case("300x4x33")
    h = handles("300x4x33", max_hits)
    got = as_tuples(h.query(d["S"], d["qry"]))
    hits, ranges = h.last_counts()
    print("max_hits", max_hits, "hits", hits, "ranges", ranges)
    assert got == d["want"]
    assert ranges > 1 and (max_hits != 1 or ranges >= 30)
    h = handles("300x4x33")
    assert as_tuples(h.query(d["S"], d["qry"])) == got and h.last_counts() == (hits, 1)


def test_second_batch_on_the_same_handle(handles):
    d, e = case("300x4x5"), case("300x4x33")
    h = handles("300x4x5")
    first = as_tuples(h.query(d["S"], d["qry"]))
    other = as_tuples(h.query(e["S"], e["qry"]))       # another batch against the same database in between
    assert as_tuples(h.query(d["S"], d["qry"])) == first == d["want"]
    assert other == cm.composite_rows(d["R"], d["ref"], e["S"], e["qry"])


def test_query_before_load_is_a_state_error():
    from metakssd_amd import capi
    h = capi.Composite(0)
    try:
        for call in (lambda: h.query_begin(1), lambda: h.query_component(0, [1], [1], [0, 1]), lambda: h.query_finish(1)):
            with pytest.raises(capi.MkError) as e:
                call()
            assert e.value.code == capi.MK_ERR_STATE
        assert capi.lib.mk_composite_load_begin(h.h, 2, 2) == 0
        h._check(capi.lib.mk_composite_load_component(h.h, 0, None, np.zeros(3, np.uint64).ctypes.data))
        with pytest.raises(capi.MkError) as e:     # component 1 of the database is still missing
            h.query_begin(1)
        assert e.value.code == capi.MK_ERR_STATE
    finally:
        h.close()


def test_handle_tests_under_poison():
    """MK_POISON fills every allocation of the library before use (read once per process: a process of its own)"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "handle_equals_model or cuts_do_not or second_batch"], env=dict(os.environ, MK_POISON="0xA5"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


# ---- command line -------------------------------------------------------------------------------------------------------------------
def run_cli(cli, args, env=None):
    r = subprocess.run(cli + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, (args, r.stderr.decode())
    return r.stdout


def split_timing(out):
    """(the output without the --timing line, the line's JSON)"""
    lines = out.split(b"\n")
    t = [ln for ln in lines if ln.startswith(b'{"composite_timing"')]
    assert len(t) == 1, out[-500:]
    return b"\n".join(ln for ln in lines if ln is not t[0]), json.loads(t[0])["composite_timing"]


@pytest.fixture(scope="module")
def marker_db(shuf_files, tmp_path_factory):
    """README recipe on the golden inputs; a query directory of five samples and one of a single sample"""
    tmp = tmp_path_factory.mktemp("composite_cli")
    prod = [tg.PRODUCT_CLI, "dist", "-p", "4"]
    mixes = [(0.7, 0.0, 0.3), (0.0, 1.0, 0.0), (0.2, 0.5, 0.3), (0.0, 0.1, 0.9), (1.0, 0.0, 0.0)]
    files = [cm.strain_mix_fastq(str(tmp / ("sample%d.fq" % i)), 300 + i, w) for i, w in enumerate(mixes)]
    db, q5 = cm.build_marker_db("composite_mix_L1K7", shuf_files, tmp, prod, [tg.PRODUCT_CLI, "set"], query_files=files)
    q1 = str(tmp / "q1")
    import golden_cases as gc
    one = gc.build_input("single_q", str(tmp), spec="fq:mix")
    r = subprocess.run(prod + ["-L", shuf_files("L1K7"), "-A", "-o", q1, one], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    return db, q5, q1, tmp


@pytest.mark.parametrize("poison", [None, "0xA5"])
def test_cli_routes_print_the_same_bytes(marker_db, poison):
    db, q5, _, tmp = marker_db
    env = dict(os.environ, MK_POISON=poison) if poison else None
    comp = [tg.PRODUCT_CLI, "composite"]
    want = run_cli([tg.ORACLE_CLI, "composite"], ["-r", db, "-q", q5])
    assert len({ln.split(b"\t")[0] for ln in want.splitlines()}) >= 3     # rows of several samples (the all-sB sample has none: no marker is private to sB)
    res, t = split_timing(run_cli(comp, ["-r", db, "-q", q5, "--timing"], env))
    assert t["route"] == "resident" and t["samples"] == 5 and t["batches"] >= 1 and t["hits"] > 0
    per, t = split_timing(run_cli(comp, ["-r", db, "-q", q5, "--timing", "--per-query"], env))
    assert t["route"] == "per-query" and t["samples"] == 5
    assert res == want and per == want
    assert run_cli(comp, ["-r", db, "-q", q5], env) == want
    if os.path.exists(REF_CLI) and not poison:
        assert run_cli([REF_CLI, "composite"], ["-r", db, "-q", q5]) == want
    # small batches: one sample per batch
    res, t = split_timing(run_cli(comp, ["-r", db, "-q", q5, "--timing", "--batch-mib", "0"], env))
    assert res == want and t["batches"] == 5


def test_cli_abv_files_are_the_same(marker_db):
    db, q5, _, tmp = marker_db
    dirs = {}
    for who, cli, extra in (("resident", [tg.PRODUCT_CLI, "composite"], []), ("per", [tg.PRODUCT_CLI, "composite"], ["--per-query"]),
                            ("oracle", [tg.ORACLE_CLI, "composite"], [])):
        dirs[who] = str(tmp / ("abv_" + who))
        run_cli(cli, ["-r", db, "-q", q5, "-b", "-o", dirs[who]] + extra)
    if os.path.exists(REF_CLI):
        dirs["reference"] = str(tmp / "abv_reference")
        run_cli([REF_CLI, "composite"], ["-r", db, "-q", q5, "-b", "-o", dirs["reference"]])
    names = sorted(os.listdir(dirs["oracle"]))
    assert len(names) == 5 and any(os.path.getsize(os.path.join(dirs["oracle"], f)) for f in names)
    for who, d in dirs.items():
        assert sorted(os.listdir(d)) == names, who
        for f in names:
            assert filecmp.cmp(os.path.join(d, f), os.path.join(dirs["oracle"], f), shallow=False), (who, f)


def test_cli_one_sample_keeps_the_per_query_route(marker_db):
    db, _, q1, _ = marker_db
    comp = [tg.PRODUCT_CLI, "composite"]
    per, t = split_timing(run_cli(comp, ["-r", db, "-q", q1, "--timing"]))
    assert t["route"] == "per-query" and t["samples"] == 1
    res, t = split_timing(run_cli(comp, ["-r", db, "-q", q1, "--timing", "--resident"]))
    assert t["route"] == "resident"
    assert res == per and per.count(b"\n") > 0
    assert per == run_cli([tg.ORACLE_CLI, "composite"], ["-r", db, "-q", q1])
