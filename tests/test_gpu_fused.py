"""The device-to-device hand-over behind `dist -A --composite`, at handle level.

Engine: mk_sketch_finish_keys -- the finish that ends at the key list -- gives the sketch mk_sketch_finish gives, as a multiset of
(component, id, count), returns its statuses and leaves the engine ready for the next sketch.
Composite: samples that arrive as device key lists (mk_composite_query_sample_keys, the partition kernels and the DISTINCT instances of
the lookup) give the rows of tests/composite_model.py -- every integer and the row order -- and of the host-fed route on the same data."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import composite_model as cm
import util_inputs as ui

pytestmark = pytest.mark.gpu

_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
    return _hip


def from_device(ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        assert hip().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0
    return out


class DevArray:
    """a host array copied to device memory of its own"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.p = C.c_void_p()
        assert hip().hipMalloc(C.byref(self.p), C.c_size_t(max(a.nbytes, 8))) == 0
        if a.nbytes:
            assert hip().hipMemcpy(self.p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        self.ptr = self.p.value

    def free(self):
        if self.p:
            hip().hipFree(self.p)
            self.p = None


# ---- engine -------------------------------------------------------------------------------------------------------------------------
# (table, COMPONENT_SZ): L0K6z is the L0K6 table with inner substring 0 mapped to 0, so that the poly-A read makes key 0; L1K7 with
# component_sz 5 has 16 components on its small table
GEOMETRIES = [("L0K6z", 8), ("L1K7", 8), ("L1K7", 5)]


def engine_rows():
    """ragged, N and lower-case rows, a poly-A read, and one read 70 000 times (its k-mers saturate at 65535)"""
    rs = np.random.RandomState(91)
    seqs = ui.ragged_reads(rs, 300) + ui.pool_reads(rs, 3000, 300) + [b"A" * 150, b"a" * 60]
    seqs += [ui.rand_seq(rs, 150)] * 70000
    return ui.rows_from_seqs(seqs, 304)


_rows = {}


def rows_once():
    if "r" not in _rows:
        _rows["r"] = engine_rows()
    return _rows["r"]


def multiset_of_result(res):
    t = [np.stack([np.full(len(ids), c, np.int64), ids.astype(np.int64), cnt.astype(np.int64)], 1) for c, (ids, cnt) in enumerate(res)]
    t = np.concatenate(t) if t else np.zeros((0, 3), np.int64)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def multiset_of_keys(eng, kp, cp, n):
    keys, cnt = from_device(kp, n, np.uint64), from_device(cp, n, np.uint32)
    C_, bits = eng.params.component_num, eng.params.comp_code_bits
    assert C_ == 1 << bits
    t = np.stack([(keys % np.uint64(C_)).astype(np.int64), (keys >> np.uint64(bits)).astype(np.int64), cnt.astype(np.int64)], 1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))], keys


@pytest.fixture(scope="module")
def capi():
    from metakssd_amd import capi as c
    if c.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run on the MI355X box")
    return c


@pytest.mark.parametrize("name,csz", GEOMETRIES)
def test_finish_keys_is_the_sketch_as_a_multiset(capi, shufs, name, csz):
    rows = rows_once()
    eng = capi.Engine(shufs(name), 0, component_sz=csz)
    try:
        assert eng.params.component_num == (16 if csz == 5 else 1)
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows, 304, 0)
        first = eng.finish()
        want = multiset_of_result(first)
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows, 304, 0)
        kp, cp, n = eng.finish_keys()
        got, keys = multiset_of_keys(eng, kp, cp, n)
        print(name, csz, "keys", n, "max count", int(got[:, 2].max()))
        assert n == len(want) and n > 300
        assert np.array_equal(got, want)
        assert len(np.unique(keys)) == n                       # distinct keys -> distinct (component, id)
        assert got[:, 2].max() == 65535 and got[:, 2].min() == 1
        if name == "L0K6z":
            assert (keys == 0).sum() == 1                      # key 0 with a count is an entry, as in the dump
            assert want[0, 0] == 0 and want[0, 1] == 0
        # the engine sketches again, correctly: the ordered result, not only the multiset
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows, 304, 0)
        again = eng.finish()
        for (gi, gc), (wi, wc) in zip(again, first):
            assert np.array_equal(gi, wi) and np.array_equal(gc, wc)
        # an empty sketch
        eng.begin(capi.MK_MODE_KOC)
        assert eng.finish_keys()[2] == 0
        # the other modes decide in the dump what is written: refused, and the sketch stays open
        eng.begin(capi.MK_MODE_SET)
        with pytest.raises(capi.MkError) as e:
            eng.finish_keys()
        assert e.value.code == capi.MK_ERR_ARG
        eng.finish()
    finally:
        eng.close()


def status_of(capi, call):
    try:
        call()
    except capi.CrowdedError:
        return capi.MK_ERR_CROWDED
    return capi.MK_OK


@pytest.mark.parametrize("name,csz,nmax", [("L0K6z", 8, 5000), ("L1K7", 5, 40000)])
def test_crowded_at_the_same_row_count(capi, shufs, name, csz, nmax):
    """the first row count at which the key-list finish says "crowded" (bisection: the distinct keys of a prefix only grow) is the first at
    which mk_sketch_finish does"""
    rows = capi.synth_rows_host(5, 0, nmax, 150, 160)
    eng = capi.Engine(shufs(name), 0, component_sz=csz)

    def run(n, keys):
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows[:n * 160], 160, 0)
        return status_of(capi, eng.finish_keys if keys else eng.finish)
    try:
        assert run(nmax, True) == capi.MK_ERR_CROWDED and run(1, True) == capi.MK_OK
        lo, hi = 1, nmax                    # lo fits, hi is crowded
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if run(mid, True) == capi.MK_OK:
                lo = mid
            else:
                hi = mid
        print(name, csz, "first crowded row count", hi)
        assert run(lo, False) == capi.MK_OK and run(hi, False) == capi.MK_ERR_CROWDED
        assert run(lo, True) == capi.MK_OK and run(hi, True) == capi.MK_ERR_CROWDED
        eng.begin(capi.MK_MODE_KOC)         # and after a crowded key-list finish the next sketch is legal and right
        eng.push_reads(rows[:50 * 160], 160, 0)
        a = multiset_of_result(eng.finish())
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows[:50 * 160], 160, 0)
        assert np.array_equal(multiset_of_keys(eng, *eng.finish_keys())[0], a)
    finally:
        eng.close()


def test_stream_that_ends_in_a_header_is_a_format_error_from_both(capi, shufs):
    eng = capi.Engine(shufs("L1K7"), 0)
    try:
        codes = []
        for fin in (eng.finish, eng.finish_keys):
            eng.begin(capi.MK_MODE_KOC)
            capi._check(capi.lib.mk_sketch_push_stream(eng.h, b">only a header", 14, 1), eng.h)
            with pytest.raises(capi.MkError) as e:
                fin()
            codes.append(e.value.code)
        assert codes == [capi.MK_ERR_FORMAT, capi.MK_ERR_FORMAT]
        eng.begin(capi.MK_MODE_KOC)
        assert eng.finish_keys()[2] == 0
    finally:
        eng.close()


def test_finish_keys_time_goes_to_finish_ms(capi, shufs):
    eng = capi.Engine(shufs("L1K7"), 0)
    try:
        eng.profile_enable(True)
        eng.profile_reset()
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(capi.synth_rows_host(3, 0, 2000, 150, 160), 160, 0)
        assert eng.finish_keys()[2] > 0
        assert eng.profile()["finish_ms"] > 0.0
    finally:
        eng.close()


# ---- composite ----------------------------------------------------------------------------------------------------------------------
def concat(lists, dtype):
    index = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = np.concatenate([np.asarray(x, dtype=dtype) for x in lists]) if lists else np.zeros(0, dtype)
    return flat.astype(dtype), index


def key_case(R, C_, S, seed, universe, ref_len, qry_len):
    """tests/test_gpu_composite.py's kind of random case, with samples whose ids are distinct (they are key lists): a database of R sketches
    in C_ components (ids from a small universe, a sketch may hold an id twice; id 0 of component 0 is in sketch 0), S samples with
    counts up to 70 000.  With three samples or more, sample 1 has no keys and sample 2 only keys no sketch has.
    -> the host-fed form (ids, counts clamped to 16 bits, positions) and per sample the key list (u64 keys, u32 counts, shuffled)"""
    rs = np.random.RandomState(seed)
    bits = {1: 0, 16: 4}[C_]
    ref_comps = []
    for c in range(C_):
        refs = [rs.randint(0, universe, rs.randint(0, 2 * ref_len + 1)) for _ in range(R)]
        if c == 0:
            refs[0] = np.concatenate([[0], refs[0]])
        ref_comps.append(concat(refs, np.uint32))
    per = [[None] * S for _ in range(C_)]
    for c in range(C_):
        for s in range(S):
            ids = rs.permutation(universe)[:rs.randint(0, 2 * qry_len + 1)]
            if s == 0 and c == 0 and 0 not in ids:
                ids = np.concatenate([ids, [0]])
            if S >= 3 and s == 1:
                ids = ids[:0]
            if S >= 3 and s == 2:
                ids = universe + 5 + np.arange(min(ids.size, 200))
            cnt = rs.geometric(0.05, ids.size).astype(np.int64)
            cnt[::17] = 70000                                  # clamps to 65535
            if s == 0 and c == 0:
                cnt[ids == 0] = 9
            per[c][s] = (ids.astype(np.int64), cnt)
    qry = []
    for c in range(C_):
        ids, index = concat([per[c][s][0] for s in range(S)], np.uint32)
        cnt = concat([np.minimum(per[c][s][1], 65535) for s in range(S)], np.uint16)[0]
        qry.append((ids, cnt, index))
    lists = []
    for s in range(S):
        keys = np.concatenate([(per[c][s][0].astype(np.uint64) << np.uint64(bits)) | np.uint64(c) for c in range(C_)])
        cnt = np.concatenate([per[c][s][1] for c in range(C_)]).astype(np.uint32)
        o = rs.permutation(keys.size)
        lists.append((keys[o], cnt[o]))
    return dict(R=R, S=S, C=C_, bits=bits, ref=ref_comps, qry=qry, lists=lists)


CASES = {
    "1c_1s": lambda: key_case(3, 1, 1, 11, 60, 30, 40),
    "1c_2s": lambda: key_case(40, 1, 2, 12, 400, 30, 150),
    "1c_33s": lambda: key_case(300, 1, 33, 13, 3000, 40, 1200),
    "16c_1s": lambda: key_case(40, 16, 1, 14, 400, 30, 150),
    "16c_2s": lambda: key_case(40, 16, 2, 15, 400, 30, 150),
    "16c_33s": lambda: key_case(300, 16, 33, 16, 3000, 40, 300),
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


def query_keys(h, d, nsamples=None, bits=None):
    """the case's samples as device key lists through one batch"""
    S = d["S"]
    h.query_begin(S if nsamples is None else nsamples)
    for k, (keys, cnt) in enumerate(d["lists"]):
        a, b = DevArray(keys), DevArray(cnt)
        try:
            h.query_sample_keys(k, a.ptr if keys.size else 0, b.ptr if keys.size else 0, keys.size, d["bits"] if bits is None else bits)
        finally:
            a.free()    # "when the call returns the list may be reused": freed at once
            b.free()
    return as_tuples(h.query_finish(S if nsamples is None else nsamples))


@pytest.fixture(scope="module")
def handles(capi):
    made = {}

    def get(name, max_hits=None):
        if name not in made:
            h = capi.Composite(0)
            h.load(case(name)["R"], case(name)["ref"])
            made[name] = h
        made[name].set_option(capi.MK_COMPOSITE_OPT_MAX_HITS, max_hits if max_hits else 1 << 26)
        return made[name]
    yield get
    for h in made.values():
        h.close()


def test_cases_are_what_they_say():
    d = case("16c_33s")
    assert d["want"][1] == [] and d["want"][2] == [] and len(d["lists"][1][0]) == 0 and len(d["lists"][2][0]) > 1000
    assert sum(len(s) for s in d["want"]) > 1000
    assert (d["lists"][0][0] == 0).sum() == 1 and int(d["ref"][0][0][0]) == 0            # key 0: in sample 0 and in the database
    assert max(int(c.max()) for _, c in d["lists"] if c.size) == 70000
    assert max(int(q[1].max()) for q in d["qry"]) == 65535
    tops = {r[6] for s in d["want"] for r in s}
    assert 65535 in tops                                                                  # a clamped count reaches a row
    for keys, _ in d["lists"]:
        assert len(np.unique(keys)) == keys.size
    for name in CASES:
        assert sum(len(s) for s in case(name)["want"]) > 0 or name == "1c_1s", name


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_samples_equal_model(name, handles):
    d = case(name)
    assert query_keys(handles(name), d) == d["want"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_fed_equals_host_fed(name, handles):
    """the same distinct samples through the (sample, id) table route and through the DISTINCT instances"""
    d = case(name)
    h = handles(name)
    host = as_tuples(h.query(d["S"], d["qry"]))
    assert host == query_keys(h, d) == d["want"]


@pytest.mark.parametrize("max_hits", [1, 40000, 200000])
def test_cuts_do_not_change_the_result(max_hits, handles):
    d = case("16c_33s")
    h = handles("16c_33s", max_hits)
    got = query_keys(h, d)
    hits, ranges = h.last_counts()
    print("max_hits", max_hits, "hits", hits, "ranges", ranges)
    assert got == d["want"]
    assert ranges > 1 and (max_hits != 1 or ranges >= 25)
    h = handles("16c_33s")
    assert query_keys(h, d) == got and h.last_counts() == (hits, 1)
    assert h.last_kernel_ms()[1] > 0.0


def test_device_batch_then_host_batch_and_back(handles):
    d = case("16c_33s")
    h = handles("16c_33s")
    assert query_keys(h, d) == d["want"]
    assert as_tuples(h.query(d["S"], d["qry"])) == d["want"]
    assert query_keys(h, d) == d["want"]
    e = case("16c_2s")      # a smaller batch of other samples against this database, then the large one again
    assert query_keys(h, e) == cm.composite_rows(d["R"], d["ref"], e["S"], e["qry"])
    assert as_tuples(h.query(d["S"], d["qry"])) == d["want"]


def test_a_batch_finished_early_has_empty_samples_at_its_end(handles):
    """the command hands samples over as they finish and flushes by size: the batch was begun with room for more"""
    d = case("16c_2s")
    assert query_keys(handles("16c_2s"), d, nsamples=d["S"] + 3) == d["want"] + [[], [], []]


def test_errors(capi, handles):
    d = case("16c_2s")
    h = handles("16c_2s")
    keys, cnt = d["lists"][0]
    a, b = DevArray(keys), DevArray(cnt)
    ids, c16, index = d["qry"][0]
    try:
        def code(call):
            with pytest.raises(capi.MkError) as e:
                call()
            return e.value.code
        # before a batch
        h.query_begin(2)
        h.query_finish(2)
        assert code(lambda: h.query_sample_keys(0, a.ptr, b.ptr, keys.size, 4)) == capi.MK_ERR_STATE
        # a wrong comp_code_bits, k out of order, k past the batch
        h.query_begin(2)
        assert code(lambda: h.query_sample_keys(0, a.ptr, b.ptr, keys.size, 0)) == capi.MK_ERR_ARG
        assert code(lambda: h.query_sample_keys(0, a.ptr, b.ptr, keys.size, 8)) == capi.MK_ERR_ARG
        assert code(lambda: h.query_sample_keys(1, a.ptr, b.ptr, keys.size, 4)) == capi.MK_ERR_ARG
        h.query_sample_keys(0, a.ptr, b.ptr, keys.size, 4)
        assert code(lambda: h.query_sample_keys(0, a.ptr, b.ptr, keys.size, 4)) == capi.MK_ERR_ARG
        # a device batch takes no host component
        assert code(lambda: h.query_component(0, ids, c16, index)) == capi.MK_ERR_STATE
        h.query_sample_keys(1, a.ptr, b.ptr, keys.size, 4)
        assert code(lambda: h.query_sample_keys(2, a.ptr, b.ptr, keys.size, 4)) == capi.MK_ERR_ARG
        h.query_finish(2)
        # and a host batch no device sample
        h.query_begin(2)
        h.query_component(0, ids, c16, index)
        assert code(lambda: h.query_sample_keys(0, a.ptr, b.ptr, keys.size, 4)) == capi.MK_ERR_STATE
        h.query_finish(2)
        # the handle is as good as before
        assert query_keys(h, d) == d["want"]
    finally:
        a.free()
        b.free()


def test_one_component_database_refuses_four_bits(capi, handles):
    d = case("1c_2s")
    h = handles("1c_2s")
    h.query_begin(1)
    with pytest.raises(capi.MkError) as e:
        h.query_sample_keys(0, 0, 0, 0, 4)
    assert e.value.code == capi.MK_ERR_ARG
    h.query_finish(1)
    assert query_keys(h, d) == d["want"]


def test_engine_key_list_straight_into_the_handle(capi, shufs):
    """the hand-over itself: mk_sketch_finish_keys' pointers go to mk_composite_query_sample_keys; the same sketch, fetched with
    mk_sketch_finish and fed from the host, gives the same rows.  The database: the sample's own ids, dealt to five sketches"""
    eng = capi.Engine(shufs("L1K7"), 0, component_sz=5)
    h = capi.Composite(0)
    try:
        rows = capi.synth_rows_host(7, 0, 3000, 150, 160)
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows, 160, 0)
        res = eng.finish()
        R = 5
        ref = []
        for ids, _ in res:
            parts = [np.sort(ids[r::R]) for r in range(R)]
            ref.append(concat(parts, np.uint32))
        h.load(R, ref)
        qry = [(ids, cnt, np.array([0, len(ids)], np.uint64)) for ids, cnt in res]
        want = cm.composite_rows(R, ref, 1, qry)
        assert len(want[0]) == R
        assert as_tuples(h.query(1, qry)) == want
        eng.begin(capi.MK_MODE_KOC)
        eng.push_reads(rows, 160, 0)
        kp, cp, n = eng.finish_keys()
        h.query_begin(1)
        h.query_sample_keys(0, kp, cp, n, eng.params.comp_code_bits)
        eng.begin(capi.MK_MODE_KOC)          # the list may be reused: the next sketch begins before the batch is finished
        eng.push_reads(rows[:160 * 10], 160, 0)
        assert as_tuples(h.query_finish(1)) == want
        eng.finish()
    finally:
        h.close()
        eng.close()


def test_handle_tests_under_poison():
    """MK_POISON fills every allocation of the library before use (read once per process: a process of its own)"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "device_samples_equal_model or device_fed_equals or cuts_do_not or then_host_batch or finished_early or errors or "
                        "straight_into or finish_keys_is_the_sketch"],
                       env=dict(os.environ, MK_POISON="0xA5"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
