"""Batches at their limits: the late id copy of mk_sketch_batch_end, MK_BATCH_MAX_FILES, the table-bits clamp.

Every case compares each file's components, id by id, with the oracle's co_from_fasta() of that file alone, and asserts through
mk_sketch_batch_home_ids() that the branch it is about was taken: how many ids came home in the batch's own launch sequence and how
many by the copy mk_sketch_batch_end queues when the batch left more than its pinned block holds.  MK_OPT_BATCH_HOME_IDS lowers that
block so that tiny batches reach the copy; the 1 024-file case reaches it with no hook at all.

Seconds per case on an MI355X box: 1.9 for each of the two L2K11 boundary cases (the oracle's 2^29-slot table, see FEWER), 0.36 for
the 1 024 files, 0.07 for each side of the clamp (0.19 under MK_POISON), a few milliseconds for every other case.
"""
import gzip

import numpy as np
import pytest

import util_inputs as ui

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from metakssd_amd import capi as c
    if c.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run on the MI355X box")
    return c


_engines = {}


@pytest.fixture(scope="module")
def engine_for(capi, shufs):
    """one engine per geometry for the small cases; every test sets the options it needs and puts them back"""
    def get(name):
        if name not in _engines:
            _engines[name] = capi.Engine(shufs(name), 0)
        return _engines[name]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def _texts():
    """the file list of test_gpu_parity._batch_texts, small: three genomes of several contigs (repeats and reverse complements inside a
    file: -u), one with an N in every row (wide rows then have extension rows), CRLF, an inline header, no header at all, only a header,
    the empty file, TL - 1 and TL bases, no newline at the end, 7-base lines; the last file is a short one"""
    rs = np.random.RandomState(61)
    g = ui.rand_seq(rs, 24000)
    L = len(g)
    texts = []
    for i in range(3):
        a, b = (i * L) // 4, (i * L) // 4 + L // (4 if i % 3 else 9)
        contigs = [g[a:b], ui.revcomp(g[a + 100:a + 100 + (b - a) // 3]), g[a:a + 57] + b"N" * (i + 1) + g[a + 57:a + 900]]
        texts.append(ui.fasta_bytes(contigs))
    sq = bytearray(g[9000:15000])
    sq[::97] = b"N" * len(sq[::97])
    texts.append(ui.fasta_bytes([bytes(sq)]))
    texts.append(b">h1\r\n" + g[:1000] + b"\r\n" + g[1000:2000] + b"\r\n\r\n" + g[2000:5000] + b"\n>\n" + g[7000:9000].lower() + b"\n")
    texts.append(b">x\n" + g[:700] + b">inline header to the end of this line\n" + g[700:1400] + b"\n")
    texts.append(g[300:4000] + b"\n" + g[100:2000] + b"\n")            # no header at all
    texts.append(b">only header\n")
    texts.append(b"")                                                 # empty file: an empty sketch
    texts.append(b">h\n" + g[:21] + b"\n>g\n" + g[:22] + b"\n")
    texts.append(b">h\n" + g[500:3000] + b"\n>t\n" + g[4000:5000])     # no newline at the end
    texts.append(b">h\n" + b"\n".join(g[i:i + 7] for i in range(0, 3000, 7)) + b"\n")
    texts.append(b">last\n" + g[16000:16000 + 2900] + b"\n")
    return texts


TEXTS = _texts()
# L2K11: a genome with a reverse complement inside, CRLF, only a header, empty, no newline at the end, the short last one.  (The oracle
# clears and dumps the reference's 2^29-slot table for every file it is given, text or none: 2.5 s a file on one core.)
FEWER = [1, 4, 7, 8, 10, 12]
CUT_OFF = b">h\n" + ui.rand_seq(np.random.RandomState(62), 500) + b"\n>cut off"   # ends inside a header line
_want = {}


@pytest.fixture(scope="module")
def want_for(shufs, oracle_for):
    """-> (texts, the oracle's sketch of each of them alone): computed once per geometry and flavour and shared (never changed)"""
    def get(name, uniq):
        if (name, uniq) not in _want:
            ora = oracle_for(shufs(name))
            texts = [TEXTS[i] for i in FEWER] if name == "L2K11" else TEXTS
            out = []
            for t in texts:
                rc, w = ora.co_from_fasta(t, uniq=uniq) if t else (0, None)
                assert rc == 0
                out.append(None if w is None else [ids for ids, _ in w])
            _want[(name, uniq)] = (texts, out)
        return _want[(name, uniq)]
    yield get
    _want.clear()


def total_ids(want, skip=()):
    return sum(sum(len(c) for c in w) for i, w in enumerate(want) if w is not None and i not in skip)


def check(res, want, ncomp, label):
    """status, component_num and every id of every file; -> the number of files that were sketched alone"""
    assert len(res) == len(want), label
    n_alone = 0
    for i, (st, alone, comps) in enumerate(res):
        assert st == 0, "%s file %d: status %d" % (label, i, st)
        assert alone in (0, 1)
        n_alone += alone
        assert len(comps) == ncomp, "%s file %d: %d components" % (label, i, len(comps))
        if want[i] is None:
            assert all(len(c) == 0 for c in comps), "%s file %d: ids from an empty file" % (label, i)
            continue
        for k, (g, w) in enumerate(zip(comps, want[i])):
            assert len(g) == len(w), "%s file %d component %d: %d ids vs oracle %d (alone=%d)" % (label, i, k, len(g), len(w), alone)
            assert np.array_equal(g, w), "%s file %d component %d: id order/content differs (alone=%d)" % (label, i, k, alone)
    return n_alone


def set_hooks(capi, eng, home=0, tab_bits=0):
    eng.set_option(capi.MK_OPT_BATCH_HOME_IDS, home)
    eng.set_option(capi.MK_OPT_BATCH_TAB_BITS, tab_bits)


# ---- B1: the boundaries of the late copy -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniq", [False, True])
@pytest.mark.parametrize("name", ["L1K7", "L2K11"])
def test_late_copy_boundaries(capi, engine_for, want_for, name, uniq):
    """the block holds 4 ids, half of them, all but the last 1-4, exactly all: the ids are the oracle's for every setting, and as many
    come late as do not fit; two rounds (with and without the last file) so that n takes two residues mod 4"""
    texts_all, want_all = want_for(name, uniq)
    mode = capi.MK_MODE_UNIQ_SET if uniq else capi.MK_MODE_SET
    eng = engine_for(name)
    ncomp = eng.params.component_num
    residues = set()
    try:
        for texts, want in ((texts_all, want_all), (texts_all[:-1], want_all[:-1])):
            set_hooks(capi, eng)
            eng.batch_begin(texts, mode)
            assert check(eng.batch_end(), want, ncomp, "%s uniq=%s default" % (name, uniq)) == 0
            with_batch, late = eng.batch_home_ids()
            n = with_batch + late
            print("%s uniq=%s: %d files, n = %d ids (with the batch %d, late %d)" % (name, uniq, len(texts), n, with_batch, late))
            assert late == 0 and n == total_ids(want) and n >= 16
            residues.add(n % 4)
            for cap in (4, (n // 2) & ~3, (n - 1) & ~3, (n + 3) & ~3):
                set_hooks(capi, eng, home=cap)
                eng.batch_begin(texts, mode)
                assert check(eng.batch_end(), want, ncomp, "%s uniq=%s block of %d ids" % (name, uniq, cap)) == 0
                with_batch, late = eng.batch_home_ids()
                print("    block of %d ids: with the batch %d, late %d" % (cap, with_batch, late))
                assert with_batch == min(n, cap) and late == n - min(n, cap), "block of %d ids, n = %d" % (cap, n)
            assert 1 <= n - ((n - 1) & ~3) <= 4
        assert len(residues) >= 2, "n was meant to take two residues mod 4: %s" % sorted(residues)
    finally:
        set_hooks(capi, eng)


# ---- B2: every way a batch is fed -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,name", [("texts", "L1K7"), ("one_buffer", "L1K7"), ("rows_pinned", "L2K11"), ("rows_pageable", "L2K11"),
                                        ("wide_pinned", "L2K11"), ("wide_pageable", "L2K11"), ("gz", "L1K7"), ("gunzip", "L1K7")])
def test_late_copy_on_every_route(capi, engine_for, want_for, route, name):
    """a block of 64 ids: texts in separate buffers and in one, packed rows read in place and copied, wide rows with extension rows,
    gzip files inflated by one wave and by many waves a file"""
    texts, want = want_for(name, False)
    eng = engine_for(name)
    ncomp = eng.params.component_num
    try:
        set_hooks(capi, eng, home=64)
        if route in ("texts", "one_buffer"):
            eng.batch_begin(texts, capi.MK_MODE_SET, one_buffer=route == "one_buffer")
        elif route in ("gz", "gunzip"):
            keep = [i for i, t in enumerate(texts) if t]             # (a gzip file of no text is not what mk_gzip_scan accepts)
            texts, want = [texts[i] for i in keep], [want[i] for i in keep]
            eng.batch_begin_gz([gzip.compress(t, 6, mtime=0) for t in texts], capi.MK_MODE_SET, gunzip={} if route == "gunzip" else None)
        else:
            fmt = capi.MK_ROWS_WIDE if route.startswith("wide") else capi.MK_ROWS_PACKED
            rows = []
            for t in texts:
                r, rc = capi.fasta_pack_rows(t, 2 * eng.params.k, fmt)
                assert rc == 0
                rows.append(r)
            if fmt == capi.MK_ROWS_WIDE:
                assert any(int(r[:4].view(np.uint32)[0]) & 0x20000 for r in rows if r.size), "no extension row in the inputs"
            eng.batch_begin_rows(rows, capi.MK_MODE_SET, pinned=route.endswith("pinned"), fmt=fmt)
        assert check(eng.batch_end(), want, ncomp, route) == 0
        if route in ("gz", "gunzip"):
            assert eng.batch_gz_status(len(texts)) == [0] * len(texts)
        with_batch, late = eng.batch_home_ids()
        print("%s at %s: with the batch %d, late %d" % (route, name, with_batch, late))
        assert with_batch == 64 and late == total_ids(want) - 64 and late > 0
    finally:
        set_hooks(capi, eng)


# ---- B3: late ids together with the slow paths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniq", [False, True])
def test_late_copy_with_files_sketched_alone(capi, engine_for, want_for, shufs, oracle_for, uniq):
    """512 slots a file and a block of 64 ids: several files are sketched alone inside mk_sketch_batch_end, between the queued copy of
    the late ids and the wait for it; one file ends inside a header line (MK_ERR_FORMAT for that file only)"""
    name = "L1K7"
    _, want = want_for(name, uniq)
    mode = capi.MK_MODE_UNIQ_SET if uniq else capi.MK_MODE_SET
    eng = engine_for(name)
    ncomp = eng.params.component_num
    at = 5                                                                # the bad file in the middle, not at the end
    texts = TEXTS[:at] + [CUT_OFF] + TEXTS[at:]
    try:
        set_hooks(capi, eng, home=64, tab_bits=9)
        eng.batch_begin(texts, mode)
        res = eng.batch_end()
        assert res[at][0] == capi.MK_ERR_FORMAT and res[at][2] == []
        res = res[:at] + res[at + 1:]
        n_alone = check(res, want, ncomp, "uniq=%s" % uniq)
        with_batch, late = eng.batch_home_ids()
        # (the ids of the text in front of the cut-off header are in the batch's lists too: written, counted, handed to nobody)
        rc, w = oracle_for(shufs(name)).co_from_fasta(CUT_OFF[:CUT_OFF.rindex(b">")], uniq=uniq)
        assert rc == 0
        in_batch = total_ids(want, skip=[i for i, r in enumerate(res) if r[1]]) + sum(len(ids) for ids, _ in w)
        print("uniq=%s: %d files alone, with the batch %d, late %d" % (uniq, n_alone, with_batch, late))
        assert n_alone >= 3, "the small tables were meant to overflow"
        assert with_batch == 64 and late == in_batch - 64 and late > 0
    finally:
        set_hooks(capi, eng)


# ---- B4: two batches in flight ---------------------------------------------------------------------------------------------------------
def test_late_copy_two_batches_in_flight(capi, engine_for, want_for):
    """begin A, begin B, end A, end B with a block of 64 ids: A's late copy is queued behind B's kernels.  What mk_sketch_batch_end(A)
    handed out is the engine's memory and stays intact until the next mk_sketch_batch_end: through the begin of a third batch"""
    name = "L1K7"
    _, want = want_for(name, False)
    eng = engine_for(name)
    ncomp = eng.params.component_num
    cut = 5
    try:
        set_hooks(capi, eng, home=64)
        eng.batch_begin(TEXTS[:cut], capi.MK_MODE_SET)                     # A
        eng.batch_begin(TEXTS[cut:], capi.MK_MODE_SET, one_buffer=True)    # B
        res_a = eng.batch_end(views=True)
        assert check(res_a, want[:cut], ncomp, "A") == 0
        with_batch, late = eng.batch_home_ids()
        assert with_batch == 64 and late == total_ids(want[:cut]) - 64 and late > 0
        eng.batch_begin(TEXTS[2:9], capi.MK_MODE_SET)                      # a third batch, B still in flight
        assert check(res_a, want[:cut], ncomp, "A after the begin of a third batch") == 0
        del res_a
        assert check(eng.batch_end(), want[cut:], ncomp, "B") == 0
        with_batch, late = eng.batch_home_ids()
        assert with_batch == 64 and late == total_ids(want[cut:]) - 64 and late > 0
        assert check(eng.batch_end(), want[2:9], ncomp, "third") == 0
        with_batch, late = eng.batch_home_ids()
        assert with_batch == 64 and late == total_ids(want[2:9]) - 64 and late > 0
        eng.begin(capi.MK_MODE_SET)                                        # the ordinary path afterwards
        eng.push_stream(TEXTS[0])
        got = eng.finish()
        assert len(got) == ncomp and all(np.array_equal(g, w) for (g, _), w in zip(got, want[0]))
    finally:
        set_hooks(capi, eng)


# ---- B5: the natural trigger -----------------------------------------------------------------------------------------------------------
def test_1024_files_leave_more_ids_than_the_block_holds(capi, shufs, oracle_for):
    """MK_BATCH_MAX_FILES files of 9 000 random bases at L0K6, no hook: about 9.2 M ids, the block holds 8 Mi -- the rest comes late.
    Every one of the 1 024 sketches is the oracle's; 1 025 files are refused.  (0.36 s, most of it the oracle.)"""
    rs = np.random.RandomState(65)
    nfiles = 1024
    texts = [b">g%04d\n" % i + ui.rand_seq(rs, 9000) + b"\n" for i in range(nfiles)]
    ora = oracle_for(shufs("L0K6"))
    want = []
    for t in texts:
        rc, w = ora.co_from_fasta(t)
        assert rc == 0
        want.append([ids for ids, _ in w])
    eng = capi.Engine(shufs("L0K6"), 0)
    try:
        ncomp = eng.params.component_num
        eng.batch_begin(texts, capi.MK_MODE_SET)
        res = eng.batch_end()
        with_batch, late = eng.batch_home_ids()
        assert len(res) == nfiles
        alone = [i for i, r in enumerate(res) if r[1]]
        print("1024 files: with the batch %d, late %d, %d files alone, %d ids by the oracle" % (with_batch, late, len(alone), total_ids(want)))
        for i, (st, al, comps) in enumerate(res):                          # (whole files at a time: 1 024 x component_num numpy calls otherwise)
            assert st == 0 and len(comps) == ncomp, "file %d: status %d" % (i, st)
            assert [len(c) for c in comps] == [len(c) for c in want[i]], "file %d (alone=%d): component sizes" % (i, al)
            assert np.array_equal(np.concatenate(comps), np.concatenate(want[i])), "file %d (alone=%d): ids differ" % (i, al)
        assert len(alone) * 20 <= nfiles, "%d files were sketched alone" % len(alone)
        assert with_batch == 8 << 20 and late > 0
        assert with_batch + late == total_ids(want, skip=alone)
        with pytest.raises(capi.MkError) as ei:
            eng.batch_begin([b">t\nACGT\n"] * (nfiles + 1), capi.MK_MODE_SET)
        assert ei.value.code == capi.MK_ERR_ARG
        eng.batch_begin(texts[:3], capi.MK_MODE_SET)                       # the engine is still usable
        assert check(eng.batch_end(), want[:3], ncomp, "after the refusal") == 0
    finally:
        eng.close()


# ---- B6: both sides of the table clamp --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfiles", [512, 513])
def test_table_bits_clamp(capi, shufs, oracle_for, nfiles):
    """tiny files, one of 22 000 and one of 40 000 bases at L0K6.  512 files: 512 << 17 is 2^26 slots, no clamp, both large files stay
    in the batch.  513 files: 2^16 slots a file, at most 32 768 keys -- the 40 000-base file is sketched alone, the other still fits.
    (4.3 GB of device memory at 2^26 slots; 0.07 s a case.)"""
    rs = np.random.RandomState(66)
    at22, at40 = 3, nfiles // 2
    texts = []
    for i in range(nfiles):
        n = 22000 if i == at22 else 40000 if i == at40 else int(rs.randint(100, 301))
        texts.append(ui.fasta_bytes([ui.rand_seq(rs, n)]))
    ora = oracle_for(shufs("L0K6"))
    want = []
    for t in texts:
        rc, w = ora.co_from_fasta(t)
        assert rc == 0
        want.append([ids for ids, _ in w])
    assert 20000 < total_ids(want[at22:at22 + 1]) <= 32768 < total_ids(want[at40:at40 + 1]) <= 65536
    eng = capi.Engine(shufs("L0K6"), 0)
    try:
        ncomp = eng.params.component_num
        eng.batch_begin(texts, capi.MK_MODE_SET)
        res = eng.batch_end()
        with_batch, late = eng.batch_home_ids()
        alone = [i for i, r in enumerate(res) if r[1]]
        print("%d files: alone %s, with the batch %d, late %d" % (nfiles, alone, with_batch, late))
        check(res, want, ncomp, "%d files" % nfiles)
        assert alone == ([] if nfiles == 512 else [at40])
        assert late == 0 and with_batch == total_ids(want, skip=alone)
    finally:
        eng.close()


# ---- B7: option errors -------------------------------------------------------------------------------------------------------------------
def test_home_ids_option_errors(capi, engine_for, want_for):
    name = "L1K7"
    _, want = want_for(name, False)
    eng = engine_for(name)
    ncomp = eng.params.component_num
    try:
        set_hooks(capi, eng)
        for bad in (1, 2, 3, -1, -4, -64):
            with pytest.raises(capi.MkError) as ei:
                eng.set_option(capi.MK_OPT_BATCH_HOME_IDS, bad)
            assert ei.value.code == capi.MK_ERR_ARG, bad
        eng.batch_begin(TEXTS[:3], capi.MK_MODE_SET)
        for v in (0, 64):
            with pytest.raises(capi.MkError) as ei:
                eng.set_option(capi.MK_OPT_BATCH_HOME_IDS, v)
            assert ei.value.code == capi.MK_ERR_STATE
        assert check(eng.batch_end(), want[:3], ncomp, "after the refused option") == 0
        n = total_ids(want[:3])
        assert eng.batch_home_ids() == (n, 0)                              # the refused values left the rule as it was
        eng.set_option(capi.MK_OPT_BATCH_HOME_IDS, 5)                      # rounded up to a multiple of 4
        eng.batch_begin(TEXTS[:3], capi.MK_MODE_SET)
        assert check(eng.batch_end(), want[:3], ncomp, "block of 5 -> 8 ids") == 0
        assert eng.batch_home_ids() == (8, n - 8)
        eng.set_option(capi.MK_OPT_BATCH_HOME_IDS, 1 << 30)                # it caps from above and never raises the block
        eng.batch_begin(TEXTS[:3], capi.MK_MODE_SET)
        assert check(eng.batch_end(), want[:3], ncomp, "a cap above the rule") == 0
        assert eng.batch_home_ids() == (n, 0)
    finally:
        set_hooks(capi, eng)
