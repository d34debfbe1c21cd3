"""`dist -A --long-reads` / mk_sketch_push_fastq_long on the GPU: FASTQ lines of any length through the base stream.

Geometries: L3K11 (tuned pair-filter kernel), L1K7 (generic kernel), L0K6 (every k-mer accepted).  Every comparison is bit-exact:
against Oracle.koc_from_rows on one wide row per read (the reference's per-read loop on a row of any width), against
Oracle.koc_from_fastq where the reads are under 4 095 characters, and against the directories the real reference wrote from the
chopped files (tests/golden/longreads, tests/test_longreads_model.py).  Every expected sketch is checked for not being trivial: a
stated number of keys, a count above 1, and a difference to the sketch of the same reads truncated at 4 094 characters."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import composite_model as cm
import golden_cases as gc
import longreads_cases as lc
import test_golden as tg
import util_inputs as ui

pytestmark = pytest.mark.gpu
shuf_files = tg.shuf_files
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "longreads")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
BIN = tg.PRODUCT_CLI
DIST = [BIN, "dist", "-p", "4"]


@pytest.fixture(scope="module")
def capi():
    from metakssd_amd import capi as c
    if c.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run on the MI355X box")
    return c


@pytest.fixture(scope="module")
def engine_for(capi):
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = capi.Engine(lc.get_shuf(geom), 0)
        return made[geom]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def oracles(oracle_for):
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = oracle_for(lc.get_shuf(geom))
        return made[geom]
    return get


def frozen(w):
    for ids, counts in w:
        ids.setflags(write=False)
        counts.setflags(write=False)
    return w


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def assert_same(got, want, label=""):
    assert len(got) == len(want), label
    for c, ((gi, gc_), (wi, wc)) in enumerate(zip(got, want)):
        assert len(gi) == len(wi), "%s component %d: %d ids vs oracle %d" % (label, c, len(gi), len(wi))
        assert np.array_equal(gi, wi), "%s component %d: id order/content differs" % (label, c)
        assert gc_ is not None and np.array_equal(gc_, wc), "%s component %d: counts differ" % (label, c)


def sketch_of_reads(ora, seqs):
    rows, stride = lc.rows_of(seqs)
    rc, w = ora.koc_from_rows(rows, stride)
    assert rc == 0
    return frozen(w)


def assert_not_trivial(ora, seqs, want, min_keys, label):
    """at least min_keys keys, a count above 1, and not the sketch of the reads truncated at the reference's line width"""
    assert sum(len(w[0]) for w in want) >= min_keys, label
    assert max(int(w[1].max()) for w in want if len(w[1])) > 1, label
    assert not same(want, sketch_of_reads(ora, [s[:lc.FQ_MAX] for s in seqs])), label + ": truncated reads give the same sketch"


@pytest.fixture(scope="module")
def want_for(oracles):
    """case -> the oracle's sketch of its reads on wide rows, computed once per module, never changed, checked for not being trivial"""
    made = {}

    def get(case):
        if case not in made:
            ora = oracles(lc.CASES[case][1])
            w = sketch_of_reads(ora, lc.reads(case))
            assert_not_trivial(ora, lc.reads(case), w, lc.MIN_KEYS[case], case)
            made[case] = w
        return made[case]
    return get


def assert_is_fixture(got, case):
    for c, (ids, cnt) in enumerate(got):
        assert np.asarray(ids, dtype="<u4").tobytes() == open(os.path.join(GOLD, case, "combco.%d" % c), "rb").read(), (case, c)
        assert np.asarray(cnt, dtype="<u2").tobytes() == open(os.path.join(GOLD, case, "combco.%d.a.u16" % c), "rb").read(), (case, c)


def push_cuts(capi, eng, text, cuts):
    """the text in the pieces that the offsets `cuts` leave, the last one final"""
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    edges = [0] + [c for c in cuts if 0 < c < len(b)] + [len(b)]
    for i in range(len(edges) - 1):
        part = np.ascontiguousarray(b[edges[i]:edges[i + 1]])
        last = i == len(edges) - 2
        capi._check(capi.lib.mk_sketch_push_fastq_long(eng.h, part.ctypes.data if len(part) else None, len(part), 1 if last else 0), eng.h)


# ---- 1. lengths ---------------------------------------------------------------------------------------------------------------------
MODES = ["whole", "63", "1023", "1024", "1025", "4099", "bytewise300", "oversize"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", ["L3K11", "L1K7", "L0K6"])
def test_lengths(capi, engine_for, want_for, geom, mode):
    """reads of 0 .. 70 001 bases, line ends on every offset of a step and on both sides of a segment bound: pushed whole (the small
    pitch), in pieces that cut every kind of line anywhere, byte by byte over the first 300 bytes, and with a piece longer than the text"""
    case = "lengths_" + geom
    text, want, eng = lc.fastq(case), want_for(case), engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    if mode == "whole":
        eng.push_fastq_long(text)
    elif mode == "oversize":
        eng.push_fastq_long(text, piece=len(text) + 1000)
    elif mode == "bytewise300":
        push_cuts(capi, eng, text, list(range(1, 301)))
    else:
        eng.push_fastq_long(text, piece=int(mode))
    got = eng.finish()
    assert_same(got, want, "%s %s" % (case, mode))
    assert_is_fixture(got, case)


# ---- 2. dirty text ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [None, 1025, 61])
@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_dirty_text(capi, engine_for, want_for, geom, piece):
    """runs of N, lower case, CRLF line ends, '>' and '@' in headers, sequences and quality lines, a quality line that starts with '@'"""
    case = "dirty_" + geom
    text = lc.fastq(case)
    assert b"\r\n" in text and b"\n@III" in text and b">" in text.split(b"\n")[0] and any(ln[:1] == b"@" for ln in text.split(b"\n")[3::4])
    eng = engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    eng.push_fastq_long(text, piece=piece)
    got = eng.finish()
    assert_same(got, want_for(case), "%s piece=%s" % (case, piece))
    assert_is_fixture(got, case)


@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_bytes_above_127_in_a_sequence(capi, engine_for, oracles, geom):
    """the reference indexes its 128-entry base table out of bounds with them; the oracle and the device define them as no base"""
    rs = np.random.RandomState(77)
    pool = ui.rand_seq(rs, 60000)
    marked = b"".join(pool[a:a + 500] + (b"\x80", b"\xff\xc3\xa9")[a // 500 % 2] for a in range(2000, 30000, 500))  # 56 places
    seqs = [pool[:9000], marked, b"\xa5" * 300, pool[100:60000]]
    text = b"".join(b"@h%d \xc3\xa9\n" % i + s + b"\n+\n" + b"\x80" * len(s) + b"\n" for i, s in enumerate(seqs))
    ora = oracles(geom)
    want = sketch_of_reads(ora, seqs)
    assert_not_trivial(ora, seqs, want, {"L3K11": 8, "L1K7": 3000}[geom], geom)
    if geom == "L1K7":  # they do reset the window: without them 56 x 13 more windows, one in sixteen accepted
        assert not same(want, sketch_of_reads(ora, [s.replace(b"\x80", b"").replace(b"\xff\xc3\xa9", b"") for s in seqs]))
    eng = engine_for(geom)
    for piece in (None, 4099):
        eng.begin(capi.MK_MODE_KOC)
        eng.push_fastq_long(text, piece=piece)
        assert_same(eng.finish(), want, "%s piece=%s" % (geom, piece))


# ---- 3. file ends -------------------------------------------------------------------------------------------------------------------
def three_records(geom):
    rs = np.random.RandomState(31)
    a = ui.rand_seq(rs, 400)
    seqs = [a[:300], a[100:350], a[40:110] + a[40:110]]  # overlapping cuts, the last read twice the same 70 bases: counts above 1
    return seqs, ui.fastq_bytes(seqs)


@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_file_ends(capi, engine_for, oracles, geom):
    """a three-record file truncated at every byte of its last record, each truncation pushed whole and in two pieces cut inside that
    record: the record counts only when its fourth line has a byte (iseq2comem.c:673).  Reads under 4 095 characters: koc_from_fastq
    is the oracle as it is"""
    seqs, text = three_records(geom)
    ora, eng = oracles(geom), engine_for(geom)
    start = len(ui.fastq_bytes(seqs[:2]))
    rc, full = ora.koc_from_fastq(text)
    rc2, two = ora.koc_from_fastq(text[:start])
    assert rc == 0 and rc2 == 0 and not same(full, two)
    assert sum(len(w[0]) for w in full) >= {"L1K7": 10, "L0K6": 300}[geom] and max(int(w[1].max()) for w in full if len(w[1])) > 1
    with_last = 0
    for n in range(start, len(text) + 1):
        cut = text[:n]
        rc, want = ora.koc_from_fastq(cut)
        assert rc == 0
        with_last += same(want, full)
        assert same(want, full) or same(want, two)
        for cuts in ([], [start + (n - start) // 2]):
            eng.begin(capi.MK_MODE_KOC)
            push_cuts(capi, eng, cut, cuts)
            assert_same(eng.finish(), want, "%s cut at %d of %d, pieces %s" % (geom, n, len(text), cuts))
    assert with_last == len(seqs[2]) + 1  # from the first quality byte on, with or without the final '\n'


@pytest.mark.parametrize("geom", ["L1K7"])
def test_empty_file_and_trailing_blank_lines(capi, engine_for, oracles, geom):
    seqs, text = three_records(geom)
    ora, eng = oracles(geom), engine_for(geom)
    for t, pieces in [(b"", None), (b"", 7), (b"\n", None), (text + b"\n", None), (text + b"\n\n\n", 64), (text + b"\n\n\n\n", None), (text + b"\n" * 9, 5),
                      (b"\n\n\n\n" + text, None)]:
        rc, want = ora.koc_from_fastq(t)
        assert rc == 0
        eng.begin(capi.MK_MODE_KOC)
        eng.push_fastq_long(t, piece=pieces)
        assert_same(eng.finish(), want, "%r... + %d bytes, piece=%s" % (t[:4], len(t), pieces))
    # nothing but a final call, and a final call of no bytes behind text
    eng.begin(capi.MK_MODE_KOC)
    capi._check(capi.lib.mk_sketch_push_fastq_long(eng.h, None, 0, 1), eng.h)
    assert sum(len(g[0]) for g in eng.finish()) == 0
    rc, want = ora.koc_from_fastq(text[:-1])
    eng.begin(capi.MK_MODE_KOC)
    eng.push_fastq_long(text[:-1], final=False)
    capi._check(capi.lib.mk_sketch_push_fastq_long(eng.h, None, 0, 1), eng.h)
    assert_same(eng.finish(), want, "open last record closed by an empty final push")
    assert sum(len(w[0]) for w in want) > 0


# ---- 4. / 5. saturation and a crowded table ----------------------------------------------------------------------------------------------
def test_count_saturates_at_65535(capi, engine_for, oracles):
    seqs = [b"A" * 70000]
    want = sketch_of_reads(oracles("L0K6"), seqs)
    assert sum(len(w[0]) for w in want) == 1 and max(int(w[1].max()) for w in want if len(w[1])) == 65535
    assert not same(want, sketch_of_reads(oracles("L0K6"), [seqs[0][:lc.FQ_MAX]]))
    eng = engine_for("L0K6")
    for piece in (None, 10007):
        eng.begin(capi.MK_MODE_KOC)
        eng.push_fastq_long(ui.fastq_bytes(seqs), piece=piece)
        assert_same(eng.finish(), want, "70 000 A, piece=%s" % piece)


def test_crowded_beyond_hashlimit(capi, engine_for, oracles):
    """one read of 120 000 random bases at L0K6: more distinct 12-mers than hashlimit (78 642 of 131 071 slots)"""
    seq = ui.rand_seq(np.random.RandomState(41), 120000)
    rows, stride = lc.rows_of([seq])
    rc, _ = oracles("L0K6").koc_from_rows(rows, stride)
    assert rc != 0  # the reference's "the context space is too crowd"
    rc, ok = oracles("L0K6").koc_from_rows(*lc.rows_of([seq[:lc.FQ_MAX]]))
    assert rc == 0  # the truncated read would not have been
    eng = engine_for("L0K6")
    eng.begin(capi.MK_MODE_KOC)
    eng.push_fastq_long(ui.fastq_bytes([seq]), piece=50021)
    with pytest.raises(capi.MkError) as ei:
        eng.finish()
    assert ei.value.code == capi.MK_ERR_CROWDED
    eng.begin(capi.MK_MODE_KOC)  # the engine goes on
    eng.push_fastq_long(ui.fastq_bytes([seq[:lc.FQ_MAX]]))
    assert_same(eng.finish(), frozen(ok), "after a crowded sketch")


# ---- 6. short reads: the existing -A golden cases through the long route ------------------------------------------------------------------
SHORT_CASES = ["ragged500_L1K7", "ragged500_crlf_L1K7", "ragged500_trunc_L1K7", "ragged500_nonl_L1K7", "pool2000_L0K6", "dense150_L0K6"]


@pytest.mark.parametrize("case", SHORT_CASES)
def test_short_read_golden_case_through_the_abi(capi, engine_for, case, tmp_path):
    entry = tg.MANIFEST["cases"][case]
    assert entry["flags"] == ["-A"] and not entry["aborted"] and entry["shuf"] in lc.GEOMS
    text = open(gc.build_input(case, str(tmp_path)), "rb").read()
    exp = os.path.join(gc.GOLDEN, "expected", case)
    eng = engine_for(entry["shuf"])
    for piece in (None, 4099):
        eng.begin(capi.MK_MODE_KOC)
        eng.push_fastq_long(text, piece=piece)
        got = eng.finish()
        assert sum(len(g[0]) for g in got) == entry["stat"]["all_ctx_ct"] > 100
        for c, (ids, cnt) in enumerate(got):
            assert np.asarray(ids, dtype="<u4").tobytes() == open(os.path.join(exp, "combco.%d" % c), "rb").read(), (case, c, piece)
            assert np.asarray(cnt, dtype="<u2").tobytes() == open(os.path.join(exp, "combco.%d.a" % c), "rb").read(), (case, c, piece)


def test_state_errors(capi, engine_for):
    eng = engine_for("L1K7")
    for begin in (lambda: eng.begin(capi.MK_MODE_SET), lambda: eng.begin_occ(2)):
        begin()
        with pytest.raises(capi.MkError) as ei:
            eng.push_fastq_long(b"@r\nACGT\n+\nIIII\n")
        assert ei.value.code == capi.MK_ERR_STATE and "MK_MODE_KOC" in str(ei.value)
        eng.finish()
    eng.begin(capi.MK_MODE_KOC)
    eng.push_fastq_long(b"@r\nACGT\n+\nIIII\n")
    with pytest.raises(capi.MkError) as ei:
        eng.push_fastq_long(b"@r\nACGT\n+\nIIII\n")
    assert ei.value.code == capi.MK_ERR_STATE and "final" in str(ei.value)
    eng.finish()
    eng.begin(capi.MK_MODE_KOC)
    eng.push_stream(b">g\nACGTACGTACGTACGTACGT\n", final=False)
    with pytest.raises(capi.MkError) as ei:
        eng.push_fastq_long(b"@r\nACGT\n+\nIIII\n")
    assert ei.value.code == capi.MK_ERR_STATE
    eng.push_stream(b"", final=True)
    eng.finish()


# ---- 7. command line ----------------------------------------------------------------------------------------------------------------
def run_cli(args, env=None):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, (args, r.stderr.decode(errors="replace")[-500:])
    return r.stdout


@pytest.fixture(scope="module")
def lr_shufs(tmp_path_factory):
    d = tmp_path_factory.mktemp("longreads_shufs")
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = str(d / (geom + ".shuf"))
            lc.get_shuf(geom).write(made[geom])
        return made[geom]
    return get


def check_dir(out, cases, inputs):
    """a sketch directory of the files `inputs` against the reference-made fixtures of `cases`, file blocks in input order"""
    stat, names = tg.parse_stat(os.path.join(out, "cofiles.stat"))
    assert names == inputs
    e = [MANIFEST["cases"][c] for c in cases]
    assert stat["koc"] == 1 and stat["ctx_ct"] == [x["keys"] for x in e] and stat["all_ctx_ct"] == sum(x["keys"] for x in e)
    for k in ("shuf_id", "kmerlen", "dim_rd_len", "comp_num"):
        assert stat[k] == e[0]["stat"][k]
    C = stat["comp_num"]
    for c in range(C):
        assert open(os.path.join(out, "combco.%d" % c), "rb").read() == b"".join(open(os.path.join(GOLD, x, "combco.%d" % c), "rb").read() for x in cases)
        assert open(os.path.join(out, "combco.%d.a" % c), "rb").read() == b"".join(open(os.path.join(GOLD, x, "combco.%d.a.u16" % c), "rb").read() for x in cases)


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("case", ["lengths_L3K11", "lengths_L1K7", "dirty_L0K6"])
def test_cli_reproduces_the_reference_directory(case, gz, lr_shufs, tmp_path):
    geom = lc.CASES[case][1]
    inp = str(tmp_path / (case + (".fq.gz" if gz else ".fq")))
    if gz:
        with gzip.GzipFile(inp, "wb", mtime=0) as f:
            f.write(lc.fastq(case))
    else:
        open(inp, "wb").write(lc.fastq(case))
    out = str(tmp_path / "out")
    stdout = run_cli(DIST + ["-L", lr_shufs(geom), "-A", "--long-reads", "--timing", "-o", out, inp]).decode()
    check_dir(out, [case], [inp])
    routes = [json.loads(ln) for ln in stdout.splitlines() if ln.startswith('{"input"')]
    assert len(routes) == 1 and routes[0]["route"] == "long-reads" and routes[0]["source"] == ("zcat" if gz else "file")
    assert routes[0]["text_bytes"] == len(lc.fastq(case)) and routes[0]["pieces"] == 1
    # without the switch nothing changes: the same refusal of the long lines
    r = subprocess.run(DIST + ["-L", lr_shufs(geom), "-A", "-o", str(tmp_path / "out2"), inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout.count(b"\n") <= 2 and b"outside the framing contract" in r.stderr


def test_cli_two_files_in_one_run(lr_shufs, tmp_path):
    inputs = []
    for case in ("lengths_L1K7", "dirty_L1K7"):
        inputs.append(str(tmp_path / (case + ".fq")))
        open(inputs[-1], "wb").write(lc.fastq(case))
    out = str(tmp_path / "out")
    run_cli(DIST + ["-L", lr_shufs("L1K7"), "-A", "--long-reads", "-o", out] + inputs)
    _, names = tg.parse_stat(os.path.join(out, "cofiles.stat"))
    assert sorted(names) == sorted(inputs)
    check_dir(out, [os.path.basename(n)[:-3] for n in names], names)


@pytest.mark.parametrize("case", ["ragged500_L1K7", "ragged500_nonl_L1K7", "ragged500_gz_L1K7", "pool2000_L2K11"])
def test_cli_short_read_golden_case_with_the_switch(case, shuf_files, tmp_path):
    """an existing -A golden case (16 components at L2K11) run with --long-reads equals its reference-made directory"""
    entry = tg.MANIFEST["cases"][case]
    inp = gc.build_input(case, str(tmp_path))
    out = str(tmp_path / "out")
    run_cli(DIST + ["-L", shuf_files(entry["shuf"])] + entry["flags"] + ["--long-reads", "-o", out, inp])
    tg.check_against_golden(case, out, inp)


def test_cli_composite_equals_two_steps(shuf_files, tmp_path):
    """`dist -A --long-reads --composite db` prints what `dist -A --long-reads -o d` + `composite -q d` print, for reads of 3 000 to 9 000
    bases drawn from two of the marker database's strains"""
    db, _ = cm.build_marker_db("composite_mix_L1K7", shuf_files, tmp_path, DIST, [BIN, "set"])
    rs = np.random.RandomState(12)
    ga, gc_ = b"".join(gc._strain("sA")), b"".join(gc._strain("sC"))
    files = []
    for k, share in enumerate((0.8, 0.3)):
        seqs = []
        for _ in range(60):
            g = ga if rs.rand() < share else gc_
            n = int(rs.randint(3000, 9001))
            a = int(rs.randint(0, len(g) - n))
            seqs.append(ui.revcomp(g[a:a + n]) if rs.rand() < 0.5 else g[a:a + n])
        assert max(len(s) for s in seqs) > lc.FQ_MAX
        files.append(str(tmp_path / ("long%d.fq" % k)))
        open(files[-1], "wb").write(ui.fastq_bytes(seqs))
    shuf = shuf_files("L1K7")
    d = str(tmp_path / "d")
    run_cli(DIST + ["-L", shuf, "-A", "--long-reads", "-o", d] + files)
    want = run_cli([BIN, "composite", "-r", db, "-q", d])
    assert len({ln.split(b"\t")[0] for ln in want.splitlines()}) == 2 and want.count(b"\n") >= 4
    assert run_cli(DIST + ["-L", shuf, "-A", "--long-reads", "--composite", db] + files) == want


# ---- 8. poison ----------------------------------------------------------------------------------------------------------------------
def test_abi_tests_under_poison():
    """MK_POISON fills every allocation of the library before use (read once per process: a process of its own): the ABI tests again --
    a kernel that read what nobody wrote (the text buffer's slack, summaries past the last segment, the carry) would not match"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "test_lengths or test_dirty_text or test_bytes_above or test_file_ends or test_empty_file or test_count_saturates or "
                        "test_crowded or test_short_read_golden_case_through_the_abi or test_state_errors"],
                       env=dict(os.environ, MK_POISON="0xA5"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    m = re.search(r"(\d+) passed", out)
    assert r.returncode == 0 and m and int(m.group(1)) == len(MODES) * 3 + 6 + 2 + 2 + 1 + 1 + 1 + len(SHORT_CASES) + 1 and "skipped" not in out, out[-3000:]
