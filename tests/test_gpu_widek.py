"""Wide k-mers on the GPU: k 12-16, subk up to 7, clamped subspaces (tests/widek_cases.py), on every route.

From k = 13 on the unituple, the candidate record {fwd lo, fwd hi, ord lo, ord hi} and the key reduction need their upper 32 bits;
with k - drlevel <= 9 the 12-bit pf is ADDED onto outer-context bits the shift did not vacate (keys carry and collide by design);
subk 7 means a 1 GiB .shuf, 2^28 accept bits and a filter index clamped to 14 bits.  Every comparison is bit-exact: against the CPU
oracle (pinned to the reference at these geometries by tests/test_widek_golden.py), against tests/byread_model.py, and against the
reference-made fixtures of tests/golden/widek where one exists.  The inputs carry planted k-mers; what they were planted for (key
counts, top bits, both strands, saturated counts, colliding unituples, sixteen non-empty components) is re-asserted on the oracle's
output, so a test that shrank to nothing fails.

Light geometries first (tables of 131 071 to 33 554 393 slots), the three heavy ones (536 870 909 slots, a 4.3 GB oracle table,
as L2K11) last, each in exactly the tests named for it.  The (16,7,7) table is generated once per module and written to disk only
in the single command-line case."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import byread_model as bm
import widek_cases as wc
from test_widek_golden import BYREAD_CASES, CASES, GOLD, build_sketch_dir, check_dist_dir, write_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
LIGHT_BYREAD = ["W13S6D5", "W14S6D6"]


@pytest.fixture(scope="module")
def capi():
    from metakssd_amd import capi as c
    if c.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run on the MI355X box")
    return c


@pytest.fixture(scope="module")
def engine_for(capi):
    made = {}

    def get(name):
        if name not in made:
            made[name] = capi.Engine(wc.get_shuf(name), 0)
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def handles(capi):
    made = {}

    def get(name):
        if name not in made:
            made[name] = capi.ByRead(wc.get_shuf(name), 0)
        return made[name]
    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def want_for(oracle_for):
    """(geometry, what) -> the oracle's sketch, computed once per module and never changed.  One oracle at a time for the heavy
    geometries (4.3 GB each), the light ones are kept."""
    oracles, results = {}, {}

    def oracle(name):
        if name not in oracles:
            if name in wc.HEAVY:
                for n in [n for n in oracles if n in wc.HEAVY]:
                    del oracles[n]
            oracles[name] = oracle_for(wc.get_shuf(name))
        return oracles[name]

    def get(name, what, *args):
        key = (name, what) + args
        if key not in results:
            inp, ora = wc.get_input(name), oracle(name)
            if what == "koc":
                rc, w = ora.koc_from_rows(inp.row_array(160), 160)
            elif what in ("fa", "fa_u"):
                rc, w = ora.co_from_fasta(inp.fasta(), uniq=what == "fa_u")
            elif what == "file":
                rc, w = ora.co_from_fasta(inp.fasta_files()[args[0]], uniq=args[1])
            elif what == "occ":
                rc, w = ora.co_from_fastq(inp.fastq(), Q=args[1], M=args[0])
            assert rc == 0, key
            for ids, counts in w:
                ids.setflags(write=False)
                if counts is not None:
                    counts.setflags(write=False)
            results[key] = w
        return results[key]
    return get


def assert_same(got, want, label=""):
    assert len(got) == len(want), label
    for c, ((gi, gc), (wi, wc_)) in enumerate(zip(got, want)):
        assert len(gi) == len(wi), "%s component %d: %d ids vs oracle %d" % (label, c, len(gi), len(wi))
        assert np.array_equal(gi, wi), "%s component %d: id order/content differs" % (label, c)
        if wc_ is not None:
            assert gc is not None and np.array_equal(gc, wc_), "%s component %d: counts differ" % (label, c)


def assert_is_fixture(got, case, counts=False):
    """a sketch from the ABI against the reference's combco files of `case`"""
    for c, (ids, cnt) in enumerate(got):
        assert np.asarray(ids, dtype="<u4").tobytes() == open(os.path.join(GOLD, case, "combco.%d" % c), "rb").read(), (case, c)
        if counts:
            assert np.asarray(cnt, dtype="<u2").tobytes() == open(os.path.join(GOLD, case, wc.fixture_name("combco.%d.a" % c)), "rb").read(), (case, c)


# ---- 1. counted rows ----------------------------------------------------------------------------------------------------------------
def check_counted_rows(capi, eng, name, want_for, stride, pushes):
    inp = wc.get_input(name)
    want = want_for(name, "koc")
    ids, counts = [w[0] for w in want], [w[1] for w in want]
    # the input still is what it was planted for (the FASTA sketch's size only where another test needs that sketch anyway)
    wc.check_conditions(name, ids, counts, [w[0] for w in want_for(name, "fa")] if name in wc.LIGHT else None)
    rows = inp.row_array(stride)
    n = len(inp.rows)
    per = (n + pushes - 1) // pushes
    eng.begin(capi.MK_MODE_KOC)
    for s0 in range(0, n, per):
        eng.push_reads(rows[s0 * stride:(s0 + per) * stride], stride, s0)
    got = eng.finish()
    assert_same(got, want, "%s stride %d, %d pushes" % (name, stride, pushes))
    assert_is_fixture(got, name + "_fq_A", counts=True)  # the rows are the FASTQ's reads: the reference's -A sketch


@pytest.mark.parametrize("pushes", [1, 3])
@pytest.mark.parametrize("stride", [160, 308])
@pytest.mark.parametrize("name", wc.LIGHT)
def test_counted_rows_light(capi, engine_for, want_for, name, stride, pushes):
    """push_reads, -A: 48- to 56-bit unituples through the generic kernel's record, additive pf, probe chains and a saturated
    count in the 131 071-slot table of (12,6,6)"""
    check_counted_rows(capi, engine_for(name), name, want_for, stride, pushes)


# ---- 2. FASTA device stream ---------------------------------------------------------------------------------------------------------
def check_fasta_stream(capi, eng, name, want_for, uniq):
    fa = wc.get_input(name).fasta()
    flavour = "fa_u" if uniq else "fa"
    want = want_for(name, flavour)
    assert sum(len(w[0]) for w in want) >= wc.MIN_KEYS[name]
    for piece in (None, 4099 if len(fa) < (1 << 20) else 100003):  # whole, and in pieces that cut lines, headers and k-mers anywhere
        eng.begin(capi.MK_MODE_UNIQ_SET if uniq else capi.MK_MODE_SET)
        eng.push_stream(fa, piece=piece)
        got = eng.finish()
        assert_same(got, want, "%s uniq=%s piece=%s" % (name, uniq, piece))
        assert_is_fixture(got, name + "_" + flavour)


@pytest.mark.parametrize("uniq", [False, True])
@pytest.mark.parametrize("name", wc.LIGHT)
def test_fasta_device_stream_light(capi, engine_for, want_for, name, uniq):
    check_fasta_stream(capi, engine_for(name), name, want_for, uniq)


# ---- 3. a batch of files ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", wc.LIGHT)
def test_batch_of_six_files(capi, engine_for, want_for, name):
    """mk_sketch_batch_begin / _end: six files of unequal sizes in one launch sequence, every file's sketch the oracle's sketch of
    that file alone.  The per-file tables are sized for random text (bases / 16^drlevel), far below what planted k-mers leave: the
    larger files overflow them and are sketched alone by mk_sketch_batch_end -- at (12,6,6) all but the smallest."""
    texts = wc.get_input(name).fasta_files()
    eng = engine_for(name)
    for uniq in (False, True):
        want = [want_for(name, "file", i, uniq) for i in range(len(texts))]
        assert all(sum(len(w[0]) for w in ws) > 0 for ws in want)
        eng.batch_begin(texts, capi.MK_MODE_UNIQ_SET if uniq else capi.MK_MODE_SET, one_buffer=uniq)
        res = eng.batch_end()
        assert len(res) == len(texts)
        for i, (st, alone, comps) in enumerate(res):
            assert st == 0, (name, i, st)
            assert_same([(c, None) for c in comps], want[i], "%s uniq=%s file %d (alone=%d)" % (name, uniq, i, alone))
        if name == wc.SATURATE:
            assert sum(alone for _, alone, _ in res) >= 3, "the small per-file tables were meant to overflow"


# ---- 4. FASTQ set -------------------------------------------------------------------------------------------------------------------
def check_fastq_set(capi, eng, name, want_for, M, Q):
    data = wc.get_input(name).fastq()
    want = want_for(name, "occ", M, Q)
    n_ids = sum(len(w[0]) for w in want)
    # every k-mer is planted once, three in ten twice, a hundred sixteen times; a window survives -Q 53 when none of its 2k quality
    # bytes is '#' or '+' (4 % of the bytes): about 0.96^2k = 0.27-0.38 of the occurrences
    floor = {(1, 0): wc.MIN_KEYS[name], (1, 53): wc.MIN_KEYS[name] // 8, (2, 0): 500, (2, 53): 50, (7, 0): 50, (7, 53): 1}[(M, Q)]
    assert n_ids >= floor, (name, M, Q, n_ids)
    TL = 2 * wc.GEOMS[name][0]
    rows, n, nrec, used, rc = capi.fastq_frame_q(data, 304, TL, qmin=Q)
    assert rc == 0 and used == len(data)
    eng.begin_occ(M)
    eng.push_reads(rows, 304, 0)
    got = eng.finish()
    assert all(g[1] is None for g in got)
    assert_same(got, want, "%s M=%d Q=%d" % (name, M, Q))
    if (M, Q) == (2, 53):
        assert_is_fixture(got, name + "_fq_n2Q53")


@pytest.mark.parametrize("Q", [0, 53])
@pytest.mark.parametrize("M", [1, 2, 7])
@pytest.mark.parametrize("name", ["W12S5D5", "W13S6D5"])
def test_fastq_set_light(capi, engine_for, want_for, name, M, Q):
    check_fastq_set(capi, engine_for(name), name, want_for, M, Q)


# ---- 5. by-read ids and reverse through the ABI -------------------------------------------------------------------------------------
def same_byread(got, want_ids, want_index, tag):
    ids, index = got[0], got[1]
    assert len(ids) == len(want_ids)
    for c in range(len(ids)):
        assert np.array_equal(ids[c], want_ids[c]), (tag, "ids", c, len(ids[c]), len(want_ids[c]))
        assert np.array_equal(index[c], want_index[c]), (tag, "index", c)


def check_byread_abi(h, name):
    P = wc.params(name)
    text = wc.get_input(name).fasta()
    want_ids, want_index = bm.byread(text, P)
    assert sum(len(x) for x in want_ids) >= wc.MIN_KEYS[name]
    got = h.run(text)
    same_byread(got, want_ids, want_index, name)
    ids, index, records, _ = got
    rev = wc.rev_table(name)  # (the model's inverse table once, not per call: a pass over 16^subk entries)
    lines = [h.reverse_ids(ids[c], c) for c in range(len(ids))]
    for c in range(len(ids)):
        assert lines[c] == bm.kmer_lines(ids[c], c, P, rev), (name, "reverse", c)
    case = name + "_byread"
    if case in BYREAD_CASES:  # the reference's files, and its `reverse -b` text by the cursor rule
        e = BYREAD_CASES[case]
        assert records == e["records"] and sum(len(x) for x in ids) == e["ids"]
        for c in range(len(ids)):
            assert ids[c].tobytes() == open(os.path.join(GOLD, case, "combco.%d" % c), "rb").read(), (case, c)
            assert index[c].tobytes() == open(os.path.join(GOLD, case, "combco.index.%d" % c), "rb").read(), (case, c)
        W = P.TL + 1
        out, cur = [], [0] * len(ids)
        for n in range(records):
            out.append(b">read %d\n" % (n + 1))
            for c in range(len(ids)):
                k = int(index[c][n + 1]) - int(index[c][n])
                out.append(lines[c][cur[c] * W:(cur[c] + k) * W])
                cur[c] += k
        assert b"".join(out) == gzip.open(os.path.join(GOLD, case, "reverse_b.txt.gz")).read()
    # ids over the whole id range (the top bits of a 32-bit id, every component end)
    rs = np.random.RandomState(33)
    id_bits = 4 * (P.k - P.drlevel) - P.comp_code_bits
    for c in sorted({0, P.component_num - 1}):
        rid = np.concatenate((rs.randint(0, 1 << id_bits, size=100003, dtype=np.int64), [0, (1 << id_bits) - 1])).astype(np.uint32)
        assert h.reverse_ids(rid, c) == bm.kmer_lines(rid, c, P, rev), (name, "random ids", c)


@pytest.mark.parametrize("name", LIGHT_BYREAD)
def test_byread_abi_light(handles, name):
    """hob = 2(k - subk) reaches 14-16 bits, the drtuple 32-36 bits before the component is taken off"""
    check_byread_abi(handles(name), name)


def test_byread_chunk_invariance(handles):
    """(13,6,5): the same text whole, byte by byte over its first 300 bytes, and in pieces of 63, 1 023, 1 024 and 1 025 bytes"""
    h = handles("W13S6D5")
    text = wc.get_input("W13S6D5").fasta()[:60000]
    whole = h.run(text)
    same_byread(whole, *bm.byread(text, wc.params("W13S6D5")), tag="whole")
    assert sum(len(x) for x in whole[0]) > 500
    for tag, cuts in [("bytewise", list(range(1, 301)))] + [(str(s), list(range(s, len(text), s))) for s in (63, 1023, 1024, 1025)]:
        got = h.run(text, pieces=cuts)
        same_byread(got, whole[0], whole[1], tag)
        assert got[2] == whole[2]


# ---- 6. command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuf_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("widek_shufs")
    made = {}

    def get(name):
        if name not in made:
            p = str(d / (name + ".shuf"))
            wc.get_shuf(name).write(p)
            made[name] = p
        return made[name]
    yield get
    for p in made.values():
        os.remove(p)


def run_cli(args, cwd):
    r = subprocess.run([BIN] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, (args, r.stderr.decode(errors="replace")[-500:])
    return r.stdout


def check_cli_dist(case, shuf_files, tmp_path):
    e = CASES[case]
    inp = write_input(e["geometry"], e["input"], tmp_path)
    out = str(tmp_path / "out")
    run_cli(["dist", "-L", shuf_files(e["geometry"])] + e["flags"] + ["-p", "8", "-o", out, inp], tmp_path)
    check_dist_dir(case, out, inp)


def check_cli_reverse(name, shuf_files, tmp_path):
    """`dist --byread` + `reverse -b`, and plain `reverse -o` on the reference-made sketch directory"""
    shuf = shuf_files(name)
    case = name + "_byread"
    inp = write_input(name, "fa", tmp_path)
    out = str(tmp_path / "br")
    run_cli(["dist", "-L", shuf, "--byread", "-o", out, inp], tmp_path)
    want = sorted(f for f in BYREAD_CASES[case]["files"] if f.startswith("combco"))
    assert sorted(f for f in os.listdir(out) if f.startswith("combco")) == want
    for f in want:
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(GOLD, case, f), "rb").read(), (case, f)
    assert run_cli(["reverse", "-L", shuf, "-b", out], tmp_path) == gzip.open(os.path.join(GOLD, case, "reverse_b.txt.gz")).read(), case
    case = name + "_reverse"
    e = build_sketch_dir(case, str(tmp_path / "sk"))
    (tmp_path / "kmers").mkdir()
    run_cli(["reverse", "-L", shuf, "-o", str(tmp_path / "kmers"), str(tmp_path / "sk")], tmp_path)
    assert sorted(os.listdir(str(tmp_path / "kmers"))) == sorted(e["outputs"])
    for f in e["outputs"]:
        assert open(str(tmp_path / "kmers" / f), "rb").read() == gzip.open(os.path.join(GOLD, case, "kmers", f + ".gz")).read(), (case, f)


@pytest.mark.parametrize("case", sorted(c for c in CASES if CASES[c]["geometry"] in wc.LIGHT))
def test_cli_dist_reproduces_reference_light(case, shuf_files, tmp_path):
    check_cli_dist(case, shuf_files, tmp_path)


def test_cli_reverse_reproduces_reference_light(shuf_files, tmp_path):
    check_cli_reverse("W13S6D5", shuf_files, tmp_path)


# ---- 7. poison ----------------------------------------------------------------------------------------------------------------------
def test_handle_tests_under_poison():
    """MK_POISON fills every allocation of the library before use (read once per process: a process of its own): the handle tests of
    the light geometries again -- a kernel that read what nobody wrote would not match"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k",
                        "counted_rows_light or fasta_device_stream_light or byread_abi_light"], env=dict(os.environ, MK_POISON="0xA5"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and " passed" in out and "32 passed" in out, out[-3000:]


# ---- fuzz ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [21, 22])
def test_randomized_engine_vs_oracle_wide_k(seed):
    """tools/fuzz_parity.py --geom: its flavours, strides, pushes, merges and dirty reads drawn over the five light geometries"""
    geoms = sum((["--geom", "%d,%d,%d" % wc.GEOMS[n][:3]] for n in wc.LIGHT), [])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), "--cases", "150", "--seed", str(seed)] + geoms,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "150 cases, 0 mismatches" in out, out[-1500:]


# ---- the heavy geometries: 536 870 909 slots, sixteen components; each in the tests named here and nowhere else -----------------------
def test_k16_table_is_generated_once():
    """the (16,7,7) .shuf: 16^7 entries (1 GiB), some seconds of host time paid here, once per module, and by no other test"""
    t = wc.get_shuf("W16S7D7").table
    assert t.size == 16 ** 7 and int(np.count_nonzero(t < 4096)) == 4096 and wc.get_shuf("W16S7D7") is wc.get_shuf("W16S7D7")
    assert wc.rev_table("W16S7D7") is not None


@pytest.mark.parametrize("name", wc.HEAVY)
def test_counted_rows_heavy(capi, engine_for, want_for, name):
    """(12,6,3) unclamped; (15,6,6) 60-bit unituples; (16,7,7) the full 64 bits: tupmask and the reverse complement shift by 0,
    28 inner bits against a 14-bit filter index"""
    check_counted_rows(capi, engine_for(name), name, want_for, 160, 1)


@pytest.mark.parametrize("uniq", [False, True])
def test_fasta_device_stream_k16(capi, engine_for, want_for, uniq):
    check_fasta_stream(capi, engine_for("W16S7D7"), "W16S7D7", want_for, uniq)


@pytest.mark.parametrize("Q", [0, 53])
@pytest.mark.parametrize("M", [1, 2, 7])
def test_fastq_set_k15(capi, engine_for, want_for, M, Q):
    check_fastq_set(capi, engine_for("W15S6D6"), "W15S6D6", want_for, M, Q)


@pytest.mark.parametrize("name", ["W12S6D3", "W16S7D7"])
def test_byread_abi_heavy(handles, name):
    check_byread_abi(handles(name), name)


def test_recovered_kmers_occur_in_their_record(handles):
    """(12,6,3), the only unclamped geometry here: every k-mer `reverse` gives back for a record's ids occurs in that record, on one
    strand (needs no model)"""
    h = handles("W12S6D3")
    recs = [b"".join(r.upper() for r in wc.get_input("W12S6D3").rows[i:i + 40]) for i in range(0, 1160, 40)]
    text = b"".join(b">r%d\n" % i + b"\n".join(r[j:j + 60] for j in range(0, len(r), 60)) + b"\n" for i, r in enumerate(recs))
    ids, index, records, _ = h.run(text)
    assert records == len(recs)
    W = h.params.TL + 1
    total = 0
    for c in range(len(ids)):
        assert index[c][0] == 0 and index[c][-1] == len(ids[c])
        lines = h.reverse_ids(ids[c], c)
        for n, r in enumerate(recs):
            both = r + b"|" + r.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
            for i in range(int(index[c][n]), int(index[c][n + 1])):
                kmer = lines[i * W:(i + 1) * W - 1]
                assert lines[(i + 1) * W - 1:(i + 1) * W] == b"\n" and kmer in both, (c, n, kmer)
                total += 1
    assert total >= 2000


@pytest.mark.parametrize("case", sorted(c for c in CASES if CASES[c]["geometry"] in ("W12S6D3", "W15S6D6")) + ["W16S7D7_fq_A"])
def test_cli_dist_reproduces_reference_heavy(case, shuf_files, tmp_path):
    """every fixture directory of (12,6,3) and (15,6,6); one case for (16,7,7), the only test that writes its 1 GiB .shuf"""
    check_cli_dist(case, shuf_files, tmp_path)


def test_cli_reverse_reproduces_reference_unclamped(shuf_files, tmp_path):
    check_cli_reverse("W12S6D3", shuf_files, tmp_path)
