"""The long route of the -n / -Q reader (`dist -n N -Q q --long-reads-q`, mk_sketch_push_fastq_long_q) without a GPU.

The fixtures of tests/golden/longreads_q were written by the real reference from the CHOPPED files (tests/longreads_q_cases.py,
tests/golden/make_golden_longreads_q.py).  Here: the oracle's fastq2co on the chopped file == fixture == an independent model in
Python (mask the whole reads column by column, walk them as wide rows, keep the keys seen at least M times); the model's record rule
and mask are those of the host framer on every truncation of a small file and on the dirty case; the seeded inputs still are what the
reference was run on and what they were built for; the command line refuses what the route cannot do, with exact text and status,
before the device is touched."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import longreads_cases as lc
import longreads_q_cases as qc
import test_cli_surface as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "longreads_q")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
run = cs.run


def sub(M, Q):
    return "n%d_Q%d" % (M, Q)


def fixture(case, M, Q):
    """[ids] per component, as the reference wrote them"""
    C = MANIFEST["cases"][case]["runs"][sub(M, Q)]["stat"]["comp_num"]
    return [np.fromfile(os.path.join(GOLD, case, sub(M, Q), "combco.%d" % c), dtype="<u4") for c in range(C)]


def same_ids(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def model(ora, text, M, Q):
    """the rule in Python: masked whole reads as wide rows through the reference's per-read loop, keys seen at least M times"""
    rows, stride = lc.rows_of(qc.masked(text, Q))
    rc, koc = ora.koc_from_rows(rows, stride)
    assert rc == 0
    return [ids[cnt >= M] for ids, cnt in koc]


@pytest.fixture(scope="module")
def oracles(oracle_for):
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = oracle_for(lc.get_shuf(geom))
        return made[geom]
    return get


def test_manifest_covers_every_case():
    assert sorted(MANIFEST["cases"]) == sorted(qc.FIXTURE_CASES)
    for case, e in MANIFEST["cases"].items():
        assert e["geometry"] == qc.CASES[case][1] and sorted(e["runs"]) == sorted(sub(M, Q) for M, Q in qc.MQ)
        assert e["longest_read"] > lc.FQ_MAX and e["pieces"] > e["reads"]
        for r in e["runs"].values():
            assert r["keys"] >= qc.MIN_KEYS[case] and r["stat"]["koc"] == 0 and r["stat"]["infile_num"] == 1 and r["stat"]["ctx_ct"] == [r["keys"]]
        k = {name: r["keys"] for name, r in e["runs"].items()}
        assert k["n2_Q53"] < k["n1_Q53"] < k["n1_Q0"]


def test_fixture_tree_equals_manifest():
    want = {os.path.join(case, name, f): h for case, e in MANIFEST["cases"].items() for name, r in e["runs"].items() for f, h in r["files"].items()}
    have = {os.path.relpath(os.path.join(dp, f), GOLD) for dp, _, fs in os.walk(GOLD) for f in fs} - {"manifest.json"}
    assert have == set(want)
    for rel, h in want.items():
        assert hashlib.sha256(open(os.path.join(GOLD, rel), "rb").read()).hexdigest() == h, "fixture changed: " + rel
        assert os.path.getsize(os.path.join(GOLD, rel)) <= 256 << 10


@pytest.mark.parametrize("case", qc.FIXTURE_CASES)
def test_inputs_are_what_the_reference_was_run_on(case, tmp_path):
    e = MANIFEST["cases"][case]
    assert hashlib.sha256(qc.fastq(case)).hexdigest() == e["fastq_sha256"]
    assert hashlib.sha256(qc.chopped(case)).hexdigest() == e["chopped_sha256"]
    p = str(tmp_path / "x.shuf")
    lc.get_shuf(e["geometry"]).write(p)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == MANIFEST["shufs"][e["geometry"]]
    assert max(len(ln) for ln in qc.chopped(case).split(b"\n")) <= lc.FQ_MAX < max(len(ln) for ln in qc.fastq(case).split(b"\n"))


@pytest.mark.parametrize("case", qc.FIXTURE_CASES)
def test_lengths_q_file_is_built_as_described(case):
    """lc.fastq's layout; a low byte on every offset of a 64-byte step and on both sides of a segment bound; low runs across the
    chopping boundaries; bytes equal to Q, to Q - 1 and at or above 0x80; about one byte in a hundred below Q"""
    text, base = qc.fastq(case), lc.fastq(qc.base_case(case))
    assert len(text) == len(base) and np.array_equal(lc.line_end_offsets(text), lc.line_end_offsets(base))
    assert [ln for i, ln in enumerate(text.split(b"\n")) if i % 4 != 3] == [ln for i, ln in enumerate(base.split(b"\n")) if i % 4 != 3]
    t = np.frombuffer(text, np.uint8)
    ends = lc.line_end_offsets(text)
    isq = np.zeros(len(t), bool)
    for a, b in zip(ends[2::4], ends[3::4]):
        isq[a + 1:b] = True
    low = isq & (t.view(np.int8) < qc.Q)
    at = np.flatnonzero(low)
    assert set(int(x) % 64 for x in at) == set(range(64))
    assert any(low[x + 1] for x in at if x % 1024 == 1023), "no low run across a segment bound"
    vals = set(int(x) for x in t[isq])
    assert {qc.Q, qc.Q - 1, 0x80, 0xFF} <= vals
    assert 0.005 < low.sum() / isq.sum() < 0.02
    tl, step = qc.TL(case), lc.FQ_MAX - (qc.TL(case) - 1)
    for q in qc.quals(case):
        lowq = np.frombuffer(q, np.int8) < qc.Q
        for cut in range(step, len(q), step):  # where a piece starts, and where the piece before it ends
            assert lowq[cut - 1] and lowq[cut]
            if cut - step + lc.FQ_MAX < len(q):
                assert lowq[cut - step + lc.FQ_MAX - 1] and lowq[cut - step + lc.FQ_MAX]
    assert tl - 1 < step


def test_chopping_keeps_every_window_with_its_qualities():
    rs = np.random.RandomState(6)
    for tl in (12, 14, 22):
        for n in (0, 1, tl, 4094, 4095, 4094 + 4094 - (tl - 1) + 1, 20000):
            s = bytes(rs.randint(65, 91, size=n).astype(np.uint8))
            q = bytes(rs.randint(33, 127, size=n).astype(np.uint8))
            pieces = qc.chop_q([s], [q], tl)
            assert [p for p, _ in pieces] == lc.chop([s], tl) and all(len(p) == len(x) for p, x in pieces)
            windows = [(p[i:i + tl], x[i:i + tl]) for p, x in pieces for i in range(len(p) - tl + 1)]
            assert windows == [(s[i:i + tl], q[i:i + tl]) for i in range(len(s) - tl + 1)]


@pytest.mark.parametrize("case", qc.FIXTURE_CASES)
def test_oracle_on_chopped_file_equals_model_equals_reference(case, oracles):
    ora = oracles(qc.CASES[case][1])
    sets = {}
    for M, Q in qc.MQ:
        rc, got = ora.co_from_fastq(qc.chopped(case), Q, M)
        assert rc == 0
        ids = [g[0] for g in got]
        assert same_ids(ids, fixture(case, M, Q)), "the oracle differs from the reference's directory at " + sub(M, Q)
        assert same_ids(model(ora, qc.fastq(case), M, Q), ids), "the Python model differs from the oracle at " + sub(M, Q)
        sets[(M, Q)] = {(c, int(x)) for c, a in enumerate(ids) for x in a}
        assert len(sets[(M, Q)]) >= qc.MIN_KEYS[case]
    assert sets[(1, 53)] < sets[(1, 0)] and sets[(2, 53)] and sets[(2, 53)] < sets[(1, 53)]


def framer_lines(text, tl, qmin, final=True):
    """the sequence lines the host framer (mk_fastq_frame_q, records_before = 0) gives for reads of at most 4 094 characters"""
    from metakssd_amd import capi
    rows, nrows, nrec, used, rc = capi.fastq_frame_q(text, 4096, tl, qmin=qmin, final=final)
    assert rc == 0 and nrows == nrec
    return [bytes(rows[i * 4096:(i + 1) * 4096]).split(b"\n")[0] for i in range(nrows)]


SMALL = b"@a\nACGTACGTACGTAAC\n+\nIIII5IIII4IIIII\n@b x\nTTGACCAGTACGTACG\n+b\n@III>II\x80IIIIIII\n@c\nGGATCCGATTACAGATTACA\n+\nIIIIIIIIIIIIIIIIII\n"


@pytest.mark.parametrize("qmin", [-128, 0, 11, 53, 74])
def test_record_rule_and_mask_of_the_model(qmin):
    """qc.masked against the host framer on every truncation of a small file: the record rule, the first-record exception, the '\\n' of a
    short quality line as its last column's quality (10: masked from qmin 11 on) and 0 behind it"""
    for n in range(len(SMALL) + 1):
        cut = SMALL[:n]
        assert qc.masked(cut, qmin) == framer_lines(cut, 12, qmin), n
    assert qc.masked(SMALL, 53)[0] == b"ACGTACGTANGTAAC" and qc.masked(SMALL, 53)[1][7] == ord("N")
    assert qc.masked(SMALL, 11)[2].endswith(b"TANN") and qc.masked(SMALL, 10)[2].endswith(b"TACN") and qc.masked(SMALL, 0)[2].endswith(b"TACA")


def test_the_two_record_rules_differ():
    """a last quality line without its '\\n' counts under -A's rule and not here"""
    cut = SMALL[:-1]
    assert len(lc.records(cut)) == 3 and len(qc.masked(cut, 0)) == 2


@pytest.mark.parametrize("case", [c for c in qc.CASES if qc.CASES[c][0] == "dirty_q"])
@pytest.mark.parametrize("qmin", [-128, 0, 53, 74])
def test_model_equals_host_framer_on_dirty_text(case, qmin):
    text = qc.fastq(case)
    lines = text.split(b"\n")
    assert max(len(ln) for ln in lines[1::4]) == lc.FQ_MAX  # reads of at most 4 094 characters: one row a record at stride 4 096
    short = [len(lines[4 * r + 1]) - len(lines[4 * r + 3]) for r in range(len(qc.reads(case)))]
    assert {1, 65} <= set(short) and min(short) < 0 and any(not lines[4 * r + 3] and lines[4 * r + 1] for r in range(len(short)))
    assert any(ln.endswith(b"\r") for ln in lines[3::4]) and any(b"@" in ln[1:] and b">" in ln for ln in lines[3::4])
    assert qc.masked(text, qmin) == framer_lines(text, qc.TL(case), qmin)


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_library_and_binding():
    h = open(os.path.join(ROOT, "include", "metakssd_hip.h")).read()
    assert re.search(r"\bint mk_sketch_push_fastq_long_q\(mk_engine \*e, const uint8_t \*text, uint64_t n, int final, int32_t qmin\);", h)
    assert re.search(r"\bint mk_sketch_push_fastq_long_q_device\(mk_engine \*e, const uint8_t \*d_text, uint64_t n, int final, int32_t qmin\);", h)
    assert re.search(r"\bint mk_sketch_push_gzip_long_q\(mk_engine \*e, int fd, size_t size, const mk_gunzip_opts \*opts, int32_t qmin, int final, mk_gunzip_stats \*st\);", h)
    assert re.search(r"\bint mk_sketch_push_bgzf_long_q\(mk_engine \*e, int fd, size_t size, const mk_bgzf_opts \*o, int32_t qmin, int final, mk_bgzf_stats \*st\);", h)
    comment = h[:h.index("int mk_sketch_push_fastq_long_q(")].rsplit("/*", 1)[1]  # the entry point cites the reference lines it stands for
    assert "iseq2comem.c:343-379" in comment and "mk_fastq_frame_q" in comment
    from metakssd_amd import capi
    for name in ("mk_sketch_push_fastq_long_q", "mk_sketch_push_fastq_long_q_device", "mk_sketch_push_gzip_long_q", "mk_sketch_push_bgzf_long_q"):
        fn = getattr(capi.lib, name)  # AttributeError: not in the library
        assert fn.argtypes is not None and ctypes.c_int32 in fn.argtypes
    for name in ("push_fastq_long_q", "push_fastq_long_q_device", "push_gzip_long_q", "push_bgzf_long_q"):
        assert callable(getattr(capi.Engine, name))


@pytest.fixture()
def world(tmp_path):
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    return dict(fq=str(fq), shuf=str(tmp_path / "none.shuf"), tmp=tmp_path)  # the .shuf is never read: every refusal comes first


def refused(text, *args):
    assert run("dist", *args) == (1, "", "metakssd: " + text + "\n")


SWITCHES = ["--long-reads-q", "--long-inflate-q"]


@pytest.mark.parametrize("sw", SWITCHES)
def test_with_A(world, sw):
    refused(sw + " does not go with -A: --long-reads is the route of the counted sketch", "-L", world["shuf"], "-A", "-n", "2", sw, world["fq"])
    refused(sw + " does not go with -A: --long-reads is the route of the counted sketch", "-L", world["shuf"], sw, "-A", world["fq"])


@pytest.mark.parametrize("sw", SWITCHES)
def test_with_byread(world, sw):
    out = world["tmp"] / "o"
    for args in (["--byread", sw], [sw, "-Q", "20", "--byread"]):
        refused(sw + " does not go with --byread: per-read sketches keep the framing contract", "-L", world["shuf"], "-o", out, *args, world["fq"])
    assert not out.exists()


@pytest.mark.parametrize("sw", SWITCHES)
def test_with_devices(world, sw):
    refused(sw + " works on one GPU: --device D, not --devices", "-L", world["shuf"], "-n", "2", sw, "--devices", "0,1", world["fq"])
    refused(sw + " works on one GPU: --device D, not --devices", "-L", world["shuf"], "--devices", "0", sw, world["fq"])


@pytest.mark.parametrize("sw", SWITCHES)
def test_with_composite(world, sw):
    refused(sw + " does not go with --composite: the report reads the counted sketch", "-L", world["shuf"], sw, "--composite", str(world["tmp"]), world["fq"])


@pytest.mark.parametrize("opt", ["--device-inflate", "--device-gunzip"])
def test_with_a_device_inflate_route(world, opt):
    for args in ([opt, "--long-reads-q"], ["--long-reads-q", opt]):
        refused("--long-reads-q reads .gz files through zcat: not --device-inflate or --device-gunzip", "-L", world["shuf"], "-Q", "53", *args, world["fq"])
    for args in ([opt, "--long-inflate-q"], ["--long-inflate-q", opt]):
        refused("--long-inflate-q chooses the device route itself: not --device-inflate or --device-gunzip", "-L", world["shuf"], *args, world["fq"])


@pytest.mark.parametrize("sw", SWITCHES)
@pytest.mark.parametrize("other", ["--long-reads", "--long-inflate"])
def test_with_the_A_routes_switches(world, sw, other):
    for args in ([sw, other], [other, "-A", sw]):
        refused("%s is the route of dist without -A: not with %s" % (sw, other), "-L", world["shuf"], *args, world["fq"])


@pytest.mark.parametrize("sw", ["--long-reads", "--long-inflate"])
def test_the_A_routes_switches_still_refuse_n_and_Q(world, sw):
    refused(sw + " does not take -n or -Q: their reader frames lines of up to 19998 characters itself", "-L", world["shuf"], "-A", sw, "-n", "2", world["fq"])


def test_refusals_need_no_device(world):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cs.CLI, "dist", "-L", world["shuf"], "--long-reads-q", "-A", world["fq"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"metakssd: --long-reads-q does not go with -A: --long-reads is the route of the counted sketch\n")


def test_usage_does_not_change():
    """tests/test_cli_surface.py pins the usage text; the switches are documented in the README and in the option loop"""
    assert run() == (2, "", cs.USAGE)
