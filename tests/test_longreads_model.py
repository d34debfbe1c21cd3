"""The long-read route (`dist -A --long-reads`, mk_sketch_push_fastq_long) without a GPU.

What the route must compute needs no new model: Oracle.koc_from_rows walks a row of any width with the reference's per-read loop
(iseq2comem.c:682-720), so one row per read at stride = longest read + 1 is the sketch wanted.  It is pinned to the reference itself
through the CHOPPED file (tests/longreads_cases.py): the fixtures of tests/golden/longreads were written by the real reference at -p 1
from those files (tests/golden/make_golden_longreads.py).  Here: oracle on wide rows == oracle on the chopped file == fixture, the
seeded inputs still are what the reference was run on and what they were built for, and the command line refuses what the route
cannot do, with exact text and status, before the device is touched."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import longreads_cases as lc
import test_cli_surface as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "longreads")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
run = cs.run


def fixture(case):
    """[(ids, counts)] per component, as the reference wrote them"""
    C = MANIFEST["cases"][case]["stat"]["comp_num"]
    return [(np.fromfile(os.path.join(GOLD, case, "combco.%d" % c), dtype="<u4"), np.fromfile(os.path.join(GOLD, case, "combco.%d.a.u16" % c), dtype="<u2"))
            for c in range(C)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def oracles(oracle_for):
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = oracle_for(lc.get_shuf(geom))
        return made[geom]
    return get


def test_manifest_covers_every_case():
    assert sorted(MANIFEST["cases"]) == sorted(lc.CASES)
    for case, e in MANIFEST["cases"].items():
        assert (e["kind"], e["geometry"]) == lc.CASES[case]
        assert e["keys"] >= lc.MIN_KEYS[case] and e["max_count"] > 1 and e["longest_read"] > lc.FQ_MAX and e["pieces"] > e["reads"]
        assert e["stat"]["koc"] == 1 and e["stat"]["infile_num"] == 1 and e["stat"]["ctx_ct"] == [e["keys"]]


def test_fixture_tree_equals_manifest():
    want = {os.path.join(case, f): h for case, e in MANIFEST["cases"].items() for f, h in e["files"].items()}
    have = {os.path.relpath(os.path.join(dp, f), GOLD) for dp, _, fs in os.walk(GOLD) for f in fs} - {"manifest.json"}
    assert have == set(want)
    for rel, h in want.items():
        assert hashlib.sha256(open(os.path.join(GOLD, rel), "rb").read()).hexdigest() == h, "fixture changed: " + rel
        assert os.path.getsize(os.path.join(GOLD, rel)) <= 256 << 10 and not rel.endswith(".a")


@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_inputs_are_what_the_reference_was_run_on(case, tmp_path):
    e = MANIFEST["cases"][case]
    assert hashlib.sha256(lc.fastq(case)).hexdigest() == e["fastq_sha256"]
    assert hashlib.sha256(lc.chopped(case)).hexdigest() == e["chopped_sha256"]
    p = str(tmp_path / "x.shuf")
    lc.get_shuf(e["geometry"]).write(p)
    assert hashlib.sha256(open(p, "rb").read()).hexdigest() == MANIFEST["shufs"][e["geometry"]]
    assert lc.records(lc.fastq(case)) == list(lc.reads(case))  # the file holds exactly these reads, by the record rule
    assert max(len(ln) for ln in lc.chopped(case).split(b"\n")) <= lc.FQ_MAX < max(len(ln) for ln in lc.fastq(case).split(b"\n"))


@pytest.mark.parametrize("geom", sorted(lc.GEOMS))
def test_lengths_file_is_built_as_described(geom):
    """every length the kernels change paths at, line ends on every offset of a 64-byte step and on both sides of a segment bound"""
    case, tl = "lengths_" + geom, lc.TL(geom)
    have = {len(s) for s in lc.reads(case)}
    assert have == set(lc.lengths(tl)) and {0, 1, tl - 1, tl, tl + 1, 4094, 4095, 4096, 8193, 70001} <= have
    text = lc.fastq(case)
    ends = lc.line_end_offsets(text)
    seq_ends = ends[1::4]  # the '\n' behind every sequence line
    assert len(seq_ends) == len(lc.reads(case)) == 68
    assert set(int(x) % 64 for x in seq_ends) == set(range(64))
    assert {1022, 1023, 0, 1} <= set(int(x) % 1024 for x in seq_ends)
    assert set(int(x) % 64 for x in ends) == set(range(64))


def test_chopping_keeps_every_window_once():
    """every window of tl characters of a read lies in exactly one piece, and the pieces keep the windows' order"""
    rs = np.random.RandomState(5)
    for tl in (12, 14, 22):
        for n in (0, 1, tl, 4094, 4095, 4094 + 4094 - (tl - 1), 4094 + 4094 - (tl - 1) + 1, 20000):
            s = bytes(rs.randint(65, 91, size=n).astype(np.uint8))
            pieces = lc.chop([s], tl)
            assert all(len(p) <= lc.FQ_MAX for p in pieces)
            windows = [p[i:i + tl] for p in pieces for i in range(len(p) - tl + 1)]
            assert windows == [s[i:i + tl] for i in range(len(s) - tl + 1)]


@pytest.mark.parametrize("case", sorted(lc.CASES))
def test_wide_rows_equal_chopped_file_equal_reference(case, oracles):
    ora = oracles(lc.CASES[case][1])
    rows, stride = lc.wide_rows(case)
    rc, wide = ora.koc_from_rows(rows, stride)
    assert rc == 0
    rc, chopped = ora.koc_from_fastq(lc.chopped(case))
    assert rc == 0
    assert same(wide, chopped), "the oracle's loop on whole reads and on their pieces differ"
    assert same(wide, fixture(case)), "the oracle differs from the reference's directory"
    keys = sum(len(w[0]) for w in wide)
    assert keys >= lc.MIN_KEYS[case] and max(int(w[1].max()) for w in wide if len(w[1])) > 1
    rows, stride = lc.truncated_rows(case)
    rc, cut = ora.koc_from_rows(rows, stride)
    assert rc == 0 and not same(wide, cut), "reads truncated at 4 094 characters give the same sketch: the case shows nothing"


def test_record_rule_of_the_model(oracles):
    """lc.records against the oracle's FASTQ reader on reads the reference takes whole: every truncation of a small file"""
    ora = oracles("L0K6")
    text = b"@a\nACGTACGTACGTAAC\n+\nIIIIIIIIIIIIIII\n@b x\nTTGACCAGTACGTACG\n+b\n@III>IIIIIIIIIII\n@c\nGGATCCGATTACAGATTACA\n+\nIIIIIIIIIIIIIIIIIIII\n"
    for n in range(len(text) + 1):
        cut = text[:n]
        rc, want = ora.koc_from_fastq(cut)
        rows, stride = lc.rows_of(lc.records(cut))
        rc2, got = ora.koc_from_rows(rows, stride)
        assert rc == 0 and rc2 == 0 and same(got, want), n


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def test_symbol_in_header_and_binding():
    h = open(os.path.join(ROOT, "include", "metakssd_hip.h")).read()
    assert re.search(r"\bint mk_sketch_push_fastq_long\(mk_engine \*e, const uint8_t \*text, uint64_t n, int final\);", h)
    comment = h[:h.index("int mk_sketch_push_fastq_long(")].rsplit("/*", 1)[1]  # the entry point cites the reference lines it stands for
    assert "iseq2comem.c:657-727" in comment and ":673" in comment and ":682-690" in comment
    from metakssd_amd import capi
    assert capi.lib.mk_sketch_push_fastq_long.argtypes is not None and callable(capi.Engine.push_fastq_long)


@pytest.fixture()
def world(tmp_path):
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    return dict(fq=str(fq), shuf=str(tmp_path / "none.shuf"), tmp=tmp_path)  # the .shuf is never read: every refusal comes first


def refused(text, *args):
    assert run("dist", *args) == (1, "", "metakssd: " + text + "\n")


def test_without_A(world):
    refused("--long-reads needs -A: it is the route of the counted sketch", "-L", world["shuf"], "--long-reads", world["fq"])


@pytest.mark.parametrize("opt", [("-n", "2"), ("-Q", "20")])
def test_with_n_or_Q(world, opt):
    refused("--long-reads does not take -n or -Q: their reader frames lines of up to 19998 characters itself", "-L", world["shuf"], "-A", "--long-reads",
            *opt, world["fq"])


def test_with_byread(world):
    out = world["tmp"] / "o"
    for args in (["--byread", "--long-reads"], ["--long-reads", "-A", "--byread"]):
        refused("--long-reads does not go with --byread: per-read sketches keep the framing contract", "-L", world["shuf"], "-o", out, *args, world["fq"])
    assert not out.exists()


def test_with_devices(world):
    refused("--long-reads works on one GPU: --device D, not --devices", "-L", world["shuf"], "-A", "--long-reads", "--devices", "0,1", world["fq"])
    refused("--long-reads works on one GPU: --device D, not --devices", "-L", world["shuf"], "--devices", "0", "-A", "--long-reads", world["fq"])


@pytest.mark.parametrize("opt", ["--device-inflate", "--device-gunzip"])
def test_with_a_device_inflate_route(world, opt):
    refused("--long-reads reads .gz files through zcat: not --device-inflate or --device-gunzip", "-L", world["shuf"], "-A", opt, "--long-reads", world["fq"])
    refused("--long-reads reads .gz files through zcat: not --device-inflate or --device-gunzip", "-L", world["shuf"], "-A", "--long-reads", opt, world["fq"])


def test_refusals_need_no_device(world):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cs.CLI, "dist", "-L", world["shuf"], "--long-reads", world["fq"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"metakssd: --long-reads needs -A: it is the route of the counted sketch\n")


def test_usage_does_not_change():
    """tests/test_cli_surface.py pins the usage text; the switch is documented in the README and in the option loop"""
    assert run() == (2, "", cs.USAGE)
