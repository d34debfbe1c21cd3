"""A concatenation of gzip members inflated by many wavefronts (MK_GUNZIP_MEMBERS: mk_inflate_stream, mk_sketch_push_gzip,
`dist -A --device-gunzip --gunzip-members`): the text against zlib byte for byte, the piece table with its kinds and
every status against tests/gunzip_members_model.py, the member count against the true one, and the command line against the golden
directories and the run without switches."""
import filecmp
import functools
import gzip
import json
import os
import subprocess

import pytest

import bgzf_util as bu
import golden_cases as gc
import gunzip_model as gm
import gunzip_members_model as mm
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
MANIFEST = json.load(open(os.path.join(gc.GOLDEN, "manifest.json")))
TEXT = bu.golden_text("fq_ragged")
SPANS = (256, 1024, 65536)
RATIO = 1040  # no deflate stream gives more than 1032 bytes a compressed byte: with this R no legal piece can meet its capacity
LEGAL = {n: (f, t) for n, f, t in mm.legal_files(TEXT)}
STATUS = {n: (f, w) for n, f, w in mm.status_files(TEXT)}
assert (capi.MK_INFL_BAD_MEMBER, capi.MK_INFL_MISSED, capi.MK_INFL_CRC, capi.MK_INFL_OUTPUT_LEN, capi.MK_INFL_BAD_DISTANCE) == \
    (mm.BAD_MEMBER, mm.MISSED, mm.CRC, mm.OUTPUT_LEN, mm.BAD_DISTANCE)


@functools.lru_cache(maxsize=None)
def model(name, span):
    return mm.run_file(LEGAL[name][0], span, RATIO)


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


def status_text(st):
    return capi.lib.mk_gunzip_status_text(st).decode()


def check(infl, f, text, span, want, **kw):
    """want: the model's (status OK, text, pieces, members)"""
    assert want[0] == mm.OK and want[1] == text == gzip.decompress(f)
    got, st, pieces, n, members = infl.stream(f, span_bytes=span, ratio=RATIO, cap=len(text), members=True, **kw)
    assert st == 0, status_text(st)
    assert n == len(text) and got == text
    assert pieces == want[2]
    assert members == len(want[3])
    return pieces


def expect_status(infl, f, want, span, **kw):
    got, st, pieces, n, members = infl.stream(f, span_bytes=span, ratio=RATIO, cap=1 << 20, members=True, **kw)  # (guards are checked in there)
    assert st == want, "%s, not %s" % (status_text(st), status_text(want))
    assert got is None


@pytest.mark.parametrize("span", SPANS)
def test_two_members(infl, span):
    f, text = LEGAL["two_l6_m1"]
    pieces = check(infl, f, text, span, model("two_l6_m1", span))
    assert span > 256 or len(pieces) > 100
    nspans = (len(f) + span - 1) // span
    for batch in (1, 8):  # a boundary and a member's CRC cross batches
        if batch < nspans:
            check(infl, f, text, span, model("two_l6_m1", span), batch_spans=batch)


def test_163_members_fail_without_the_flag(infl):
    f, text = LEGAL["m600"]
    assert f.count(b"\x1f\x8b\x08") == 163
    pieces = check(infl, f, text, 256, model("m600", 256))
    assert len(pieces) > 100 and all(kind == mm.MEMBER for _, kind, _ in pieces[1:])
    check(infl, f, text, 256, model("m600", 256), batch_spans=8)
    pieces = check(infl, f, text, 65536, model("m600", 65536))
    assert pieces == [(0, mm.BLOCK, len(TEXT))]
    assert model("m600", 65536)[3] == model("m600", 256)[3] and len(model("m600", 256)[3]) == 163
    assert infl.stream(f, span_bytes=256, ratio=RATIO)[1] == capi.MK_INFL_TRAILING  # without the flag, as ever


@pytest.mark.parametrize("k", range(1, 9))
def test_boundary_at_every_bit_alignment(infl, k):
    f, text = LEGAL["align_%d" % k]
    for span in SPANS:
        check(infl, f, text, span, model("align_%d" % k, span))


@pytest.mark.parametrize("name", ["fextra", "fname", "fcomment", "fhcrc", "all_four"])
def test_header_variants_on_the_second_member(infl, name):
    f, text = LEGAL[name]
    for span in SPANS:
        check(infl, f, text, span, model(name, span))


def test_fextra_across_a_span_and_a_batch_boundary(infl):
    f, text = LEGAL["fextra_700"]
    h, pay, _ = mm.split_file(f)
    at = f.index(b"\x1f\x8b\x08\x04", 10) - h  # the second header in the payload
    assert at // 256 != (at + 12 + 700) // 256
    for span in SPANS:
        check(infl, f, text, span, model("fextra_700", span))
    check(infl, f, text, 256, model("fextra_700", 256), batch_spans=1)
    check(infl, f, text, 1024, model("fextra_700", 1024), batch_spans=1)


@pytest.mark.parametrize("name", ["empty_first", "empty_middle", "empty_last", "empty_three"])
def test_empty_members(infl, name):
    f, text = LEGAL[name]
    for span in SPANS:
        check(infl, f, text, span, model(name, span))
    check(infl, f, text, 256, model(name, 256), batch_spans=1)
    assert [n for n, _, _ in model(name, 1024)[3]].count(0) == (3 if name == "empty_three" else 1)


def test_member_piece_without_symbols(infl):
    f, text, span = mm.zero_symbol_file(TEXT)
    want = mm.run_file(f, span, RATIO)
    assert [t for t in want[2] if t[1] == mm.MEMBER and t[2] == 0]
    check(infl, f, text, span, want)
    check(infl, f, text, span, want, batch_spans=1)
    for s in SPANS:
        check(infl, f, text, s, model("zero_symbols", s))


@pytest.mark.parametrize("name", ["stored_only", "fixed_only"])
def test_members_that_open_with_stored_and_fixed_blocks(infl, name):
    f, text = LEGAL[name]
    h, pay, _ = mm.split_file(f)
    second = f.index(b"\x1f\x8b\x08", 10) - h
    for span in SPANS:
        pieces = check(infl, f, text, span, model(name, span))
        assert (8 * second, mm.MEMBER) not in [p[:2] for p in pieces]  # never a piece start


@pytest.mark.parametrize("name", sorted(STATUS))
def test_statuses(infl, name):
    f, want = STATUS[name]
    for span in SPANS:
        assert mm.run_file(f, span, RATIO)[0] == want
        expect_status(infl, f, want, span)
    expect_status(infl, f, want, 256, batch_spans=1)


def test_false_member_start_is_missed(infl):
    f, text = mm.missed_file()
    assert mm.run_file(f, 1024, RATIO)[0] == mm.MISSED
    expect_status(infl, f, capi.MK_INFL_MISSED, 1024)
    check(infl, f, text, 65536, mm.run_file(f, 65536, RATIO))


def test_without_the_flag_nothing_changed(infl):
    f, text = LEGAL["two_l6_m1"]
    _, pay, _ = mm.split_file(f)
    for span in SPANS:
        mst, _, want = gm.run(pay, span, RATIO)  # the parent's model over the same payload
        got, st, pieces, n = infl.stream(f, span_bytes=span, ratio=RATIO)
        assert mst == gm.TRAILING and st == capi.MK_INFL_TRAILING and got is None
        assert pieces == want


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuf_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shuf")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = str(d / (name + ".shuf"))
            gc.make_shuf(name, cache[name])
        return cache[name]
    return get


def run_cli(shuf, flags, out, inp, extra=(), env=None):
    r = subprocess.run([CLI, "dist", "-L", shuf] + list(flags) + ["-p", "4", "--quiet", "--timing", "-o", out] + list(extra) + [inp],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    routes = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return r, routes


def same_dir(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and "cofiles.stat" in fa
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def golden_text_of(case):
    kind, base, *variant = gc.CASES[case]["input"].split(":")
    v = variant[0] if variant else ""
    return bu.golden_text("fq_%s%s" % (base, "_" + v if v in ("crlf", "trunc", "nonl") else ""))


def five_members(text):
    """cut where no record starts: a record straddles every boundary"""
    cuts = [len(text) * k // 5 for k in range(6)]
    for k in range(1, 5):
        while text[cuts[k] - 1:cuts[k]] == b"\n":
            cuts[k] += 1
    parts = [text[a:b] for a, b in zip(cuts, cuts[1:])]
    assert b"".join(parts) == text and all(parts)
    return b"".join(mm.gz(gm.deflate(p, 6, 1), p) for p in parts)


FQ_A_CASES = sorted(c for c, e in gc.CASES.items() if e["flags"] == ["-A"] and e["input"].startswith("fq:") and c in MANIFEST["cases"])
SECOND = next(c for c in FQ_A_CASES if c not in ("pool2000_L1K7", "key0_L0K6z"))
GUNZIP = ["--device-gunzip", "--gunzip-span-bytes", "1024"]
MEMBERS = GUNZIP + ["--gunzip-members"]


@pytest.mark.parametrize("case", ["pool2000_L1K7", SECOND])
def test_cli_five_members(case, shuf_files, tmp_path):
    entry = MANIFEST["cases"][case]
    assert not entry["aborted"]
    text = golden_text_of(case)
    f = five_members(text)
    assert gzip.decompress(f) == text
    inp = str(tmp_path / (case + ".fq.gz"))
    open(inp, "wb").write(f)
    shuf = shuf_files(entry["shuf"])
    plain = str(tmp_path / "plain")
    r, routes = run_cli(shuf, entry["flags"], plain, inp)
    assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    exp = os.path.join(gc.GOLDEN, "expected", case)
    env = dict(os.environ, MK_POISON="0xA5")
    for k, (extra, e) in enumerate(((MEMBERS, None), (MEMBERS + ["--gunzip-batch-spans", "8"], env))):
        out = str(tmp_path / ("dev%d" % k))
        r, routes = run_cli(shuf, entry["flags"], out, inp, extra, env=e)
        assert r.returncode == 0, r.stderr.decode()
        assert [x["route"] for x in routes] == ["device-gunzip"], "the device route was not taken: %s" % routes
        assert routes[0]["members"] == 5 and routes[0]["text_bytes"] == len(text) and routes[0]["pieces"] > 5
        assert k == 0 or routes[0]["batches"] > 1
        same_dir(plain, out)
        for name in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, name), os.path.join(out, name), shallow=False), "%s: %s differs from the reference" % (case, name)
    old = str(tmp_path / "old")
    r, routes = run_cli(shuf, entry["flags"], old, inp, GUNZIP)  # the switch alone: as ever
    assert r.returncode == 0, r.stderr.decode()
    assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", "more members behind the first")]
    same_dir(plain, old)


def test_cli_zero_padding_falls_back_loudly(shuf_files, tmp_path):
    case = "pool2000_L1K7"
    entry = MANIFEST["cases"][case]
    text = golden_text_of(case)
    inp = str(tmp_path / "padded.fq.gz")
    open(inp, "wb").write(five_members(text) + bytes(512))
    shuf = shuf_files(entry["shuf"])
    a, b = str(tmp_path / "plain"), str(tmp_path / "dev")
    ra, routes = run_cli(shuf, entry["flags"], a, inp)
    assert [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    rb, routes = run_cli(shuf, entry["flags"], b, inp, MEMBERS)
    assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", status_text(capi.MK_INFL_BAD_MEMBER))]
    assert status_text(capi.MK_INFL_BAD_MEMBER) not in ("unknown status", "")
    assert ra.returncode == rb.returncode
    same_dir(a, b)
