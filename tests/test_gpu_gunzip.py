"""One gzip member inflated by many wavefronts (mk_inflate_stream, mk_sketch_push_gzip, `dist -A --device-gunzip`): the text against
zlib byte for byte, the piece table against tests/gunzip_model.py, malformed streams with their exact status and guards on both
sides of the text buffer, and the command line against the golden directories and the `zcat -fc` route."""
import filecmp
import functools
import json
import os
import struct
import subprocess
import zlib

import pytest

import bgzf_util as bu
import golden_cases as gc
import gunzip_model as gm
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
MANIFEST = json.load(open(os.path.join(gc.GOLDEN, "manifest.json")))
TEXT = bu.golden_text("fq_ragged")
STREAMS = gm.legal_streams(TEXT)
BY_NAME = {n: (raw, text) for n, raw, text in STREAMS}
SPANS = (256, 1024, 65536)
assert (capi.MK_INFL_MISSED, capi.MK_INFL_CAPACITY, capi.MK_INFL_TRAILING, capi.MK_INFL_CRC) == (gm.MISSED, gm.CAPACITY, gm.TRAILING, gm.CRC)


def gz(raw, text, extra=None, name=None, comment=None, hcrc=False, crc=None, isize=None):
    """one gzip member around a raw deflate stream"""
    flg = (4 if extra is not None else 0) | (8 if name else 0) | (16 if comment else 0) | (2 if hcrc else 0)
    head = bytes([0x1f, 0x8b, 8, flg]) + b"\0\0\0\0\x00\x03"
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name:
        head += name + b"\0"
    if comment:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) if isize is None else isize) & 0xffffffff)


@functools.lru_cache(maxsize=None)
def model(name, span, ratio=1 << 20):
    return gm.run(BY_NAME[name][0], span, ratio)


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


RATIO = 1040  # no deflate stream gives more than 1032 bytes a compressed byte: with this R no legal piece can meet its capacity


def check(infl, f, raw, text, span, want_pieces=None, **kw):
    kw.setdefault("ratio", RATIO)
    got, st, pieces, n = infl.stream(f, span_bytes=span, **kw)
    assert st == 0, capi.lib.mk_inflate_status_text(st).decode()
    assert n == len(text) and got == text
    if want_pieces is None:
        mst, mtext, want_pieces = gm.run(raw, span)
        assert mst == gm.OK and mtext == text
    assert pieces == want_pieces
    return pieces


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("name", [n for n, _, _ in STREAMS])
def test_stream_equals_zlib_and_the_models_pieces(infl, name, span):
    raw, text = BY_NAME[name]
    mst, mtext, want = model(name, span)
    assert mst == gm.OK and mtext == text == zlib.decompress(raw, -15)
    pieces = check(infl, gz(raw, text), raw, text, span, want)
    if span == 256 and name in ("l1_m1", "l6_m1", "l9_m1", "repeat_20k_x10", "sync_flush", "full_flush"):
        assert len(pieces) > 20
    if name in ("fixed_only", "stored_only", "empty", "no_complete_record", "l6_m9"):
        assert len(pieces) == 1  # no non-final dynamic block start: spans without a candidate, the piece in front decodes through


def test_every_payload_alignment(infl):
    raw, text = BY_NAME["l6_m1"]
    want = model("l6_m1", 1024)[2]
    seen = set()
    for k in range(16):
        f = gz(raw, text, extra=bytes(k))
        seen.add(capi.gzip_scan_stream(f)["pay_off"] % 16)
        check(infl, f, raw, text, 1024, want)
    assert seen == set(range(16))


def test_header_variants(infl):
    raw, text = BY_NAME["l1_m2"]
    want = model("l1_m2", 1024)[2]
    for kw in (dict(name=b"reads.fastq"), dict(extra=b"xy" * 150), dict(comment=b"a comment"), dict(hcrc=True),
               dict(extra=b"q", name=b"n", comment=b"c", hcrc=True)):
        f = gz(raw, text, **kw)
        assert zlib.decompress(f, 31) == text  # the fixture itself
        check(infl, f, raw, text, 1024, want)


@pytest.mark.parametrize("name,span", [("l6_m1", 256), ("repeat_20k_x10", 256), ("l6_m9", 256), ("level0_between", 1024)])
def test_two_batches_and_many(infl, name, span):
    raw, text = BY_NAME[name]
    want = model(name, span)[2]
    nspans = (len(raw) + span - 1) // span
    for batch in ((nspans + 1) // 2, 8, 1):
        check(infl, gz(raw, text), raw, text, span, want, batch_spans=batch)


def expect_status(infl, f, want, span=1024, **kw):
    got, st, pieces, n = infl.stream(f, span_bytes=span, **kw)  # (guards on both sides of the text buffer are checked in there)
    assert st == want, "%s, not %s" % (capi.lib.mk_inflate_status_text(st).decode(), capi.lib.mk_inflate_status_text(want).decode())
    assert got is None


def missed_stream():
    """a stored block whose bytes hold, just behind the start of span 1 (1024-byte spans), the image of a valid non-final dynamic
    block header; then a final block.  The finder takes the image for a block start, the piece in front decodes past it."""
    w = bu.BitWriter()
    bu.dynamic_block(w, bu.spread(257, {65: 2, 66: 2, 67: 2, 256: 2}), [1, 1], [], 0, stop="ops")
    image = w.done()
    data = bytearray(b"\xff" * 3000)
    at = 1030 - 5  # the stored bytes start at payload byte 5
    data[at:at + len(image)] = image
    w = bu.BitWriter()
    bu.stored_block(w, bytes(data), 0)
    bu.fixed_block(w, list(b"@r\nACGT\n+\nIIII\n"), 1)
    raw = w.done()
    text = zlib.decompress(raw, -15)
    assert gm.header_valid(raw, 8 * 1030) and gm.find_candidates(raw, 1024)[0] == 8 * 1030
    return raw, text


def test_false_candidate_is_missed(infl):
    raw, text = missed_stream()
    assert gm.run(raw, 1024)[0] == gm.MISSED
    expect_status(infl, gz(raw, text), capi.MK_INFL_MISSED)
    check(infl, gz(raw, text), raw, text, 65536)  # one span: no finder, the stream is fine


def test_capacity(infl):
    text = b"A" * (1 << 20)
    raw = gm.deflate(text, 6, 9)
    assert gm.run(raw, 1024, 8)[0] == gm.CAPACITY
    expect_status(infl, gz(raw, text), capi.MK_INFL_CAPACITY, ratio=8)
    raw, text = BY_NAME["l6_m1"]
    assert gm.run(raw, 256, 2)[0] == gm.CAPACITY
    expect_status(infl, gz(raw, text), capi.MK_INFL_CAPACITY, span=256, ratio=2)


def test_damage_gives_its_status(infl):
    raw, text = BY_NAME["stored_only"]
    bad = bytearray(raw); bad[len(raw) // 2] ^= 0x10  # a stored byte: only the CRC can tell
    expect_status(infl, gz(bytes(bad), text), capi.MK_INFL_CRC)
    raw, text = BY_NAME["l6_m1"]
    for at in (len(raw) // 3, len(raw) // 2):
        bad = bytearray(raw); bad[at] ^= 0x04
        mst, mtext, _ = gm.run(bytes(bad), 1024)
        want = mst if mst else capi.MK_INFL_OUTPUT_LEN if len(mtext) != len(text) else capi.MK_INFL_CRC
        assert want and mtext != text
        expect_status(infl, gz(bytes(bad), text), want)
    expect_status(infl, gz(raw, text, crc=zlib.crc32(text) ^ 0x8000), capi.MK_INFL_CRC)
    expect_status(infl, gz(raw, text, isize=len(text) - 1), capi.MK_INFL_OUTPUT_LEN)
    expect_status(infl, gz(raw[:-300], text), gm.run(raw[:-300], 1024)[0])


def test_two_members_are_trailing(infl):
    raw, text = BY_NAME["l6_m1"]
    f = gz(raw, text) + gz(raw, text)
    assert zlib.decompress(f, 31) == text  # zlib stops behind the first member; zcat reads both
    expect_status(infl, f, capi.MK_INFL_TRAILING)
    small = gz(gm.deflate(b"@r\nAC\n+\nII\n"), b"@r\nAC\n+\nII\n")
    expect_status(infl, small + small, capi.MK_INFL_TRAILING)


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


FQ_A_CASES = sorted(c for c, e in gc.CASES.items() if e["flags"] == ["-A"] and e["input"].startswith("fq:") and c in MANIFEST["cases"])
GUNZIP = ["--device-gunzip", "--gunzip-span-bytes", "1024"]


@pytest.mark.parametrize("case", FQ_A_CASES)
def test_cli_gunzip_equals_zcat_route_and_reference(case, shuf_files, tmp_path):
    """One case, key0_L0K6z, is 37 KB of one repeated read in 645 compressed bytes: one span, so one piece, and 57 bytes of text a
    compressed byte, which the default R = 16 refuses by its own rule.  It must fall back loudly with equal files, and take the device
    route once the ratio hook allows it; every other case takes the device route with the default R and more than one piece."""
    entry = MANIFEST["cases"][case]
    assert not entry["aborted"]
    text = golden_text_of(case)
    raw = gm.deflate(text, 6, 1)
    mst, _, want = gm.run(raw, 1024, 16)
    inp = str(tmp_path / (case + ".fq.gz"))
    open(inp, "wb").write(gz(raw, text, name=b"reads.fq"))
    shuf = shuf_files(entry["shuf"])
    base = str(tmp_path / "zcat")
    r, routes = run_cli(shuf, entry["flags"], base, inp, ["--no-device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    plain = str(tmp_path / "plain")
    r, routes = run_cli(shuf, entry["flags"], plain, inp)  # without the switch: today's route
    assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    same_dir(base, plain)
    exp = os.path.join(gc.GOLDEN, "expected", case)
    runs = [(GUNZIP, mst)]
    if mst:
        assert (case, mst, len(raw) <= 1024) == ("key0_L0K6z", gm.CAPACITY, True)
        runs.append((GUNZIP + ["--gunzip-ratio", "64"], gm.OK))
        want = gm.run(raw, 1024, 64)[2]
    for k, (flags, status) in enumerate(runs):
        out = str(tmp_path / ("dev%d" % k))
        r, routes = run_cli(shuf, entry["flags"], out, inp, flags)
        assert r.returncode == 0, r.stderr.decode()
        if status:
            assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", capi.lib.mk_inflate_status_text(status).decode())]
        else:
            assert [x["route"] for x in routes] == ["device-gunzip"], "the device route was not taken"  # no silent fall-back
            assert routes[0]["text_bytes"] == len(text) and routes[0]["pieces"] == len(want)
            assert len(want) > 1 or len(raw) <= 1024
        same_dir(base, out)
        for f in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), "%s: %s differs from the reference" % (case, f)


def test_cli_batches_and_poison(shuf_files, tmp_path):
    case = "pool2000_L1K7"
    entry = MANIFEST["cases"][case]
    text = golden_text_of(case)
    inp = str(tmp_path / "pool.fq.gz")
    raw = gm.deflate(text, 6, 1)
    open(inp, "wb").write(gz(raw, text))
    exp = os.path.join(gc.GOLDEN, "expected", case)
    env = dict(os.environ, MK_POISON="0xA5")
    nspans = (len(raw) + 1023) // 1024
    for k, (batch, e) in enumerate(((8, None), ((nspans + 1) // 2, env), (0, env))):
        flags = GUNZIP + (["--gunzip-batch-spans", str(batch)] if batch else [])
        out = str(tmp_path / ("out%d" % k))
        r, routes = run_cli(shuf_files(entry["shuf"]), entry["flags"], out, inp, flags, env=e)
        assert r.returncode == 0, r.stderr.decode()
        assert [x["route"] for x in routes] == ["device-gunzip"] and routes[0]["pieces"] > 40
        assert routes[0]["pieces"] == nspans  # a piece a span: every batch has pieces
        assert routes[0]["batches"] == ((nspans + batch - 1) // batch if batch else 1)
        for f in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), f


def test_cli_statuses_fall_back_loudly_with_equal_files(shuf_files, tmp_path):
    shuf = shuf_files("L1K7")
    raw, text = BY_NAME["l6_m1"]
    mraw, mtext = missed_stream()
    one = b"@r\n" + b"A" * 150 + b"\n+\n" + b"I" * 150 + b"\n"
    big = one * 3000
    files = {"missed": (gz(mraw, mtext), [], "a piece start that is no block start"),
             "capacity": (gz(gm.deflate(big, 6, 9), big), ["--gunzip-ratio", "8"], "a piece's text exceeds its capacity"),
             "two_members": (gz(raw, text) + gz(raw, text), [], "more members behind the first")}
    for name, (f, extra, why) in files.items():
        inp = str(tmp_path / (name + ".fq.gz"))
        open(inp, "wb").write(f)
        a, b = str(tmp_path / (name + "_zcat")), str(tmp_path / (name + "_dev"))
        r, routes = run_cli(shuf, ["-A"], a, inp)
        assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
        r, routes = run_cli(shuf, ["-A"], b, inp, GUNZIP + extra)
        assert r.returncode == 0, r.stderr.decode()
        assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", why)], name
        same_dir(a, b)


def test_cli_damaged_file_fails_with_zcats_message(shuf_files, tmp_path):
    raw, text = BY_NAME["l6_m1"]
    bad = bytearray(gz(raw, text))
    bad[10 + len(raw) // 2] ^= 0x04
    inp = str(tmp_path / "bad.fq.gz")
    open(inp, "wb").write(bytes(bad))
    outs = []
    for k, extra in enumerate(([], GUNZIP)):
        out = str(tmp_path / ("out%d" % k))
        r, routes = run_cli(shuf_files("L1K7"), ["-A"], out, inp, extra)
        err = r.stderr.decode()
        assert r.returncode != 0 and "bad.fq.gz" in err and "zcat" in err, err
        assert not os.path.exists(os.path.join(out, "cofiles.stat"))
        outs.append((r.returncode, err))
    assert outs[0] == outs[1]  # today's message and exit status
