"""MK_GUNZIP_REPAIR on the device (mk_inflate_stream, mk_sketch_push_gzip / _q / _long / _long_q, `--gunzip-repair`):
the streams of tests/gunzip_repair_model.py with planted false piece starts.  With the flag the text is zlib's and status, final
piece table and repair count are the model's; without it every call gives what it gave before (MK_INFL_MISSED / MK_INFL_CAPACITY,
the fall-back to zcat); a clean stream gives the same tables with and without.  Streams are at most 64 KB, spans 256 / 1024 bytes."""
import filecmp
import functools
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_util as bu
import golden_cases as gc
import gunzip_model as gm
import gunzip_repair_model as rm
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

CLI = os.path.join(gc.ROOT, "metakssd_amd", "bin", "metakssd")
SPAN = rm.SPAN
RATIO = 1040  # no deflate stream gives more than 1032 bytes a compressed byte: with this R no legal piece can meet its capacity
assert (capi.MK_INFL_MISSED, capi.MK_INFL_CAPACITY, capi.MK_INFL_TRAILING, capi.MK_INFL_CRC) == (gm.MISSED, gm.CAPACITY, gm.TRAILING, gm.CRC)


def gz(raw, text, name=None):
    head = bytes([0x1f, 0x8b, 8, 8 if name else 0]) + b"\0\0\0\0\x00\x03" + (name + b"\0" if name else b"")
    return head + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def damaged(back):
    raw, text, bits = rm.four_images()
    bad = bytearray(raw)
    bad[len(raw) - back] ^= 0x04
    return bytes(bad), text, bits


def ragged():
    text = bu.golden_text("fq_ragged")
    return gm.deflate(text, 6, 1), text, []


def one_piece():
    text = b"A" * (1 << 20)
    return gm.deflate(text, 6, 9), text, []


# name -> (stream, span, ratio): every case of tests/test_gunzip_repair_model.py
CASES = {"missed_stream": (rm.missed_stream, SPAN, RATIO), "four_images": (rm.four_images, SPAN, RATIO), "two_rounds": (rm.two_rounds, SPAN, RATIO),
         "capacity_merges": (rm.four_images, SPAN, 4), "capacity_stands": (ragged, 256, 2), "capacity_last_piece": (one_piece, SPAN, 8),
         "damage_status": (functools.partial(damaged, 4000), SPAN, RATIO), "damage_crc": (functools.partial(damaged, 6000), SPAN, RATIO)}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (raw, text, planted bits, span, ratio, the model without the repair, the model with it): computed once, never changed"""
    make, span, ratio = CASES[name]
    raw, text, bits = make()
    return raw, text, bits, span, ratio, gm.run(raw, span, ratio), rm.run(raw, span, ratio)


def device_status(mst, mtext, text):
    """what the device says where the model's pieces are all OK: the trailer check"""
    return mst if mst else 0 if mtext == text else capi.MK_INFL_OUTPUT_LEN if len(mtext) != len(text) else capi.MK_INFL_CRC


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


def check_repaired(infl, name, **kw):
    raw, text, bits, span, ratio, _, (mst, mtext, mtable, mrep) = case(name)
    got, st, pieces, n, repairs = infl.stream(gz(raw, text), span_bytes=span, ratio=ratio, repair=True, **kw)  # (guards are checked in there)
    want = device_status(mst, mtext, text)
    assert st == want, "%s, not %s" % (capi.lib.mk_inflate_status_text(st).decode(), capi.lib.mk_inflate_status_text(want).decode())
    assert repairs == mrep
    if mst:  # the piece whose status stands is the table's last; what it had given when it stopped is not compared
        assert [s for s, _ in pieces] == [s for s, _ in mtable] and pieces[:-1] == mtable[:-1] and got is None
    else:
        assert pieces == mtable
    if want == 0:
        assert got == text == zlib.decompress(raw, -15) and n == len(text)
    return pieces


@pytest.mark.parametrize("name", sorted(CASES))
def test_repair_gives_the_models_status_table_and_count(infl, name):
    raw, text, bits, span, ratio, plain, (mst, mtext, mtable, mrep) = case(name)
    assert plain[0] in (gm.MISSED, gm.CAPACITY) and mrep > 0 or name == "capacity_last_piece"  # the fixture has something to repair
    check_repaired(infl, name)


@pytest.mark.parametrize("name", sorted(CASES))
def test_without_the_flag_nothing_changes(infl, name):
    raw, text, bits, span, ratio, (pst, _, ptable), _ = case(name)
    assert pst == (gm.CAPACITY if name.startswith("capacity") else gm.MISSED)
    for kw in ({}, {"repair": False}):
        got, st, pieces, n = infl.stream(gz(raw, text), span_bytes=span, ratio=ratio, **kw)
        assert (got, st) == (None, pst) and [s for s, _ in pieces] == [s for s, _ in ptable] and pieces[:-1] == ptable[:-1]
    nr = capi.C.c_uint64(7)
    assert capi.lib.mk_inflate_stream_repairs(infl.h, capi.C.byref(nr)) == 0 and nr.value == 0


LEGAL = gm.legal_streams(bu.golden_text("fq_ragged"))


@pytest.mark.parametrize("span", (256, 1024))
@pytest.mark.parametrize("name", [n for n, _, _ in LEGAL])
def test_a_clean_stream_costs_nothing(infl, name, span):
    raw, text = {n: (r, t) for n, r, t in LEGAL}[name]
    f = gz(raw, text)
    a = infl.stream(f, span_bytes=span, ratio=RATIO)
    b = infl.stream(f, span_bytes=span, ratio=RATIO, repair=True)
    assert a[:2] == (text, 0) and b == a + (0,)


def test_a_clean_file_keeps_its_pieces_and_batches(tmp_path):
    raw, text = {n: (r, t) for n, r, t in LEGAL}["l6_m1"]
    inp = str(tmp_path / "clean.fq.gz")
    open(inp, "wb").write(gz(raw, text))
    eng = capi.Engine(capi.Shuf.generate(*gc.SHUF_SPECS["L1K7"]), 0)
    try:
        out = []
        for repair in (False, True):
            eng.begin(capi.MK_MODE_KOC)
            st = eng.push_gzip(inp, span_bytes=SPAN, batch_spans=8, repair=repair)
            out.append((st.pieces, st.batches, st.text_bytes, st.rows, eng.gunzip_repairs(), result_key(eng.finish())))
        assert out[0] == out[1] and out[0][0] > 8 and out[0][1] > 1 and out[0][4] == 0
    finally:
        eng.close()


@pytest.mark.parametrize("name", ("four_images", "two_rounds", "capacity_merges"))
def test_batches(infl, name):
    """two batches, 8 spans a batch, a batch a span -- and the batch size at which the first image's span OPENS a batch, so that
    the false start is the first start of the next batch"""
    raw, text, bits, span = case(name)[:4]
    nspans = (len(raw) + span - 1) // span
    opens = bits[0] // (8 * span)
    assert 1 < opens < nspans and (8 * span * opens) == bits[0]
    for batch in ((nspans + 1) // 2, 8, 1, opens):
        check_repaired(infl, name, batch_spans=batch)


def test_both_flags_are_refused(infl, tmp_path):
    raw, text, bits = rm.missed_stream()
    with pytest.raises(capi.MkError) as ei:
        infl.stream(gz(raw, text), span_bytes=SPAN, members=True, repair=True)
    assert ei.value.code == capi.MK_ERR_ARG and "MK_GUNZIP_REPAIR" in str(ei.value)
    assert infl.stream(gz(raw, text), span_bytes=SPAN, repair=True)[1] == 0  # the handle goes on


# ---- the engines ----------------------------------------------------------------------------------------------------------------------
def result_key(res):
    return [(ids.tobytes(), None if cnt is None else np.asarray(cnt).tobytes()) for ids, cnt in res]


ENTRIES = {"push_gzip": (lambda e: e.begin(capi.MK_MODE_KOC), lambda e, p, **kw: e.push_gzip(p, span_bytes=SPAN, ratio=RATIO, **kw)),
           "push_gzip_q": (lambda e: e.begin_occ(2), lambda e, p, **kw: e.push_gzip(p, span_bytes=SPAN, ratio=RATIO, qmin=53, **kw)),
           "push_gzip_long": (lambda e: e.begin(capi.MK_MODE_KOC), lambda e, p, **kw: e.push_gzip_long(p, span_bytes=SPAN, ratio=RATIO, **kw)),
           "push_gzip_long_q": (lambda e: e.begin_occ(2), lambda e, p, **kw: e.push_gzip_long_q(p, 53, span_bytes=SPAN, ratio=RATIO, **kw))}


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(capi.Shuf.generate(*gc.SHUF_SPECS["L1K7"]), 0)
    yield e
    e.close()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_engine_entries(eng, tmp_path, entry):
    """the sketch of the repaired stream is the sketch of the same text compressed without images, pushed through the same entry
    without the flag.  R is 1040 throughout: with the default R = 16 the piece in front of the stored block meets its capacity at
    the block's header before it can pass the false start (the capacity rule, which test_repair_... covers with R = 4)"""
    begin, push = ENTRIES[entry]
    raw, text, bits = rm.four_images()
    planted, plain = str(tmp_path / "planted.fq.gz"), str(tmp_path / "plain.fq.gz")
    open(planted, "wb").write(gz(raw, text))
    open(plain, "wb").write(gz(rm.plain(text), text))
    begin(eng)
    st0 = push(eng, plain)
    assert eng.gunzip_repairs() == 0
    want = eng.finish()
    assert sum(len(ids) for ids, _ in want) > 0 and st0.text_bytes == len(text)
    begin(eng)
    with pytest.raises(capi.MkError) as ei:  # without the flag: as ever
        push(eng, planted)
    assert ei.value.code == capi.MK_ERR_FORMAT and ei.value.stats.bad_status == capi.MK_INFL_MISSED and eng.gunzip_repairs() == 0
    eng.finish()  # what was pushed is dropped
    for batch in (0, 8):
        begin(eng)
        st = push(eng, planted, repair=True, batch_spans=batch)
        assert eng.gunzip_repairs() == 4 and st.bad_status == 0 and st.text_bytes == len(text) and st.rows == st0.rows
        assert st.pieces == len(case("four_images")[6][2])
        assert result_key(eng.finish()) == result_key(want), (entry, batch)
    begin(eng)
    with pytest.raises(capi.MkError) as ei:
        push(eng, planted, repair=True, members=True)
    assert ei.value.code == capi.MK_ERR_ARG
    eng.finish()


# ---- the command line -----------------------------------------------------------------------------------------------------------------
ROUTES = {"device-gunzip": (["-A", "--device-gunzip"], "route"), "long-inflate": (["-A", "--long-inflate"], "source"),
          "long-inflate-q": (["-n", "2", "-Q", "53", "--long-inflate-q"], "source")}


def run_cli(shuf, flags, out, inp):
    r = subprocess.run([CLI, "dist", "-L", shuf] + flags + ["--gunzip-span-bytes", "1024", "--gunzip-ratio", str(RATIO), "-p", "4", "--quiet", "--timing", "-o", out, inp],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-600:]
    return [json.loads(ln) for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith('{"input"')]


def same_sketch(a, b):
    fa = sorted(f for f in os.listdir(a) if f.startswith("combco"))
    assert fa and fa == sorted(f for f in os.listdir(b) if f.startswith("combco"))
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_cli(route, tmp_path):
    """the input's name is the same in every run (a directory each), so the directories compare byte for byte, cofiles.stat included"""
    flags, key = ROUTES[route]
    shuf = str(tmp_path / "L1K7.shuf")
    gc.make_shuf("L1K7", shuf)
    raw, text, bits = rm.four_images()
    os.mkdir(str(tmp_path / "planted")), os.mkdir(str(tmp_path / "plain"))
    planted, plain = str(tmp_path / "planted" / "reads.fq.gz"), str(tmp_path / "plain" / "reads.fq.gz")
    open(planted, "wb").write(gz(raw, text, b"reads.fq"))
    open(plain, "wb").write(gz(rm.plain(text), text, b"reads.fq"))
    want, got, fell = str(tmp_path / "want"), str(tmp_path / "got"), str(tmp_path / "fell")
    routes = run_cli(shuf, flags, want, plain)
    assert [x[key] for x in routes] == ["device-gunzip"] and "repairs" not in routes[0] and "fallback" not in routes[0]
    routes = run_cli(shuf, flags + ["--gunzip-repair"], got, planted)
    assert [x[key] for x in routes] == ["device-gunzip"], "the device route was not taken"
    assert routes[0]["repairs"] == 4 and routes[0]["text_bytes"] == len(text) and routes[0]["pieces"] == len(case("four_images")[6][2])
    same_sketch(want, got)
    routes = run_cli(shuf, flags + ["--gunzip-repair"], str(tmp_path / "clean"), plain)  # a clean file under the switch
    assert [x[key] for x in routes] == ["device-gunzip"] and routes[0]["repairs"] == 0
    same_sketch(want, str(tmp_path / "clean"))
    routes = run_cli(shuf, flags, fell, planted)  # without the switch: the fall-back, loudly, and zcat's text gives the same sketch
    assert [(x[key], x.get("fallback")) for x in routes] == [("zcat", capi.lib.mk_gunzip_status_text(capi.MK_INFL_MISSED).decode())]
    same_sketch(want, fell)


def test_cli_refuses_both_switches(tmp_path):
    r = subprocess.run([CLI, "dist", "-L", "none.shuf", "-A", "--device-gunzip", "--gunzip-members", "--gunzip-repair", "-o", str(tmp_path / "o"), "x.fq.gz"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"--gunzip-repair does not go with --gunzip-members" in r.stderr
