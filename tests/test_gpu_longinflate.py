"""`dist -A --long-inflate` on the GPU: FASTQ text that is in HBM already -- pushed by the caller
(mk_sketch_push_fastq_long_device) or inflated there from gzip (mk_sketch_push_gzip_long) and BGZF (mk_sketch_push_bgzf_long) -- through
the long-read framing, the open record carried in HBM by mk_fql_carry_kernel.

Expected sketches need no new model: the texts are tests/longreads_cases.py's and the `lengths` / `dirty` sketches are compared bit
for bit with what the compiled reference wrote (tests/golden/longreads); small texts made here go through the oracle's own FASTQ
reader (reads under 4 095 characters) or its per-read loop on one wide row per read."""
import filecmp
import json
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_util as bu
import composite_model as cm
import dev_rows as dr
import golden_cases as gc
import gunzip_model as gm
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
GEOMS = ["L3K11", "L1K7", "L0K6"]
RATIO = 1040  # no deflate stream gives more than 1032 bytes a compressed byte: the 70 001 'I' of a quality line fit any piece's capacity


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


@pytest.fixture(scope="module")
def dev(capi):
    """text -> its address in device memory, uploaded once: 16 bytes of 0xEE, the text, 32 bytes of 0xEE"""
    hip = dr.hip_lib()
    made, bufs = {}, []

    def get(text):
        if text not in made:
            b = np.frombuffer(b"\xee" * 16 + text + b"\xee" * 32, dtype=np.uint8)
            p = dr.dev_alloc(hip, b.size)
            bufs.append(p)
            assert hip.hipMemcpy(p, b.ctypes.data, b.size, dr.H2D) == 0
            made[text] = p.value + 16
        return made[text]
    get.hip = hip
    yield get
    for p in bufs:
        hip.hipFree(p)


def frozen(w):
    for ids, counts in w:
        ids.setflags(write=False)
        counts.setflags(write=False)
    return w


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def keys(w):
    return sum(len(x[0]) for x in w)


def assert_same(got, want, label=""):
    assert len(got) == len(want), label
    for c, ((gi, gc_), (wi, wc)) in enumerate(zip(got, want)):
        assert len(gi) == len(wi), "%s component %d: %d ids vs oracle %d" % (label, c, len(gi), len(wi))
        assert np.array_equal(gi, wi), "%s component %d: id order/content differs" % (label, c)
        assert gc_ is not None and np.array_equal(gc_, wc), "%s component %d: counts differ" % (label, c)


def assert_is_fixture(got, case):
    assert keys(got) == MANIFEST["cases"][case]["keys"] >= lc.MIN_KEYS[case]
    for c, (ids, cnt) in enumerate(got):
        assert np.asarray(ids, dtype="<u4").tobytes() == open(os.path.join(GOLD, case, "combco.%d" % c), "rb").read(), (case, c)
        assert np.asarray(cnt, dtype="<u2").tobytes() == open(os.path.join(GOLD, case, "combco.%d.a.u16" % c), "rb").read(), (case, c)


def push_device(eng, ptr, n, piece=None, final=True):
    """n bytes at ptr in pieces of `piece` bytes, the last one final"""
    piece = piece or max(n, 1)
    at = 0
    while True:
        m = min(piece, n - at)
        last = at + m >= n
        eng.push_fastq_long_device(ptr + at, m, final=last and final)
        at += m
        if last:
            return


# ---- 1. the device entry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["whole", "63", "1023", "1024", "1025", "4099", "oversize"])
@pytest.mark.parametrize("geom", GEOMS)
def test_device_lengths(capi, engine_for, dev, geom, mode):
    """reads of 0 .. 70 001 bases from device memory: whole, in pieces that cut every kind of line anywhere (the 70 001-base record
    grows the carry over 30 and more pushes of 4 099 bytes, over 2 000 of 63), and with a piece longer than the text"""
    case = "lengths_" + geom
    text, eng = lc.fastq(case), engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), len(text), None if mode == "whole" else len(text) + 1000 if mode == "oversize" else int(mode))
    assert_is_fixture(eng.finish(), case)


@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_device_pointer_alignments(capi, engine_for, dev, geom):
    """the text at each of 16 consecutive byte alignments, pushed whole and in pieces of 4 099 bytes (every piece at another one)"""
    case = "lengths_" + geom
    text, eng, hip = lc.fastq(case), engine_for(geom), dev.hip
    b = np.frombuffer(text, dtype=np.uint8)
    buf = dr.dev_alloc(hip, len(text) + 64)
    try:
        for k in range(16):
            assert hip.hipMemset(buf, 0xEE, len(text) + 64) == 0
            assert hip.hipMemcpy(buf.value + k, b.ctypes.data, b.size, dr.H2D) == 0
            eng.begin(capi.MK_MODE_KOC)
            push_device(eng, buf.value + k, len(text), 4099 if k % 2 else None)
            assert_is_fixture(eng.finish(), case)  # (the finish waits: the buffer may be rewritten)
    finally:
        hip.hipFree(buf)


@pytest.mark.parametrize("piece", [None, 1025, 61])
@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_device_dirty_text(capi, engine_for, dev, geom, piece):
    case = "dirty_" + geom
    text, eng = lc.fastq(case), engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), len(text), piece)
    assert_is_fixture(eng.finish(), case)


def small_text():
    """four records in under 2 KB: the second straddles the first 1 024-byte segment bound, the last is the same 70 bases twice"""
    a = ui.rand_seq(np.random.RandomState(31), 900)
    seqs = [a[:480], a[440:500], a[100:400], a[40:110] + a[40:110]]
    text = ui.fastq_bytes(seqs)
    last = len(ui.fastq_bytes(seqs[:3]))
    first = len(ui.fastq_bytes(seqs[:1]))
    assert len(text) <= 2048 and first < 1024 < len(ui.fastq_bytes(seqs[:2])) and last < len(text)
    return seqs, text, last


@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_device_byte_by_byte(capi, engine_for, oracles, dev, geom):
    seqs, text, _ = small_text()
    rc, want = oracles(geom).koc_from_fastq(text)
    assert rc == 0 and keys(want) >= {"L1K7": 20, "L0K6": 500}[geom] and max(int(w[1].max()) for w in want if len(w[1])) > 1
    eng = engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), len(text), 1)
    assert_same(eng.finish(), want, "byte by byte")


@pytest.mark.parametrize("geom", ["L1K7"])
def test_device_truncated_at_every_byte_of_the_last_record(capi, engine_for, oracles, dev, geom):
    """the record counts only when its fourth line has a byte (iseq2comem.c:673): whole, and in two pieces cut inside that record"""
    seqs, text, start = small_text()
    ora, eng = oracles(geom), engine_for(geom)
    rc, full = ora.koc_from_fastq(text)
    rc2, three = ora.koc_from_fastq(text[:start])
    assert rc == 0 and rc2 == 0 and not same(full, three)
    with_last = 0
    for n in range(start, len(text) + 1):
        rc, want = ora.koc_from_fastq(text[:n])
        assert rc == 0 and (same(want, full) or same(want, three))
        with_last += same(want, full)
        for cut in (None, start + (n - start) // 2):
            eng.begin(capi.MK_MODE_KOC)
            if cut is None or cut in (0, n):
                push_device(eng, dev(text), n)
            else:
                eng.push_fastq_long_device(dev(text), cut, final=False)
                eng.push_fastq_long_device(dev(text) + cut, n - cut, final=True)
            assert_same(eng.finish(), want, "cut at %d of %d, first piece %s" % (n, len(text), cut))
    assert with_last == len(seqs[3]) + 1  # from the first quality byte on, with or without the final '\n'


@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_host_and_device_pushes_alternate(capi, engine_for, dev, geom):
    """one representation of the open record: pieces of 1 025 bytes come from the host and from the device in turn"""
    case = "lengths_" + geom
    text, eng = lc.fastq(case), engine_for(geom)
    b = np.frombuffer(text, dtype=np.uint8)
    eng.begin(capi.MK_MODE_KOC)
    for i, at in enumerate(range(0, len(text), 1025)):
        n, last = min(1025, len(text) - at), at + 1025 >= len(text)
        if i % 2:
            eng.push_fastq_long_device(dev(text) + at, n, final=last)
        else:
            part = np.ascontiguousarray(b[at:at + n])
            capi._check(capi.lib.mk_sketch_push_fastq_long(eng.h, part.ctypes.data, n, 1 if last else 0), eng.h)
    assert_is_fixture(eng.finish(), case)


def big_record_at(text, case):
    """where the sequence line of the 70 001-base record starts in the case's text"""
    big = [s for s in lc.reads(case) if len(s) == 70001][0]
    return text.index(b"\n" + big + b"\n") + 1


def overlap_text(geom):
    """a first record of 200 bytes, then the 70 001-base record: from the third piece of 4 099 bytes on the carry is longer than
    everything consumed so far, so a move to the front of the same buffer would overlap its source"""
    big = [s for s in lc.reads("lengths_" + geom) if len(s) == 70001][0]
    small = ui.rand_seq(np.random.RandomState(5), 95)
    text = b"@s hh\n" + small + b"\n+\n" + b"I" * 95 + b"\n" + b"@big\n" + big + b"\n+\n" + b"I" * len(big) + b"\n"
    assert text.index(b"@big") == 200
    return [small, big], text


@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_carry_longer_than_what_was_consumed(capi, engine_for, oracles, dev, geom):
    seqs, text = overlap_text(geom)
    rows, stride = lc.rows_of(seqs)
    rc, want = oracles(geom).koc_from_rows(rows, stride)
    assert rc == 0 and keys(want) >= {"L1K7": 3000, "L0K6": 12000}[geom]
    rc, cut = oracles(geom).koc_from_rows(*lc.rows_of([s[:lc.FQ_MAX] for s in seqs]))
    assert rc == 0 and not same(want, cut)
    eng = engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), len(text), 4099)
    assert_same(eng.finish(), frozen(want), "device pieces")
    eng.begin(capi.MK_MODE_KOC)
    eng.push_fastq_long(text, piece=4099)
    assert_same(eng.finish(), want, "host pieces")


@pytest.mark.parametrize("geom", ["L1K7"])
def test_two_sketches_in_a_row(capi, engine_for, oracles, dev, geom):
    """the second text is shorter than the carry the first one left: closed by its final push, and left open (no final: finished,
    dropped, begun anew -- the rule after a failed push)"""
    case = "lengths_" + geom
    text, eng = lc.fastq(case), engine_for(geom)
    _, small, _ = small_text()
    rc, want = oracles(geom).koc_from_fastq(small)
    assert rc == 0
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), len(text), 4099)
    assert_is_fixture(eng.finish(), case)
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(small), len(small), 63)
    assert_same(eng.finish(), want, "behind a closed sketch")
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), big_record_at(text, case) + 30000, 4099, final=False)  # ends inside the 70 001-base record's sequence line
    dropped = eng.finish()
    assert keys(dropped) < MANIFEST["cases"][case]["keys"]
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(small), len(small), 63)
    assert_same(eng.finish(), want, "behind an abandoned sketch")
    eng.begin(capi.MK_MODE_KOC)
    push_device(eng, dev(text), len(text), 1025)
    assert_is_fixture(eng.finish(), case)


def test_device_entry_state_errors(capi, engine_for, dev):
    eng = engine_for("L1K7")
    rec = b"@r\nACGT\n+\nIIII\n"
    eng.begin(capi.MK_MODE_SET)
    with pytest.raises(capi.MkError) as ei:
        eng.push_fastq_long_device(dev(rec), len(rec))
    assert ei.value.code == capi.MK_ERR_STATE and "MK_MODE_KOC" in str(ei.value)
    eng.finish()
    eng.begin(capi.MK_MODE_KOC)
    host = np.frombuffer(rec, dtype=np.uint8)
    with pytest.raises(capi.MkError) as ei:  # a host pointer is refused, not copied as if it were the device's
        eng.push_fastq_long_device(host.ctypes.data, len(rec))
    assert ei.value.code == capi.MK_ERR_ARG
    eng.push_fastq_long_device(dev(rec), len(rec))
    with pytest.raises(capi.MkError) as ei:
        eng.push_fastq_long_device(dev(rec), len(rec))
    assert ei.value.code == capi.MK_ERR_STATE and "final" in str(ei.value)
    eng.finish()
    eng.begin(capi.MK_MODE_KOC)
    eng.push_stream(b">g\nACGTACGTACGTACGTACGT\n", final=False)
    with pytest.raises(capi.MkError) as ei:
        eng.push_fastq_long_device(dev(rec), len(rec))
    assert ei.value.code == capi.MK_ERR_STATE
    eng.push_stream(b"", final=True)
    eng.finish()


# ---- 2. the gzip route, ABI ---------------------------------------------------------------------------------------------------------
def gz(raw, text, crc=None):
    """one gzip member around a raw deflate stream"""
    return bytes([0x1f, 0x8b, 8, 0]) + b"\0\0\0\0\x00\x03" + raw + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) & 0xffffffff)


def write(tmp_path, name, data):
    p = str(tmp_path / name)
    open(p, "wb").write(data)
    return p


SMALL = dict(span_bytes=1024, ratio=RATIO, batch_spans=8)  # the 140 KB record crosses many batches and is 8 times MK_FQ_CARRY


@pytest.mark.parametrize("level,mem", [(1, 1), (6, 1), (9, 2)])  # (small memLevels: many deflate blocks, so many piece starts)
@pytest.mark.parametrize("case", ["lengths_L3K11", "lengths_L1K7", "dirty_L0K6"])
def test_gzip_cases(capi, engine_for, tmp_path, case, level, mem):
    text, eng = lc.fastq(case), engine_for(lc.CASES[case][1])
    raw = gm.deflate(text, level, mem)
    path = write(tmp_path, "a.fq.gz", gz(raw, text))
    for geometry in (SMALL, {}):
        eng.begin(capi.MK_MODE_KOC)
        st = eng.push_gzip_long(path, **geometry)
        assert_is_fixture(eng.finish(), case)
        assert st.text_bytes == len(text) and st.rows == 0 and st.bad_status == 0 and st.frame_ms > 0
        if geometry:  # 8 KiB of compressed bytes a batch: 11 to 44 KB of them here
            assert st.batches >= 2 and st.pieces > st.batches


@pytest.mark.parametrize("every", [600, 50000])
def test_gzip_member_concatenation(capi, engine_for, tmp_path, every):
    case = "lengths_L1K7"
    text, eng = lc.fastq(case), engine_for("L1K7")
    parts = [text[a:a + every] for a in range(0, len(text), every)]
    path = write(tmp_path, "cat.fq.gz", b"".join(gz(gm.deflate(p, 6, 9), p) for p in parts))
    eng.begin(capi.MK_MODE_KOC)
    st = eng.push_gzip_long(path, members=True, **SMALL)
    assert_is_fixture(eng.finish(), case)
    assert st.members == len(parts) and st.text_bytes == len(text)
    eng.begin(capi.MK_MODE_KOC)
    with pytest.raises(capi.MkError) as ei:  # without the flag the decode says so
        eng.push_gzip_long(path, **SMALL)
    assert ei.value.code == capi.MK_ERR_FORMAT and ei.value.stats.bad_status == capi.MK_INFL_TRAILING
    assert capi.lib.mk_gunzip_status_text(capi.MK_INFL_TRAILING).decode() in str(ei.value)
    eng.finish()


def test_gzip_incomplete_last_record(capi, engine_for, oracles, tmp_path):
    seqs, text, start = small_text()
    ora, eng = oracles("L1K7"), engine_for("L1K7")
    head = text.index(b"\n", start) + 1
    plus = text.index(b"+\n", start) + 2
    cuts = {"behind the header": head, "inside the sequence": head + 50, "behind +": plus, "quality line without its end": len(text) - 1}
    rc, full = ora.koc_from_fastq(text)
    rc2, three = ora.koc_from_fastq(text[:start])
    assert rc == 0 and rc2 == 0 and not same(full, three)
    for name, n in cuts.items():
        rc, want = ora.koc_from_fastq(text[:n])
        assert rc == 0 and same(want, full if name == "quality line without its end" else three), name
        path = write(tmp_path, "cut.fq.gz", gz(gm.deflate(text[:n], 6, 9), text[:n]))
        for geometry in (dict(span_bytes=64, ratio=RATIO, batch_spans=2), {}):
            eng.begin(capi.MK_MODE_KOC)
            eng.push_gzip_long(path, **geometry)
            assert_same(eng.finish(), want, name)


def test_gzip_of_an_empty_text(capi, engine_for, tmp_path):
    """mk_gzip_scan_stream accepts it (ISIZE says nothing there), so this route takes it: one piece, no text, a closed empty sketch"""
    eng = engine_for("L1K7")
    path = write(tmp_path, "empty.fq.gz", gz(gm.deflate(b""), b""))
    eng.begin(capi.MK_MODE_KOC)
    st = eng.push_gzip_long(path)
    assert st.text_bytes == 0 and st.pieces == 1 and st.bad_status == 0
    with pytest.raises(capi.MkError) as ei:  # the stream was closed
        eng.push_fastq_long(b"@r\nACGT\n+\nIIII\n")
    assert ei.value.code == capi.MK_ERR_STATE
    assert keys(eng.finish()) == 0


@pytest.mark.parametrize("route", ["gzip", "bgzf"])
def test_two_files_into_one_sketch(capi, engine_for, tmp_path, route):
    """final=0 then final=1: the record the first file leaves open continues in the second, as in `zcat a b`"""
    case = "lengths_L1K7"
    text, eng = lc.fastq(case), engine_for("L1K7")
    cut = big_record_at(text, case) + 30000  # inside the 70 001-base record's sequence line
    assert text[:cut].count(b"\n") % 4 == 1
    paths = []
    for k, part in enumerate((text[:cut], text[cut:])):
        data = gz(gm.deflate(part, 6, 9), part) if route == "gzip" else bu.write_bgzf(part, payload=4096)[0]
        paths.append(write(tmp_path, "part%d.fq.gz" % k, data))
    eng.begin(capi.MK_MODE_KOC)
    if route == "gzip":
        eng.push_gzip_long(paths[0], final=False, **SMALL)
        eng.push_gzip_long(paths[1], final=True, **SMALL)
    else:
        eng.push_bgzf_long(paths[0], chunk_bytes=65536, final=False)
        eng.push_bgzf_long(paths[1], chunk_bytes=65536, final=True)
    assert_is_fixture(eng.finish(), case)


def test_gzip_crc_trailer_flipped(capi, engine_for, tmp_path):
    case = "lengths_L1K7"
    text, eng = lc.fastq(case), engine_for("L1K7")
    good = gz(gm.deflate(text, 6, 9), text)
    bad = bytearray(good)
    bad[len(bad) - 7] ^= 0x10  # a byte of the CRC32 field, never of the payload
    path = write(tmp_path, "crc.fq.gz", bytes(bad))
    for geometry in (SMALL, {}):
        eng.begin(capi.MK_MODE_KOC)
        with pytest.raises(capi.MkError) as ei:
            eng.push_gzip_long(path, **geometry)
        assert ei.value.code == capi.MK_ERR_FORMAT and ei.value.stats.bad_status == capi.MK_INFL_CRC and ei.value.stats.text_bytes == len(text)
        eng.finish()  # what was pushed is finished and dropped ...
        eng.begin(capi.MK_MODE_KOC)  # ... and the next sketch is exact
        eng.push_fastq_long(text, piece=4099)
        assert_is_fixture(eng.finish(), case)


# ---- 3. the BGZF route, ABI ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("payload", [65280, 4096])
@pytest.mark.parametrize("case", ["lengths_L3K11", "lengths_L1K7", "dirty_L0K6"])
def test_bgzf_cases(capi, engine_for, tmp_path, case, payload):
    text, eng = lc.fastq(case), engine_for(lc.CASES[case][1])
    data, table = bu.write_bgzf(text, payload=payload)
    path = write(tmp_path, "a.fq.gz", data)
    for chunk in (65536, 0):  # one member a chunk at payload 65 280: the 140 KB record crosses three chunks
        eng.begin(capi.MK_MODE_KOC)
        st = eng.push_bgzf_long(path, chunk_bytes=chunk)
        assert_is_fixture(eng.finish(), case)
        assert st.text_bytes == len(text) and st.rows == 0 and st.blocks == len(table) and st.bad_block == -1 and st.frame_ms > 0
        # 64 KiB chunks: sixteen members of 4 096 bytes, or one of 65 280; the empty end marker joins the last chunk
        assert st.chunks == ((len(text) + 65535) // 65536 if chunk and payload == 4096 else len(table) - 1 if chunk else 1)


def test_bgzf_incomplete_last_record_and_empty_text(capi, engine_for, oracles, tmp_path):
    seqs, text, start = small_text()
    ora, eng = oracles("L1K7"), engine_for("L1K7")
    head = text.index(b"\n", start) + 1
    for n in (head, head + 50, text.index(b"+\n", start) + 2, len(text) - 1, 0):
        rc, want = ora.koc_from_fastq(text[:n])
        assert rc == 0
        path = write(tmp_path, "cut.fq.gz", bu.write_bgzf(text[:n], payload=512)[0])
        eng.begin(capi.MK_MODE_KOC)
        st = eng.push_bgzf_long(path, chunk_bytes=65536)
        assert st.text_bytes == n
        assert_same(eng.finish(), want, "cut at %d" % n)


@pytest.mark.parametrize("block", [0, 2, 3])
def test_bgzf_block_crc_flipped(capi, engine_for, tmp_path, block):
    case = "lengths_L1K7"
    text, eng = lc.fastq(case), engine_for("L1K7")
    data, table = bu.write_bgzf(text, payload=65280)
    assert len(table) == 5  # four members of text and the end marker: 65 536-byte chunks hold one each
    bad = bytearray(data)
    bad[table[block]["in_off"] + table[block]["in_len"] - 7] ^= 0x10  # a byte of the member's CRC32 field
    path = write(tmp_path, "crc.fq.gz", bytes(bad))
    for chunk in (65536, 0):
        eng.begin(capi.MK_MODE_KOC)
        with pytest.raises(capi.MkError) as ei:
            eng.push_bgzf_long(path, chunk_bytes=chunk)
        assert ei.value.code == capi.MK_ERR_FORMAT and ei.value.stats.bad_block == block and ei.value.stats.bad_status == capi.MK_INFL_CRC
        eng.finish()
        eng.begin(capi.MK_MODE_KOC)
        eng.push_bgzf_long(write(tmp_path, "good.fq.gz", data), chunk_bytes=chunk)
        assert_is_fixture(eng.finish(), case)


# ---- 4. poison ----------------------------------------------------------------------------------------------------------------------
ABI_TESTS = ("test_device_ or test_host_and_device or test_carry_longer or test_two_sketches or test_gzip_ or test_two_files or test_bgzf_")


@pytest.mark.parametrize("byte", ["0xA5", "0x43"])
def test_abi_tests_under_poison(byte):
    """MK_POISON fills every allocation of the library before use (read once per process: a process of its own): the ABI tests again --
    a kernel that read what nobody wrote (the carry buffer behind the open record, the text buffer's slack) would not match"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", ABI_TESTS],
                       env=dict(os.environ, MK_POISON=byte), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    m = re.search(r"(\d+) passed", out)
    assert r.returncode == 0 and m and int(m.group(1)) == 64 and "skipped" not in out and "16 deselected" in out, out[-3000:]


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------
def run_cli(args, env=None, ok=True):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    if ok:
        assert r.returncode == 0, (args, r.stderr.decode(errors="replace")[-500:])
    routes = [json.loads(ln) for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith('{"input"')]
    return r, routes


@pytest.fixture(scope="module")
def lr_shufs(tmp_path_factory):
    d = tmp_path_factory.mktemp("longinflate_shufs")
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
    for c in range(stat["comp_num"]):
        assert open(os.path.join(out, "combco.%d" % c), "rb").read() == b"".join(open(os.path.join(GOLD, x, "combco.%d" % c), "rb").read() for x in cases)
        assert open(os.path.join(out, "combco.%d.a" % c), "rb").read() == b"".join(open(os.path.join(GOLD, x, "combco.%d.a.u16" % c), "rb").read() for x in cases)


def same_sketch_files(a, b):
    """the component files byte for byte (cofiles.stat holds the input's name)"""
    fa = sorted(f for f in os.listdir(a) if f.startswith("combco"))
    assert fa and fa == sorted(f for f in os.listdir(b) if f.startswith("combco"))
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def compressed(kind, text):
    return {"gzip": lambda: gz(gm.deflate(text, 6, 1), text), "bgzf": lambda: bu.write_bgzf(text, payload=65280)[0]}[kind]()


SOURCE = {"gzip": "device-gunzip", "bgzf": "device-inflate", "plain": "file"}
HOOKS = {"gzip": ["--gunzip-span-bytes", "1024", "--gunzip-ratio", str(RATIO), "--gunzip-batch-spans", "8"], "bgzf": ["--inflate-chunk-kib", "64"], "plain": []}


@pytest.mark.parametrize("kind", ["gzip", "bgzf", "plain"])
@pytest.mark.parametrize("case", ["lengths_L3K11", "lengths_L1K7", "dirty_L0K6"])
def test_cli_long_inflate(case, kind, lr_shufs, tmp_path):
    geom, text = lc.CASES[case][1], lc.fastq(case)
    plain = write(tmp_path, case + ".fq", text)
    inp = plain if kind == "plain" else write(tmp_path, case + ".fq.gz", compressed(kind, text))
    base = str(tmp_path / "long_reads_plain")
    run_cli(DIST + ["-L", lr_shufs(geom), "-A", "--long-reads", "-o", base, plain])
    for k, hooks in enumerate(([], HOOKS[kind])):
        out = str(tmp_path / ("out%d" % k))
        r, routes = run_cli(DIST + ["-L", lr_shufs(geom), "-A", "--long-inflate", "--timing", "-o", out] + hooks + [inp])
        check_dir(out, [case], [inp])
        same_sketch_files(out, base)
        assert len(routes) == 1 and routes[0]["route"] == "long-reads" and routes[0]["source"] == SOURCE[kind], "the device route was not taken"
        assert routes[0]["text_bytes"] == len(text) and "fallback" not in routes[0]
        if kind == "gzip":
            assert routes[0]["batches"] >= (2 if hooks else 1) and routes[0]["pieces"] >= routes[0]["batches"]
        if kind == "bgzf":
            assert routes[0]["chunks"] == (routes[0]["blocks"] - 1 if hooks else 1)  # (the empty end marker joins the last chunk)
    if kind != "plain":  # --no-device-inflate: today's route under the new switch too
        out = str(tmp_path / "zcat")
        r, routes = run_cli(DIST + ["-L", lr_shufs(geom), "-A", "--long-inflate", "--no-device-inflate", "--timing", "-o", out, inp])
        check_dir(out, [case], [inp])
        assert [x["source"] for x in routes] == ["zcat"] and "fallback" not in routes[0]


def test_cli_gunzip_members(lr_shufs, tmp_path):
    case = "lengths_L1K7"
    text = lc.fastq(case)
    parts = [text[a:a + 50000] for a in range(0, len(text), 50000)]
    inp = write(tmp_path, "cat.fq.gz", b"".join(gz(gm.deflate(p, 6, 9), p) for p in parts))
    out = str(tmp_path / "out")
    r, routes = run_cli(DIST + ["-L", lr_shufs("L1K7"), "-A", "--long-inflate", "--gunzip-members", "--timing", "-o", out, inp])
    check_dir(out, [case], [inp])
    assert [(x["source"], x["members"], x["text_bytes"]) for x in routes] == [("device-gunzip", len(parts), len(text))] and "fallback" not in routes[0]
    out = str(tmp_path / "out_noflag")  # without the flag: the status, loudly, and zcat reads the concatenation
    r, routes = run_cli(DIST + ["-L", lr_shufs("L1K7"), "-A", "--long-inflate", "--timing", "-o", out, inp])
    check_dir(out, [case], [inp])
    assert [(x["source"], x.get("fallback")) for x in routes] == [("zcat", capi_status_text("MK_INFL_TRAILING"))]


def capi_status_text(name):
    from metakssd_amd import capi
    return capi.lib.mk_gunzip_status_text(getattr(capi, name)).decode()


def test_cli_two_files_in_one_run(lr_shufs, tmp_path):
    cases = ("lengths_L1K7", "dirty_L1K7")
    inputs = [write(tmp_path, cases[0] + ".fq.gz", compressed("gzip", lc.fastq(cases[0]))), write(tmp_path, cases[1] + ".fq.gz", compressed("bgzf", lc.fastq(cases[1])))]
    out = str(tmp_path / "out")
    r, routes = run_cli(DIST + ["-L", lr_shufs("L1K7"), "-A", "--long-inflate", "--timing", "-o", out] + inputs)
    _, names = tg.parse_stat(os.path.join(out, "cofiles.stat"))
    assert sorted(names) == sorted(inputs)
    check_dir(out, [os.path.basename(n)[:-6] for n in names], names)
    assert sorted((x["input"], x["source"]) for x in routes) == sorted(zip(inputs, ("device-gunzip", "device-inflate")))
    assert all("fallback" not in x for x in routes)


def test_cli_composite_equals_two_steps(shuf_files, tmp_path):
    """`dist -A --long-inflate --composite db` prints what `dist -A --long-inflate -o d` + `composite -q d` print, and what the plain
    files give under --long-reads, for reads of 3 000 to 9 000 bases drawn from two of the marker database's strains"""
    db, _ = cm.build_marker_db("composite_mix_L1K7", shuf_files, tmp_path, DIST, [BIN, "set"])
    rs = np.random.RandomState(12)
    ga, gc_ = b"".join(gc._strain("sA")), b"".join(gc._strain("sC"))
    files, plain = [], []
    for k, (share, kind) in enumerate(((0.8, "gzip"), (0.3, "bgzf"))):
        seqs = []
        for _ in range(60):
            g = ga if rs.rand() < share else gc_
            n = int(rs.randint(3000, 9001))
            a = int(rs.randint(0, len(g) - n))
            seqs.append(ui.revcomp(g[a:a + n]) if rs.rand() < 0.5 else g[a:a + n])
        assert max(len(s) for s in seqs) > lc.FQ_MAX
        text = ui.fastq_bytes(seqs)
        plain.append(write(tmp_path, "long%d.fq" % k, text))
        files.append(write(tmp_path, "long%d.fq.gz" % k, compressed(kind, text)))
    shuf = shuf_files("L1K7")
    d, dp = str(tmp_path / "d"), str(tmp_path / "dp")
    r, routes = run_cli(DIST + ["-L", shuf, "-A", "--long-inflate", "--timing", "-o", d] + files)
    assert sorted(x["source"] for x in routes) == ["device-gunzip", "device-inflate"] and all("fallback" not in x for x in routes)
    run_cli(DIST + ["-L", shuf, "-A", "--long-reads", "-o", dp] + plain)
    same_sketch_files(d, dp)
    want = run_cli([BIN, "composite", "-r", db, "-q", d])[0].stdout
    assert len({ln.split(b"\t")[0] for ln in want.splitlines()}) == 2 and want.count(b"\n") >= 4
    assert run_cli(DIST + ["-L", shuf, "-A", "--long-inflate", "--composite", db] + files)[0].stdout == want


def test_cli_crc_damaged_gzip_falls_back_loudly(lr_shufs, tmp_path):
    """the trailer's CRC32 flipped: the device route reports the status and gives the file to zcat, which alone decides that it is
    damaged -- the ending is the one --long-reads gives this file"""
    text = lc.fastq("lengths_L1K7")
    bad = bytearray(compressed("gzip", text))
    bad[len(bad) - 7] ^= 0x10
    inp = write(tmp_path, "bad.fq.gz", bytes(bad))
    shuf = lr_shufs("L1K7")
    today, _ = run_cli(DIST + ["-L", shuf, "-A", "--long-reads", "--timing", "-o", str(tmp_path / "a"), inp], ok=False)
    r, routes = run_cli(DIST + ["-L", shuf, "-A", "--long-inflate", "--timing", "-o", str(tmp_path / "b"), inp], ok=False)
    assert [(x["source"], x.get("fallback")) for x in routes] == [("zcat", capi_status_text("MK_INFL_CRC"))] and "CRC" in routes[0]["fallback"].upper()
    assert today.returncode != 0 and (r.returncode, r.stderr) == (today.returncode, today.stderr) and b"zcat" in r.stderr
    assert not os.path.exists(os.path.join(str(tmp_path / "b"), "cofiles.stat"))


def test_cli_damaged_bgzf_block(lr_shufs, tmp_path):
    text = lc.fastq("lengths_L1K7")
    data, table = bu.write_bgzf(text, payload=65280)
    bad = bytearray(data)
    bad[table[2]["in_off"] + table[2]["in_len"] - 7] ^= 0x10
    inp = write(tmp_path, "bad.fq.gz", bytes(bad))
    out = str(tmp_path / "out")
    r, _ = run_cli(DIST + ["-L", lr_shufs("L1K7"), "-A", "--long-inflate", "-o", out, inp], ok=False)
    assert r.returncode == 1 and not os.path.exists(os.path.join(out, "cofiles.stat"))
    assert r.stderr.decode().strip().endswith("%s: BGZF block 2 is damaged (%s): the input was not read completely"
                                               % (inp, capi_status_text_infl("MK_INFL_CRC")))


def capi_status_text_infl(name):
    from metakssd_amd import capi
    return capi.lib.mk_inflate_status_text(getattr(capi, name)).decode()
