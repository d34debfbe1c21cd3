"""`dist -n N -Q q --long-reads-q / --long-inflate-q` on the GPU: mk_sketch_push_fastq_long_q[_device] and the two
long sinks with the quality mask -- fastq2co's reader on FASTQ lines of any length, the stream written from the quality lines.

Every comparison is bit-exact, on key lists in dump order: against the directories the real reference wrote from the chopped files
(tests/golden/longreads_q), against the Python model of the rule (tests/longreads_q_cases.py: masked whole reads through the oracle's
per-read loop, keys seen at least M times; pinned on the CPU by tests/test_longreads_q_model.py), and, wherever the host framer
accepts the text, against the host-framer route on the same engine (Engine.push_fastq(occ=True, qmin=...))."""
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
import dev_rows as dr
import gunzip_model as gm
import longreads_cases as lc
import longreads_q_cases as qc
import test_golden as tg
import util_inputs as ui

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "longreads_q")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
BIN = tg.PRODUCT_CLI
DIST = [BIN, "dist", "-p", "4"]
GEOMS = ["L3K11", "L1K7", "L0K6"]
RATIO = 1040
QMINS = [-128, 0, 53, 74]
HOST_MAX = 19998  # characters of a line the host framer takes (mk_fastq_frame_q: fastq2co's fgets() width)


def sub(M, Q):
    return "n%d_Q%d" % (M, Q)


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


def fixture(case, M, Q):
    C = MANIFEST["cases"][case]["runs"][sub(M, Q)]["stat"]["comp_num"]
    return [np.fromfile(os.path.join(GOLD, case, sub(M, Q), "combco.%d" % c), dtype="<u4") for c in range(C)]


def ids_of(result):
    assert all(cnt is None for _, cnt in result)  # a MK_MODE_OCC_SET sketch has no counts
    return [ids for ids, _ in result]


def keys(w):
    return sum(len(x) for x in w)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def assert_same(got, want, label=""):
    assert len(got) == len(want), label
    for c, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), "%s component %d: %d ids, %d wanted" % (label, c, len(g), len(w))
        assert np.array_equal(g, w), "%s component %d: id order/content differs" % (label, c)


def model(ora, text, M, Q):
    """the rule in Python: masked whole reads as wide rows through the reference's per-read loop, keys seen at least M times"""
    rows, stride = lc.rows_of(qc.masked(text, Q))
    rc, koc = ora.koc_from_rows(rows, stride)
    assert rc == 0
    out = [ids[cnt >= M] for ids, cnt in koc]
    for a in out:
        a.setflags(write=False)
    return out


def host_route(eng, text, tl, M, Q):
    """the yardstick: the host framer's rows into the same engine"""
    eng.begin_occ(M)
    eng.push_fastq(text, occ=True, TL=tl, qmin=Q)
    return ids_of(eng.finish())


def long_q(eng, text, M, Q, piece=None):
    eng.begin_occ(M)
    eng.push_fastq_long_q(text, Q, piece=piece)
    return ids_of(eng.finish())


def push_cuts(capi, eng, text, cuts, Q):
    """the text in the pieces that the offsets `cuts` leave, the last one final"""
    b = np.frombuffer(bytes(text), dtype=np.uint8)
    edges = [0] + [c for c in cuts if 0 < c < len(b)] + [len(b)]
    for i in range(len(edges) - 1):
        part = np.ascontiguousarray(b[edges[i]:edges[i + 1]])
        last = i == len(edges) - 2
        capi._check(capi.lib.mk_sketch_push_fastq_long_q(eng.h, part.ctypes.data if len(part) else None, len(part), 1 if last else 0, Q), eng.h)


def push_device(eng, ptr, n, Q, piece=None, final=True):
    piece = piece or max(n, 1)
    at = 0
    while True:
        m = min(piece, n - at)
        last = at + m >= n
        eng.push_fastq_long_q_device(ptr + at, m, Q, final=last and final)
        at += m
        if last:
            return


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------------------
MODES = ["whole", "63", "1023", "1024", "1025", "4099", "oversize"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", GEOMS)
def test_lengths_q(capi, engine_for, geom, mode):
    """reads of 0 .. 70 001 bases whose quality lines mask about one base in a hundred, for -n 1 -Q 0, -n 1 -Q 53 and -n 2 -Q 53: pushed
    whole, in pieces that cut every kind of line anywhere, and with a piece longer than the text"""
    case = "lengths_q_" + geom
    text, eng = qc.fastq(case), engine_for(geom)
    for M, Q in qc.MQ:
        piece = None if mode == "whole" else len(text) + 1000 if mode == "oversize" else int(mode)
        got = long_q(eng, text, M, Q, piece)
        assert keys(got) == MANIFEST["cases"][case]["runs"][sub(M, Q)]["keys"] >= qc.MIN_KEYS[case]
        assert_same(got, fixture(case, M, Q), "%s %s %s" % (case, sub(M, Q), mode))


@pytest.mark.parametrize("mode", ["whole", "1025", "4099"])
@pytest.mark.parametrize("geom", GEOMS)
def test_device_lengths_q(capi, engine_for, dev, geom, mode):
    case = "lengths_q_" + geom
    text, eng = qc.fastq(case), engine_for(geom)
    for M, Q in qc.MQ:
        eng.begin_occ(M)
        push_device(eng, dev(text), len(text), Q, None if mode == "whole" else int(mode))
        assert_same(ids_of(eng.finish()), fixture(case, M, Q), "%s %s %s" % (case, sub(M, Q), mode))


@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_device_pointer_alignments(capi, engine_for, dev, geom):
    """the text at each of 16 consecutive byte alignments, pushed whole and in pieces of 4 099 bytes (every piece at another one)"""
    case = "lengths_q_" + geom
    text, eng, hip = qc.fastq(case), engine_for(geom), dev.hip
    b = np.frombuffer(text, dtype=np.uint8)
    buf = dr.dev_alloc(hip, len(text) + 64)
    try:
        for k in range(16):
            assert hip.hipMemset(buf, 0xEE, len(text) + 64) == 0
            assert hip.hipMemcpy(buf.value + k, b.ctypes.data, b.size, dr.H2D) == 0
            eng.begin_occ(2)
            push_device(eng, buf.value + k, len(text), 53, 4099 if k % 2 else None)
            assert_same(ids_of(eng.finish()), fixture(case, 2, 53), "alignment %d" % k)  # (the finish waits: the buffer may be rewritten)
    finally:
        hip.hipFree(buf)


@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_host_and_device_pushes_alternate(capi, engine_for, dev, geom):
    case = "lengths_q_" + geom
    text, eng = qc.fastq(case), engine_for(geom)
    eng.begin_occ(2)
    at, k = 0, 0
    while at < len(text):
        n = min(4099 + 1000 * (k % 3), len(text) - at)
        last = at + n >= len(text)
        if k % 2:
            eng.push_fastq_long_q_device(dev(text) + at, n, 53, final=last)
        else:
            eng.push_fastq_long_q(text[at:at + n], 53, final=last)
        at += n
        k += 1
    assert_same(ids_of(eng.finish()), fixture(case, 2, 53), case)


# ---- 2. byte by byte ----------------------------------------------------------------------------------------------------------------
def small_text():
    """five records in 2 KiB: the second has a sequence line of 1 100 bytes across a segment bound and a quality line of 440 (the wave
    of its '\\n' finishes 660 columns), the fourth a quality line one short, the last the same 30 bases twice; low qualities in every
    record"""
    a = ui.rand_seq(np.random.RandomState(33), 1400)
    seqs = [a[:60], a[40:1140], a[300:350], a[20:80], a[10:40] + a[10:40]]
    quals = []
    for i, s in enumerate(seqs):
        q = bytearray(b"I" * len(s))
        for j in range(5 + i, len(s), 41):
            q[j] = qc.LOW[(i + j) % len(qc.LOW)]
        quals.append(bytes(q))
    quals[1] = quals[1][:440]
    quals[3] = quals[3][:-1]
    text = b"".join(b"@%d\n" % i + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(zip(seqs, quals)))
    assert len(text) <= 2048 and len(seqs[1]) == 1100
    return text


@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_byte_by_byte(capi, engine_for, oracles, geom):
    text, eng, ora = small_text(), engine_for(geom), oracles(geom)
    for M, Q in [(1, 53), (2, 53), (1, 11)]:  # (at qmin 11 the '\n' of the short quality line masks its column)
        want = model(ora, text, M, Q)
        assert keys(want) >= ({"L1K7": 20, "L0K6": 300}[geom] if M == 1 else 1) and not same(want, model(ora, text, M, -128))
        assert_same(host_route(eng, text, lc.TL(geom), M, Q), want, "host framer")
        eng.begin_occ(M)
        push_cuts(capi, eng, text, list(range(1, len(text))), Q)
        assert_same(ids_of(eng.finish()), want, "%s byte by byte" % sub(M, Q))


# ---- 3. the host framer as yardstick ------------------------------------------------------------------------------------------------
def framer_text(case):
    """the case's records whose lines the host framer takes"""
    if qc.CASES[case][0] == "dirty_q":
        return qc.fastq(case)
    return b"".join(b"@r%d\n" % i + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(zip(qc.reads(case), qc.quals(case))) if len(s) <= HOST_MAX)


@pytest.mark.parametrize("qmin", QMINS)
@pytest.mark.parametrize("case", ["dirty_q_L1K7", "dirty_q_L0K6", "lengths_q_L1K7", "lengths_q_L0K6", "lengths_q_L3K11"])
def test_equals_the_host_framer_route(capi, engine_for, oracles, case, qmin):
    """short, empty and over-long quality lines, CRLF ends, '@' and '>' inside quality lines; reads of up to 8 193 bases that the host
    framer cuts into windows -- the same engine, both routes"""
    geom = qc.CASES[case][1]
    text, eng = framer_text(case), engine_for(geom)
    assert max(len(ln) for ln in text.split(b"\n")) <= HOST_MAX
    for M in (1, 2):
        want = host_route(eng, text, lc.TL(geom), M, qmin)
        assert_same(want, model(oracles(geom), text, M, qmin), "host framer against the model")
        assert (keys(want) > 0) == (qmin < 74)  # ('I' is 73: at 74 every window is masked)
        for piece in (None, 1025):
            assert_same(long_q(eng, text, M, qmin, piece), want, "%s -n %d -Q %d piece=%s" % (case, M, qmin, piece))


# ---- 4. the record rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pieces", ["whole", "two"])
def test_record_rule_at_every_byte_of_the_last_record(capi, engine_for, oracles, pieces):
    """the lengths file truncated at every byte of its last record: that record counts only with its final '\\n'"""
    geom, case = "L1K7", "lengths_q_L1K7"
    text, eng, ora = qc.fastq(case), engine_for(geom), oracles(geom)
    start = text.rindex(b"\n@r67 ") + 1
    full, less = model(ora, text, 1, 53), model(ora, text[:start], 1, 53)
    # the last record's k-mers occur elsewhere in the file (the reads overlap in the pool): -n 2 shows the record, -n 1 does not
    full2, less2 = model(ora, text, 2, 53), model(ora, text[:start], 2, 53)
    assert same(full2, fixture(case, 2, 53)) and not same(full2, less2)
    # one byte short of the end -A's rule takes the record, this one does not
    assert len(lc.records(text[:-1])) == 68 and len(qc.masked(text[:-1], 53)) == 67
    for n in range(start, len(text) + 1):
        want = full2 if n == len(text) else less2
        eng.begin_occ(2)
        if pieces == "whole":
            eng.push_fastq_long_q(text[:n], 53)
        else:
            push_cuts(capi, eng, text[:n], [start + (n - start) // 2], 53)
        assert_same(ids_of(eng.finish()), want, "cut at %d of %d" % (n, len(text)))
    assert keys(full) >= keys(less)


# ---- 5. the first-record exception --------------------------------------------------------------------------------------------------
def one_record(n):
    rs = np.random.RandomState(44)
    s = ui.rand_seq(rs, n)
    q = bytearray(b"I" * n)
    for j in range(9, n, 53):
        q[j] = qc.LOW[j % len(qc.LOW)]
    return b"@only one\n" + s + b"\n+\n" + bytes(q) + b"\n"


@pytest.mark.parametrize("n", [3000, 70001])
@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_first_record_exception(capi, engine_for, oracles, geom, n):
    """one record cut to 1 line, 2 lines without '\\n', 2 lines, 3 lines, 4 lines without the last '\\n' (and inside the quality line): the
    second line is walked whenever it exists, masked by the fourth as far as that exists.  3 000 bases: against the host framer too;
    70 001 bases: one giant open record, which the host framer refuses"""
    rec, eng, ora = one_record(n), engine_for(geom), oracles(geom)
    nl = [i for i, ch in enumerate(rec) if ch == 10]
    cuts = {"1 line": nl[0] + 1, "2 lines without end": nl[1], "2 lines": nl[1] + 1, "3 lines": nl[2] + 1, "half a quality line": nl[2] + 1 + n // 2,
            "4 lines without end": len(rec) - 1, "whole": len(rec)}
    seen = []
    for name, at in cuts.items():
        text = rec[:at]
        for Q in (53, 0):
            want = model(ora, text, 1, Q)
            seen.append(keys(want))
            if n <= HOST_MAX:
                assert_same(host_route(eng, text, lc.TL(geom), 1, Q), want, name + ": host framer")
            assert_same(long_q(eng, text, 1, Q), want, name + ": one push")
            eng.begin_occ(1)
            push_cuts(capi, eng, text, [at // 2], Q)
            assert_same(ids_of(eng.finish()), want, name + ": two pushes")
            eng.begin_occ(1)
            eng.push_fastq_long_q(text, Q, final=False)
            eng.push_fastq_long_q(b"", Q, final=True)
            assert_same(ids_of(eng.finish()), want, name + ": closed by an empty push")
    assert seen[0] == seen[1] == 0 and len(set(seen[2:])) >= 3  # nothing from one line; unmasked, half masked and fully masked differ
    # not the first record: the same cuts behind a whole record give that record alone
    first = b"@first\n" + ui.rand_seq(np.random.RandomState(45), 300) + b"\n+\n" + b"I" * 300 + b"\n"
    only = model(ora, first, 1, 53)
    assert keys(only) > 0
    for at in (cuts["2 lines"], cuts["4 lines without end"]):
        assert same(model(ora, first + rec[:at], 1, 53), only)
        assert_same(long_q(eng, first + rec[:at], 1, 53, 1025), only, "behind a whole record, cut at %d" % at)


# ---- 6. the carry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_carry_longer_than_what_was_consumed(capi, engine_for, oracles, dev, geom):
    """a first record of 200 bytes, then the 70 001-base record in pieces of 4 099 bytes: the carry outgrows everything consumed, and a
    base and its quality byte arrive seventeen pushes apart"""
    case = "lengths_q_" + geom
    i = [len(s) for s in qc.reads(case)].index(70001)
    big, bigq = qc.reads(case)[i], qc.quals(case)[i]
    small = ui.rand_seq(np.random.RandomState(5), 95)
    text = b"@s hh\n" + small + b"\n+\n" + b"I" * 95 + b"\n" + b"@big\n" + big + b"\n+\n" + bigq + b"\n"
    assert text.index(b"@big") == 200
    ora, eng = oracles(geom), engine_for(geom)
    want = model(ora, text, 1, 53)
    assert keys(want) >= {"L1K7": 3000, "L0K6": 12000}[geom] and not same(want, model(ora, text, 1, 0))
    eng.begin_occ(1)
    push_device(eng, dev(text), len(text), 53, 4099)
    assert_same(ids_of(eng.finish()), want, "device pieces")
    assert_same(long_q(eng, text, 1, 53, 4099), want, "host pieces")


# ---- 7. counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_occurrence_threshold(capi, engine_for, oracles, geom):
    """k-mers seen 13, 14, 15 and 16 times (the reference's count field holds 4 bits) with -n 14 and -n 1"""
    rs = np.random.RandomState(52)
    blocks = [ui.rand_seq(rs, 60) for _ in range(4)]
    recs = []
    for b, times in zip(blocks, (13, 14, 15, 16)):
        recs += [b] * times
    order = rs.permutation(len(recs))
    text = b"".join(b"@%d\n" % i + recs[j] + b"\n+\n" + b"I" * 60 + b"\n" for i, j in enumerate(order))
    ora, eng = oracles(geom), engine_for(geom)
    one, many = model(ora, text, 1, 53), model(ora, text, 14, 53)
    three = model(ora, b"".join(b"@\n" + b + b"\n+\n" + b"I" * 60 + b"\n" for b in blocks[1:]), 1, 53)
    assert 0 < keys(many) < keys(one) and sorted(np.concatenate(many).tolist()) == sorted(np.concatenate(three).tolist())
    for M, want in ((1, one), (14, many)):
        assert_same(host_route(eng, text, lc.TL(geom), M, 53), want, "host framer -n %d" % M)
        for piece in (None, 1023):
            assert_same(long_q(eng, text, M, 53, piece), want, "-n %d piece=%s" % (M, piece))


# ---- 8. engine states ---------------------------------------------------------------------------------------------------------------
def test_two_sketches_in_a_row_and_a_koc_sketch_in_front(capi, engine_for, oracles, dev):
    geom, case = "L1K7", "lengths_q_L1K7"
    text, eng, ora = qc.fastq(case), engine_for(geom), oracles(geom)
    small = small_text()
    want = model(ora, small, 1, 53)
    i = [len(s) for s in qc.reads(case)].index(70001)
    inside = text.index(b"\n" + qc.reads(case)[i] + b"\n") + 30000  # inside the 70 001-base record's sequence line
    # a MK_MODE_KOC long sketch first: its carry and summaries are this sketch's buffers
    rows, stride = lc.rows_of(lc.records(text))
    rc, koc = ora.koc_from_rows(rows, stride)
    assert rc == 0
    eng.begin(capi.MK_MODE_KOC)
    eng.push_fastq_long(text, piece=4099)
    got = eng.finish()
    assert all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, koc))
    assert_same(long_q(eng, text, 2, 53, 4099), fixture(case, 2, 53), "behind a KOC long sketch")
    assert_same(long_q(eng, small, 1, 53, 63), want, "behind a closed sketch")
    eng.begin_occ(1)
    push_device(eng, dev(text), inside, 53, 4099, final=False)  # left open: finished, dropped, begun anew
    assert keys(ids_of(eng.finish())) < MANIFEST["cases"][case]["runs"]["n1_Q53"]["keys"]
    assert_same(long_q(eng, small, 1, 53, 63), want, "behind an abandoned sketch")
    assert_same(long_q(eng, text, 1, 0, 1025), fixture(case, 1, 0), "and the whole file again")


def test_state_and_argument_errors(capi, engine_for, dev):
    geom, case = "L1K7", "lengths_q_L1K7"
    eng, text = engine_for(geom), qc.fastq(case)
    rec = b"@r\nACGT\n+\nIIII\n"

    def exact():
        assert_same(long_q(eng, text, 2, 53, 4099), fixture(case, 2, 53), "after an error")

    def refused(code, word, call):
        with pytest.raises(capi.MkError) as ei:
            call()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)

    for begin in (lambda: eng.begin(capi.MK_MODE_KOC), lambda: eng.begin(capi.MK_MODE_SET)):  # MK_MODE_OCC_SET only, both entries
        begin()
        refused(capi.MK_ERR_STATE, "MK_MODE_OCC_SET", lambda: eng.push_fastq_long_q(rec, 53))
        refused(capi.MK_ERR_STATE, "MK_MODE_OCC_SET", lambda: eng.push_fastq_long_q_device(dev(rec), len(rec), 53))
        eng.finish()
        exact()
    eng.begin_occ(2)  # the plain entries keep refusing this sketch with their message
    refused(capi.MK_ERR_STATE, "for MK_MODE_KOC sketches only", lambda: eng.push_fastq_long(rec))
    refused(capi.MK_ERR_STATE, "for MK_MODE_KOC sketches only", lambda: eng.push_fastq_long_device(dev(rec), len(rec)))
    eng.finish()
    exact()
    eng.begin_occ(1)  # one qmin a sketch
    eng.push_fastq_long_q(rec, 53, final=False)
    refused(capi.MK_ERR_STATE, "qmin", lambda: eng.push_fastq_long_q(rec, 52))
    refused(capi.MK_ERR_STATE, "qmin", lambda: eng.push_fastq_long_q_device(dev(rec), len(rec), 0))
    eng.finish()
    exact()
    eng.begin_occ(1)  # not behind FASTA text
    eng.push_stream(b">g\nACGTACGTACGTACGTACGT\n", final=False)
    refused(capi.MK_ERR_STATE, "mk_sketch_push_stream", lambda: eng.push_fastq_long_q(rec, 53))
    eng.push_stream(b"", final=True)
    eng.finish()
    exact()
    eng.begin_occ(1)  # not behind `final`
    eng.push_fastq_long_q(rec, 53)
    refused(capi.MK_ERR_STATE, "final", lambda: eng.push_fastq_long_q(rec, 53))
    refused(capi.MK_ERR_STATE, "final", lambda: eng.push_fastq_long_q_device(dev(rec), len(rec), 53))
    eng.finish()
    exact()
    eng.begin_occ(1)  # arguments: a host pointer for the device entry, 2^31 bytes in one call, bytes without a pointer
    host = np.frombuffer(rec, dtype=np.uint8)
    refused(capi.MK_ERR_ARG, "not in the memory of device", lambda: eng.push_fastq_long_q_device(host.ctypes.data, len(rec), 53))
    refused(capi.MK_ERR_ARG, "2^31", lambda: eng.push_fastq_long_q_device(dev(rec), 1 << 31, 53))
    assert capi.lib.mk_sketch_push_fastq_long_q(eng.h, None, 5, 1, 53) == capi.MK_ERR_ARG
    eng.finish()
    exact()


# ---- 9. the sinks -------------------------------------------------------------------------------------------------------------------
def gz(raw, text, crc=None):
    """one gzip member around a raw deflate stream"""
    return bytes([0x1f, 0x8b, 8, 0]) + b"\0\0\0\0\x00\x03" + raw + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) & 0xffffffff)


def write(tmp_path, name, data):
    p = str(tmp_path / name)
    open(p, "wb").write(data)
    return p


SMALL = dict(span_bytes=1024, ratio=RATIO, batch_spans=8)


@pytest.mark.parametrize("geom", GEOMS)
def test_gzip_sink(capi, engine_for, tmp_path, geom):
    case = "lengths_q_" + geom
    text, eng = qc.fastq(case), engine_for(geom)
    path = write(tmp_path, "a.fq.gz", gz(gm.deflate(text, 6, 1), text))  # (memLevel 1: many deflate blocks, so many piece starts)
    for M, Q in qc.MQ:
        eng.begin_occ(M)
        st = eng.push_gzip_long_q(path, Q, **SMALL)
        assert_same(ids_of(eng.finish()), fixture(case, M, Q), sub(M, Q))
        assert st.text_bytes == len(text) and st.rows == 0 and st.bad_status == 0 and st.batches >= 2 and st.frame_ms > 0


def phred_text(case):
    """the case's reads with quality lines as a sequencer writes them: every byte drawn from '!' .. 'I', seeded"""
    rs = np.random.RandomState(61)
    return b"".join(b"@r%d\n" % i + rd + b"\n+\n" + bytes(rs.randint(33, 74, size=len(rd)).astype(np.uint8)) + b"\n" for i, rd in enumerate(qc.reads(case)))


@pytest.mark.parametrize("geom", ["L1K7", "L0K6"])
def test_gzip_sink_ordinary_gzip_output(capi, engine_for, oracles, tmp_path, geom):
    """what `gzip -6` writes (zlib level 6, memLevel 8, window 15, a gzip header with a name): the fixture text, and the same reads
    with varied quality bytes, which compress to few long blocks; the default geometry and small spans"""
    import gzip
    case = "lengths_q_" + geom
    eng, ora = engine_for(geom), oracles(geom)
    for name, text, M, Q, want in (("fixture", qc.fastq(case), 2, 53, fixture(case, 2, 53)), ("phred", phred_text(case), 1, 40, None)):
        if want is None:
            want = model(ora, text, M, Q)
            assert keys(want) >= {"L1K7": 100, "L0K6": 1000}[geom] and not same(want, model(ora, text, M, 0))
        path = str(tmp_path / (name + ".fq.gz"))
        with gzip.GzipFile(path, "wb", compresslevel=6, mtime=0) as f:
            f.write(text)
        for geometry in ({}, SMALL):
            eng.begin_occ(M)
            st = eng.push_gzip_long_q(path, Q, **geometry)
            assert_same(ids_of(eng.finish()), want, "%s %s" % (name, geometry))
            assert st.text_bytes == len(text) and st.bad_status == 0 and st.pieces >= 1


def test_gzip_sink_member_concatenation(capi, engine_for, tmp_path):
    case = "lengths_q_L1K7"
    text, eng = qc.fastq(case), engine_for("L1K7")
    parts = [text[a:a + 50000] for a in range(0, len(text), 50000)]
    path = write(tmp_path, "cat.fq.gz", b"".join(gz(gm.deflate(p, 6, 9), p) for p in parts))
    eng.begin_occ(2)
    st = eng.push_gzip_long_q(path, 53, members=True, **SMALL)
    assert_same(ids_of(eng.finish()), fixture(case, 2, 53), "members")
    assert st.members == len(parts) and st.text_bytes == len(text)


@pytest.mark.parametrize("geom", GEOMS)
def test_bgzf_sink(capi, engine_for, tmp_path, geom):
    case = "lengths_q_" + geom
    text, eng = qc.fastq(case), engine_for(geom)
    data, table = bu.write_bgzf(text, payload=4096)
    path = write(tmp_path, "a.fq.gz", data)
    for M, Q in qc.MQ:
        eng.begin_occ(M)
        st = eng.push_bgzf_long_q(path, Q, chunk_bytes=65536)
        assert_same(ids_of(eng.finish()), fixture(case, M, Q), sub(M, Q))
        assert st.text_bytes == len(text) and st.rows == 0 and st.blocks == len(table) and st.bad_block == -1 and st.chunks == (len(text) + 65535) // 65536


def test_gzip_sink_crc_trailer_flipped(capi, engine_for, tmp_path):
    case = "lengths_q_L1K7"
    text, eng = qc.fastq(case), engine_for("L1K7")
    bad = bytearray(gz(gm.deflate(text, 6, 9), text))
    bad[len(bad) - 7] ^= 0x10  # a byte of the CRC32 field, never of the payload
    path = write(tmp_path, "crc.fq.gz", bytes(bad))
    eng.begin_occ(2)
    with pytest.raises(capi.MkError) as ei:
        eng.push_gzip_long_q(path, 53, **SMALL)
    assert ei.value.code == capi.MK_ERR_FORMAT and ei.value.stats.bad_status == capi.MK_INFL_CRC and ei.value.stats.text_bytes == len(text)
    eng.finish()  # what was pushed is finished and dropped ...
    assert_same(long_q(eng, text, 2, 53, 4099), fixture(case, 2, 53), "after the damaged file")  # ... and the next sketch is exact


# ---- 10. poison ---------------------------------------------------------------------------------------------------------------------
ABI_TESTS = ("test_lengths_q or test_device_ or test_host_and_device or test_byte_by_byte or test_equals_the_host_framer or test_record_rule or "
             "test_first_record or test_carry_longer or test_occurrence or test_two_sketches or test_state_and or test_gzip_sink or test_bgzf_sink")


def collected(expr):
    """how many tests of this file the -k expression selects (collection only: no device, no poison)"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "--collect-only", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", expr],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return sum(1 for ln in r.stdout.decode(errors="replace").splitlines() if "::test_" in ln)


@pytest.mark.parametrize("byte", ["0xA5", "0x43"])
def test_abi_tests_under_poison(byte):
    """MK_POISON fills every allocation of the library before use (read once per process: a process of its own): the ABI tests again --
    a kernel that read what nobody wrote (the newline table past the last segment, the carry, the text buffer's slack) would not match"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", ABI_TESTS],
                       env=dict(os.environ, MK_POISON=byte), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    m = re.search(r"(\d+) passed", out)
    want = collected(ABI_TESTS)
    assert want >= 70 and r.returncode == 0 and m and int(m.group(1)) == want and "skipped" not in out and "failed" not in out, out[-3000:]


# ---- 11. the command line -----------------------------------------------------------------------------------------------------------
def run_cli(args, env=None, ok=True):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    if ok:
        assert r.returncode == 0, (args, r.stderr.decode(errors="replace")[-500:])
    routes = [json.loads(ln) for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith('{"input"')]
    return r, routes


@pytest.fixture(scope="module")
def lr_shufs(tmp_path_factory):
    d = tmp_path_factory.mktemp("longreads_q_shufs")
    made = {}

    def get(geom):
        if geom not in made:
            made[geom] = str(d / (geom + ".shuf"))
            lc.get_shuf(geom).write(made[geom])
        return made[geom]
    return get


def check_dir(out, cases, M, Q, inputs):
    """a sketch directory of the files `inputs` against the reference-made fixtures of `cases`, file blocks in input order"""
    stat, names = tg.parse_stat(os.path.join(out, "cofiles.stat"))
    assert names == inputs
    e = [MANIFEST["cases"][c]["runs"][sub(M, Q)] for c in cases]
    assert stat["koc"] == 0 and stat["ctx_ct"] == [x["keys"] for x in e] and stat["all_ctx_ct"] == sum(x["keys"] for x in e)
    for k in ("shuf_id", "kmerlen", "dim_rd_len", "comp_num"):
        assert stat[k] == e[0]["stat"][k]
    for c in range(stat["comp_num"]):
        assert open(os.path.join(out, "combco.%d" % c), "rb").read() == b"".join(open(os.path.join(GOLD, x, sub(M, Q), "combco.%d" % c), "rb").read() for x in cases)
    if len(cases) == 1:
        for f in MANIFEST["cases"][cases[0]]["runs"][sub(M, Q)]["files"]:
            assert filecmp.cmp(os.path.join(out, f), os.path.join(GOLD, cases[0], sub(M, Q), f), shallow=False), f


def same_sketch_files(a, b):
    fa = sorted(f for f in os.listdir(a) if f.startswith("combco"))
    assert fa and fa == sorted(f for f in os.listdir(b) if f.startswith("combco"))
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def flags(M, Q):
    return ["-n", str(M), "-Q", str(Q)]


@pytest.mark.parametrize("gzipped", [False, True])
@pytest.mark.parametrize("geom", GEOMS)
def test_cli_long_reads_q(geom, gzipped, lr_shufs, tmp_path):
    import gzip
    case = "lengths_q_" + geom
    text = qc.fastq(case)
    inp = str(tmp_path / (case + (".fq.gz" if gzipped else ".fq")))
    if gzipped:
        with gzip.GzipFile(inp, "wb", mtime=0) as f:
            f.write(text)
    else:
        open(inp, "wb").write(text)
    for M, Q in qc.MQ:
        out = str(tmp_path / ("out_" + sub(M, Q)))
        r, routes = run_cli(DIST + ["-L", lr_shufs(geom)] + flags(M, Q) + ["--long-reads-q", "--timing", "-o", out, inp])
        check_dir(out, [case], M, Q, [inp])
        assert [(x["route"], x["source"], x["text_bytes"]) for x in routes] == [("long-reads-q", "zcat" if gzipped else "file", len(text))]
    # without the switch nothing changes: the line of 70 001 characters is refused
    r, _ = run_cli(DIST + ["-L", lr_shufs(geom), "-n", "2", "-Q", "53", "-o", str(tmp_path / "out2"), inp], ok=False)
    assert r.returncode == 1 and b"outside the framing contract" in r.stderr


def test_cli_two_files_in_one_run(lr_shufs, tmp_path):
    cases = ["lengths_q_L1K7", "lengths_q_L1K7"]
    inputs = [write(tmp_path, "a.fq", qc.fastq(cases[0])), write(tmp_path, "b.fq", qc.fastq(cases[1]))]
    out = str(tmp_path / "out")
    run_cli(DIST + ["-L", lr_shufs("L1K7")] + flags(2, 53) + ["--long-reads-q", "-o", out] + inputs)
    _, names = tg.parse_stat(os.path.join(out, "cofiles.stat"))
    assert sorted(names) == sorted(inputs)
    check_dir(out, cases, 2, 53, names)


def compressed(kind, text):
    return {"gzip": lambda: gz(gm.deflate(text, 6, 1), text), "bgzf": lambda: bu.write_bgzf(text, payload=65280)[0]}[kind]()


SOURCE = {"gzip": "device-gunzip", "bgzf": "device-inflate"}
HOOKS = {"gzip": ["--gunzip-span-bytes", "1024", "--gunzip-ratio", str(RATIO), "--gunzip-batch-spans", "8"], "bgzf": ["--inflate-chunk-kib", "64"]}


@pytest.mark.parametrize("kind", ["gzip", "bgzf"])
@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_cli_long_inflate_q(geom, kind, lr_shufs, tmp_path):
    case = "lengths_q_" + geom
    text = qc.fastq(case)
    inp = write(tmp_path, case + ".fq.gz", compressed(kind, text))
    for k, hooks in enumerate(([], HOOKS[kind])):
        out = str(tmp_path / ("out%d" % k))
        r, routes = run_cli(DIST + ["-L", lr_shufs(geom)] + flags(2, 53) + ["--long-inflate-q", "--timing", "-o", out] + hooks + [inp])
        check_dir(out, [case], 2, 53, [inp])
        assert len(routes) == 1 and routes[0]["route"] == "long-reads-q" and routes[0]["source"] == SOURCE[kind], "the device route was not taken"
        assert routes[0]["text_bytes"] == len(text) and "fallback" not in routes[0]
    out = str(tmp_path / "zcat")  # --no-device-inflate: zcat under the new switch too
    r, routes = run_cli(DIST + ["-L", lr_shufs(geom)] + flags(2, 53) + ["--long-inflate-q", "--no-device-inflate", "--timing", "-o", out, inp])
    check_dir(out, [case], 2, 53, [inp])
    assert [(x["route"], x["source"]) for x in routes] == [("long-reads-q", "zcat")] and "fallback" not in routes[0]


@pytest.mark.parametrize("geom", ["L3K11", "L1K7"])
def test_cli_long_inflate_q_on_ordinary_gzip_output(geom, lr_shufs, tmp_path):
    """the file as `gzip -6` writes it: the device route is taken (source asserted), with the default geometry"""
    import gzip
    case = "lengths_q_" + geom
    inp = str(tmp_path / (case + ".fq.gz"))
    with gzip.GzipFile(inp, "wb", compresslevel=6, mtime=0) as f:
        f.write(qc.fastq(case))
    out = str(tmp_path / "out")
    r, routes = run_cli(DIST + ["-L", lr_shufs(geom)] + flags(2, 53) + ["--long-inflate-q", "--timing", "-o", out, inp])
    check_dir(out, [case], 2, 53, [inp])
    assert [(x["route"], x["source"], x["text_bytes"]) for x in routes] == [("long-reads-q", "device-gunzip", len(qc.fastq(case)))] and "fallback" not in routes[0]


def test_cli_gunzip_members_and_fallback(lr_shufs, tmp_path):
    from metakssd_amd import capi
    case = "lengths_q_L1K7"
    text = qc.fastq(case)
    parts = [text[a:a + 50000] for a in range(0, len(text), 50000)]
    inp = write(tmp_path, "cat.fq.gz", b"".join(gz(gm.deflate(p, 6, 9), p) for p in parts))
    out = str(tmp_path / "out")
    r, routes = run_cli(DIST + ["-L", lr_shufs("L1K7")] + flags(2, 53) + ["--long-inflate-q", "--gunzip-members", "--timing", "-o", out, inp])
    check_dir(out, [case], 2, 53, [inp])
    assert [(x["route"], x["source"], x["members"]) for x in routes] == [("long-reads-q", "device-gunzip", len(parts))] and "fallback" not in routes[0]
    out = str(tmp_path / "out_noflag")  # without the flag: the status, loudly, what was pushed is dropped and zcat reads the concatenation
    r, routes = run_cli(DIST + ["-L", lr_shufs("L1K7")] + flags(2, 53) + ["--long-inflate-q", "--timing", "-o", out, inp])
    check_dir(out, [case], 2, 53, [inp])
    assert [(x["route"], x["source"], x.get("fallback")) for x in routes] == [("long-reads-q", "zcat", capi.lib.mk_gunzip_status_text(capi.MK_INFL_TRAILING).decode())]


@pytest.mark.parametrize("case", ["dirty_q_L1K7", "lengths_q_L0K6", "lengths_q_L3K11"])
def test_cli_equals_the_default_route_where_that_reads_the_file(case, lr_shufs, tmp_path):
    """reads of at most 19 998 characters: the directory of the default route (the host framer), which is unchanged"""
    geom = qc.CASES[case][1]
    inp = write(tmp_path, case + ".fq", framer_text(case))
    for M, Q in [(1, 0), (2, 53), (1, 74)]:
        base, out = str(tmp_path / ("base_" + sub(M, Q))), str(tmp_path / ("out_" + sub(M, Q)))
        r, routes = run_cli(DIST + ["-L", lr_shufs(geom)] + flags(M, Q) + ["--timing", "-o", base, inp])
        assert all(x["route"] != "long-reads-q" for x in routes)
        r, routes = run_cli(DIST + ["-L", lr_shufs(geom)] + flags(M, Q) + ["--long-reads-q", "--timing", "-o", out, inp])
        assert [x["route"] for x in routes] == ["long-reads-q"]
        same_sketch_files(out, base)
        assert filecmp.cmp(os.path.join(out, "cofiles.stat"), os.path.join(base, "cofiles.stat"), shallow=False)
        assert (os.path.getsize(os.path.join(out, "combco.0")) > 0) == (Q < 74)  # ('I' is 73: -Q 74 masks every window, in both routes)
