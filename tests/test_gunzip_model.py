"""tests/gunzip_model.py against zlib: the finder's rule over every bit offset, and finder + marker decode + window chain + resolve
giving zlib's text, on the streams tests/test_gpu_gunzip.py gives the device"""
import zlib

import pytest

import bgzf_util as bu
import gunzip_model as gm

TEXT = bu.golden_text("fq_ragged")
STREAMS = gm.legal_streams(TEXT)
SPANS = (256, 1024, 65536)


def true_starts(raw):
    """the bits at which non-final dynamic blocks start: stop the one-piece decode in front of every block"""
    starts, at = [], 0
    while True:
        h = bu.parse_block_header(raw, at)
        if h["final"]:
            return starts
        if h["type"] == 2:
            starts.append(at)
        # the end of this block: the first bit at which a piece that starts here stops with OK
        at = block_end(raw, at)


def block_end(raw, start):
    class Stop(Exception):
        pass
    b = gm.Bits(raw, start)
    final, kind = b.get(1), b.get(2)
    assert not final
    if kind == 0:
        b.get(-b.pos & 7)
        n = b.get(16)
        b.get(16)
        return b.pos + 8 * n
    lit, dist = (gm.Code(gm.FIXED_LENS[:288]), gm.Code(gm.FIXED_LENS[288:])) if kind == 1 else gm.dynamic_header(b)
    while True:
        s = lit.decode(b)
        if s == 256:
            return b.pos
        if s > 256:
            b.get(gm.LEXT[s - 257])
            d = dist.decode(b)
            b.get(gm.DEXT[d])


@pytest.mark.parametrize("name,raw,text", [s for s in STREAMS if s[0] in ("l6_m1", "l1_m1", "l9_m2", "l6_m9", "fixed_only", "stored_only")],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_finder_rule_holds_exactly_at_the_non_final_dynamic_block_starts(name, raw, text):
    want = true_starts(raw)
    assert gm.all_valid_headers(raw) == want
    if name in ("l6_m9", "fixed_only", "stored_only"):
        assert want == []
    else:
        assert len(want) > 10


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("name,raw,text", STREAMS, ids=lambda v: v if isinstance(v, str) else "")
def test_model_gives_zlibs_text(name, raw, text, span):
    st, got, pieces = gm.run(raw, span)
    assert st == gm.OK
    assert got == zlib.decompress(raw, -15) == text
    assert sum(n for _, n in pieces) == len(text) and pieces[0][0] == 0
    assert all(8 * span * (p // (8 * span)) <= p for p, _ in pieces)
    assert len({p // (8 * span) for p, _ in pieces}) == len(pieces)  # at most one piece a span
    if span == 256 and name in ("l1_m1", "l6_m1", "repeat_20k_x10"):
        assert len(pieces) > 20
    if name in ("fixed_only", "stored_only", "empty", "l6_m9"):
        assert len(pieces) == 1


def test_markers_are_copied_from_markers_through_several_windows():
    raw = dict((n, r) for n, r, _ in STREAMS)["repeat_20k_x10"]
    starts = [0] + gm.find_candidates(raw, 256)
    marks = total = 0
    for k in range(1, len(starts)):
        end = starts[k + 1] if k + 1 < len(starts) else None
        st, syms, _ = gm.decode_piece(raw, starts[k], end, 1 << 30, False, end is None)
        assert st == gm.OK
        marks += sum(s >= 0x8000 for s in syms)
        total += len(syms)
    assert marks > total // 2 and total > 4 * gm.WINDOW


def test_statuses():
    raw = dict((n, r) for n, r, _ in STREAMS)["l6_m1"]
    assert gm.run(raw, 256, ratio=2)[0] == gm.CAPACITY
    assert gm.run(raw + raw, 1024)[0] == gm.TRAILING
    assert gm.run(raw[:-40], 1024)[0] in (gm.INPUT, gm.BAD_BLOCK, gm.BAD_CODE, gm.BAD_LENGTHS, gm.BAD_DISTANCE)
    one = gm.deflate(b"A" * (1 << 20), 6, 9)
    assert gm.run(one, 1024, ratio=8)[0] == gm.CAPACITY
