"""tests/gunzip_members_model.py, the model of the device's inflate of a concatenation of gzip members, against zlib:
the text of every file tests/test_gpu_gunzip_members.py gives the device, the member rule and the block rule of the finder on files
whose candidates are known, and the statuses.  No GPU."""
import gzip

import pytest

import bgzf_util as bu
import gunzip_model as gm
import gunzip_members_model as mm

TEXT = bu.golden_text("fq_ragged")
SPANS = (256, 1024, 65536)
RATIO = 1040
LEGAL = mm.legal_files(TEXT)
STATUS = mm.status_files(TEXT)


def test_the_text_is_the_golden_one():
    assert len(TEXT) == 97730


@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("name", [n for n, _, _ in LEGAL])
def test_model_equals_zlib(name, span):
    f, text = next((f, t) for n, f, t in LEGAL if n == name)
    assert gzip.decompress(f) == text
    st, got, table, members = mm.run_file(f, span, RATIO)
    assert st == mm.OK and got == text
    assert sum(n for _, _, n in table) == len(text) and table[0][:2] == (0, mm.BLOCK)
    assert sum(n for n, _, _ in members) == len(text)
    if span == 65536 and len(f) <= 65536:
        assert len(table) == 1


def test_member_rule_on_600_byte_members():
    f = mm.cut_members(TEXT, 600)
    assert (len(f), f.count(b"\x1f\x8b\x08")) == (30062, 163)
    h, pay, _ = mm.split_file(f)
    true_starts, at = [], 0
    for a in range(0, len(TEXT), 600):
        true_starts.append(at - h)
        at += len(mm.gz(gm.deflate(TEXT[a:a + 600]), TEXT[a:a + 600]))
    assert at == len(f) and len(true_starts) == 163
    assert mm.magic_offsets(pay, 0, len(pay)) == true_starts[1:]
    assert mm.all_member_starts(pay) == true_starts[1:]  # the 162 inner starts: none false, none missed
    assert gm.all_valid_headers(pay) == []               # every block is final: the block rule holds nowhere
    st, text, table, members = mm.run(pay, 256, RATIO, mm.split_file(f)[2])
    assert st == mm.OK and text == TEXT and len(members) == 163
    assert len(table) > 100 and all(k == mm.MEMBER and s // 8 in true_starts for s, k, _ in table[1:])
    st, text, table, members = mm.run(pay, 65536, RATIO, mm.split_file(f)[2])
    assert (st, text, table, len(members)) == (mm.OK, TEXT, [(0, mm.BLOCK, len(TEXT))], 163)


def test_block_rule_on_two_members():
    raw = gm.deflate(TEXT, 6, 1)
    f = mm.gz(raw, TEXT) + mm.gz(raw, TEXT, name=b"abcd")
    _, pay, _ = mm.split_file(f)
    own = gm.all_valid_headers(raw)
    assert len(own) == 88
    second = 8 * (len(raw) + 8 + 10 + 5)  # trailer, fixed header, "abcd\0"
    assert second == 178712
    assert own[0] == 0 and gm.all_valid_headers(pay) == own + [second + p for p in own]  # nothing in the trailer and header between
    assert mm.all_member_starts(pay) == [len(raw) + 8]


def test_zero_symbol_member_piece():
    f, text, span = mm.zero_symbol_file(TEXT)
    st, got, table, members = mm.run_file(f, span, RATIO)
    assert st == mm.OK and got == text and [n for n, _, _ in members] == [len(TEXT), 0, len(TEXT)]
    assert [t for t in table if t[1] == mm.MEMBER and t[2] == 0]


def test_alignments_cover_every_bit():
    assert sorted(mm.aligned_member(TEXT, k)[2] for k in range(1, 9)) == list(range(8))


def test_stored_and_fixed_members_are_no_piece_starts():
    for name in ("stored_only", "fixed_only"):
        f = dict((n, f) for n, f, _ in LEGAL)[name]
        _, pay, _ = mm.split_file(f)
        second = f.index(b"\x1f\x8b\x08", 10) - (len(f) - len(pay) - 8)
        assert second not in mm.all_member_starts(pay) and len(mm.all_member_starts(pay)) == 1


@pytest.mark.parametrize("name", [n for n, _, _ in STATUS])
def test_statuses(name):
    f, want = next((f, w) for n, f, w in STATUS if n == name)
    for span in SPANS:
        assert mm.run_file(f, span, RATIO)[0] == want
    if want in (mm.CRC, mm.OUTPUT_LEN):
        assert gm.run(mm.split_file(f)[1], 1024)[0] == gm.TRAILING  # without the flag


def test_false_member_start_is_missed():
    f, text = mm.missed_file()
    _, pay, _ = mm.split_file(f)
    assert mm.member_valid(pay, 1030) and mm.find_candidates(pay, 1024)[0] == (8 * 1030, mm.MEMBER)
    assert mm.run_file(f, 1024, RATIO)[0] == mm.MISSED
    assert mm.run_file(f, 65536, RATIO)[:2] == (mm.OK, text)


def test_one_member_equals_the_one_member_model():
    """on a file of one member the two models agree, but for the kind in the table"""
    for name, raw, text in gm.legal_streams(TEXT)[:4]:
        st, got, table = gm.run(raw, 1024, RATIO)
        assert mm.run(raw, 1024, RATIO)[:3] == (st, got, [(s, mm.BLOCK, n) for s, n in table])
