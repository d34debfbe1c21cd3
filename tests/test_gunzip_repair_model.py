"""tests/gunzip_repair_model.py against zlib: the repair rule of MK_GUNZIP_REPAIR on streams with planted false
piece starts.  Every test first asserts what its fixture is for -- without the repair the status is MISSED (or CAPACITY), the
planted bits are the finder's candidates -- so a changed helper cannot turn it into a test of nothing.  The device is held against
the same model in tests/test_gpu_gunzip_repair.py."""
import functools
import zlib

import pytest

import bgzf_util as bu
import gunzip_model as gm
import gunzip_repair_model as rm

SPAN = rm.SPAN


@functools.lru_cache(maxsize=None)
def fixture(name):
    return getattr(rm, name)()


def test_missed_stream_resumes_at_a_fixed_block():
    raw, text, bits = fixture("missed_stream")
    assert gm.find_candidates(raw, SPAN) == bits and gm.run(raw, SPAN)[0] == gm.MISSED
    st, got, table, repairs = rm.run(raw, SPAN)
    assert (st, got, repairs) == (gm.OK, text, 1) and got == zlib.decompress(raw, -15)
    assert len(table) == 2 and table[0] == (0, 3000) and table[1][0] not in bits
    b = gm.Bits(raw, table[1][0])  # the resumed piece starts at the final FIXED block: a block of any type may start one
    assert (b.get(1), b.get(2)) == (1, 1)


def test_four_images_drop_in_one_step_and_no_piece_is_new():
    raw, text, bits = fixture("four_images")
    cands = gm.find_candidates(raw, SPAN)
    assert len(bits) == 4 and all(b in cands for b in bits) and gm.run(raw, SPAN)[0] == gm.MISSED
    at = 0
    for b in bits:  # in the `@` line of a record of the stored part, at the first byte of a span
        assert b % (8 * SPAN) == 0 and raw[b // 8:b // 8 + 42] == rm.header_image()
        at = text.index(rm.header_image(), at + 1)
        line = text.rfind(b"\n", 0, at) + 1
        assert text[line:line + 2] == b"@r" and text[at + 42:at + 43] == b"\n" and text[:line].count(b"\n") % 4 == 0
    st, got, table, repairs = rm.run(raw, SPAN)
    assert (st, got, repairs) == (gm.OK, text, 4) and got == zlib.decompress(raw, -15)
    assert [s for s, _ in table] == [0] + [c for c in cands if c not in bits]  # the tail's first block was a candidate already
    assert len(table) > 16


def test_two_false_starts_with_true_ones_between_take_two_new_pieces():
    raw, text, bits = fixture("two_rounds")
    cands = gm.find_candidates(raw, SPAN)
    assert len(bits) == 2 and all(b in cands for b in bits) and gm.run(raw, SPAN)[0] == gm.MISSED
    assert any(bits[0] < c < bits[1] for c in cands)  # true starts between the two
    st, got, table, repairs = rm.run(raw, SPAN)
    assert (st, got, repairs) == (gm.OK, text, 2)
    new = [s for s, _ in table if s and s not in cands]
    assert len(new) == 2 and bits[0] < new[0] < bits[0] + 8 * SPAN and bits[1] < new[1] < bits[1] + 8 * SPAN
    assert all(gm.header_valid(raw, s) for s in new)  # block starts the finder did not take: the image was its span's candidate
    assert len(table) == len(cands) + 1  # two dropped, two new


def test_capacity_merges_until_the_stored_block_fits():
    raw, text, bits = fixture("four_images")
    st, _, table = gm.run(raw, SPAN, 4)
    assert st == gm.CAPACITY
    k = len(table) - 1  # the piece in front of the stored block, and no piece in front of it meets its capacity
    starts = [0] + gm.find_candidates(raw, SPAN)
    assert starts[k + 1] == bits[0] and table[k][0] == starts[k]
    st, got, table4, repairs = rm.run(raw, SPAN, 4)
    assert (st, got, repairs) == (gm.OK, text, 4)
    assert table4 == rm.run(raw, SPAN)[2]


def test_capacity_stands_after_eight_merges():
    text = bu.golden_text("fq_ragged")
    raw = gm.deflate(text, 6, 1)
    st, _, table = gm.run(raw, 256, 2)
    assert st == gm.CAPACITY and len(table) == 1 and len(gm.find_candidates(raw, 256)) > 20
    st, got, table, repairs = rm.run(raw, 256, 2)
    assert (st, got, len(table), repairs) == (gm.CAPACITY, None, 1, rm.MERGES)
    one = b"A" * (1 << 20)  # the stream's last piece: nothing to merge with
    assert rm.run(gm.deflate(one, 6, 9), SPAN, 8)[::3] == (gm.CAPACITY, 0)


@pytest.mark.parametrize("back", (4000, 6000))
def test_damage_behind_a_repaired_piece_gives_its_own_status(back):
    raw, text, bits = fixture("four_images")
    bad = bytearray(raw)
    bad[len(raw) - back] ^= 0x04
    assert 8 * (len(raw) - back) > bits[-1] + 8 * 26000  # in the dynamic blocks behind the stored one
    assert gm.run(bytes(bad), SPAN)[0] == gm.MISSED  # without the repair the false start hides it
    st, got, table, repairs = rm.run(bytes(bad), SPAN)
    assert repairs == 4 and st != gm.MISSED
    assert st == (gm.BAD_CODE if back == 4000 else gm.OK) and got != text  # (OK: only the CRC can tell)


@pytest.mark.parametrize("name", ("l6_m1", "sync_flush", "level0_between", "stored_only"))
def test_a_clean_stream_is_untouched(name):
    raw, text = {n: (r, t) for n, r, t in gm.legal_streams(bu.golden_text("fq_ragged"))}[name]
    for span in (256, 1024):
        assert rm.run(raw, span) == gm.run(raw, span) + (0,)
