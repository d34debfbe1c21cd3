"""mk_bgzf_scan (host code, no GPU): a file counts as BGZF only when every byte of it belongs to a well-formed member; anything
else stays on the `zcat -fc` route"""
import glob
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_util as bz
import golden_cases as gc
from metakssd_amd import capi

RAGGED = bz.golden_text("fq_ragged")


@pytest.mark.parametrize("payload,level", [(100, 1), (65280, 6), (7, 0)])
def test_writer_makes_files_gzip_and_zcat_read(payload, level, tmp_path):
    """guards the fixture writer: Python's gzip and the zcat binary both give the original text back"""
    data = RAGGED[:3000] if payload == 7 else RAGGED
    f, table = bz.write_bgzf(data, payload=payload, level=level)
    assert gzip.decompress(f) == data
    assert table[-1]["isize"] == 0 and f.endswith(bz.EOF_MARKER)
    if shutil.which("zcat"):
        p = tmp_path / "x.fq.gz"
        p.write_bytes(f)
        r = subprocess.run(["zcat", "-fc", "--", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == data
    m, d = bz.max_distance_member(bytes(np.random.RandomState(1).randint(0, 256, 32768, dtype=np.uint8)))
    assert gzip.decompress(m) == d


@pytest.mark.parametrize("payload", [1, 7, 100, 65280])
def test_scan_returns_what_the_writer_used(payload):
    data = RAGGED[:600] if payload == 1 else RAGGED[:5000] if payload == 7 else RAGGED
    f, table = bz.write_bgzf(data, payload=payload, level=6)
    assert capi.bgzf_scan(f) == table


def test_scan_random_sizes_empty_member_and_no_end_marker(tmp_path):
    rs = np.random.RandomState(5)
    sizes, left = [], len(RAGGED)
    while left:
        n = min(left, int(rs.choice([1, 2, 63, 64, 65, 1000, 4096, 30000, 65280])))
        sizes.append(n)
        left -= n
        if len(sizes) == 3:
            sizes.append(0)  # an empty member in the middle
    for eof in (True, False):
        f, table = bz.write_bgzf(RAGGED, sizes=sizes, level=1, eof=eof)
        assert gzip.decompress(f) == RAGGED
        assert capi.bgzf_scan(f) == table
        p = tmp_path / ("eof%d.gz" % eof)
        p.write_bytes(f)
        assert capi.bgzf_scan(path=str(p)) == table  # through the file descriptor
    # an end marker in the middle, and a file that is nothing but the end marker
    f2 = bz.write_bgzf(RAGGED[:1000], payload=300)[0] + bz.write_bgzf(RAGGED[1000:2000], payload=300)[0]
    t2 = capi.bgzf_scan(f2)
    assert t2 is not None and sum(t["isize"] for t in t2) == 2000 and [t["isize"] for t in t2].count(0) == 2
    assert capi.bgzf_scan(bz.EOF_MARKER) == [{"in_off": 0, "out_off": 0, "in_len": 28, "pay_off": 18, "pay_len": 2, "crc32": 0, "isize": 0}]
    # a second subfield in front of 'BC' moves the payload
    m = bz.member_raw(bz.deflate_raw(b"ACGT" * 10), b"ACGT" * 10, extra_subfields=b"XY" + struct.pack("<H", 3) + b"abc")
    t3 = capi.bgzf_scan(m)
    assert t3 is not None and t3[0]["pay_off"] == 25 and t3[0]["isize"] == 40 and t3[0]["in_len"] == len(m)


def test_committed_golden_gz_files_stay_on_the_zcat_route():
    files = sorted(glob.glob(os.path.join(gc.GOLDEN, "inputs", "*.gz")))
    assert files
    for p in files:
        assert capi.bgzf_scan(path=p) is None, p
        assert capi.bgzf_scan(open(p, "rb").read()) is None, p


def test_not_bgzf():
    f, table = bz.write_bgzf(RAGGED[:20000], payload=5000, level=6)
    assert capi.bgzf_scan(f) is not None
    assert capi.bgzf_scan(b"") is None
    assert capi.bgzf_scan(f + gzip.compress(b"tail\n")) is None              # a plain gzip member behind the chain
    assert capi.bgzf_scan(gzip.compress(b"head\n") + f) is None              # ... and in front of it
    assert capi.bgzf_scan(f[:table[2]["in_off"]] + gzip.compress(b"mid\n") + f[table[2]["in_off"]:]) is None
    assert capi.bgzf_scan(f + b"\0") is None and capi.bgzf_scan(f + b"garbage") is None  # trailing bytes
    for cut in (1, 8, 27, 29, 100):                                           # (28 would take exactly the end marker off)
        assert capi.bgzf_scan(f[:-cut]) is None, cut                          # a member cut off by the end of the file
    no_eof = bz.write_bgzf(RAGGED[:20000], payload=5000, eof=False)[0]
    assert capi.bgzf_scan(no_eof[:-3]) is None
    last = table[-2]
    past = bytearray(f[:last["in_off"] + last["in_len"]])                     # BSIZE of the last member points past the end
    struct.pack_into("<H", past, last["in_off"] + 16, last["in_len"] + 10)
    assert capi.bgzf_scan(bytes(past)) is None
    short = bytearray(f)                                                      # BSIZE smaller than header + trailer
    struct.pack_into("<H", short, 16, 20)
    assert capi.bgzf_scan(bytes(short)) is None
    data = b"ACGT" * 10
    d = bz.deflate_raw(data)
    nobc = b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"XY" + struct.pack("<HH", 2, len(d) + 25) + d + \
        struct.pack("<II", zlib.crc32(data), len(data))
    assert gzip.decompress(nobc) == data and capi.bgzf_scan(nobc) is None     # an extra field without 'BC'
    flg = bytearray(f)
    flg[3] = 4 | 8                                                            # FLG is not FEXTRA exactly
    assert capi.bgzf_scan(bytes(flg)) is None
    big = bytearray(f)
    struct.pack_into("<I", big, table[0]["in_len"] - 4, 65537)                # ISIZE above 64 KiB
    assert capi.bgzf_scan(bytes(big)) is None
    slen = bytearray(f)
    struct.pack_into("<H", slen, 14, 3)                                       # 'BC' with SLEN 3
    assert capi.bgzf_scan(bytes(slen)) is None


def test_inflate_has_no_cpu_path():
    if capi.device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(capi.MkError) as ei:
        capi.Inflate(0)
    assert ei.value.code == capi.MK_ERR_NO_DEVICE and "no CPU path" in str(ei.value)


# ---- the hand-made deflate streams of tests/test_gpu_bgzf.py: zlib says what they are -------------------------------------------------
RANDOM = bytes(np.random.RandomState(77).randint(0, 256, 200000, dtype=np.uint8))
LEGAL = {"long_codes": bz.legal_long_codes, "degenerate": bz.legal_degenerate, "header_ops": bz.legal_header_ops,
         "length_258": bz.legal_length_258, "literal_runs": bz.legal_literal_runs, "random": lambda: bz.legal_random(RANDOM)}


@pytest.mark.parametrize("group", sorted(LEGAL))
def test_hand_made_legal_streams_are_what_zlib_reads(group):
    cases = LEGAL[group]()
    assert len({c[0] for c in cases}) == len(cases) >= 3
    for c in cases:
        name, raw, text = c[:3]
        assert zlib.decompress(raw, -15) == text, name
        assert gzip.decompress(bz.member_raw(raw, text)) == text, name
        if len(c) > 3:
            assert c[3](bz.parse_block_header(raw)), name  # the header does what the case is named for
        if group == "random":
            assert bz.first_block_type(raw) == 2 and len(set(text)) == 256, name


@pytest.mark.parametrize("maxl,maxd,flip", [(15, 15, False), (15, 15, True), (10, 8, False), (11, 9, True)])
def test_chain_case_decodes_a_symbol_at_every_code_length(maxl, maxd, flip):
    lit_lens, dist_lens, tokens = bz.chain_case(maxl, maxd, 1, flip)
    assert bz.kraft(lit_lens) == bz.kraft(dist_lens) == 32768
    lit, dist = bz.used_symbols(tokens)
    assert sorted({lit_lens[s] for s in lit}) == list(range(1, maxl + 1))
    assert sorted({dist_lens[s] for s in dist}) == list(range(1, maxd + 1))
    assert 2000 <= len(bz.apply_tokens(tokens)) <= 4500
    w = bz.BitWriter()
    bz.dynamic_block(w, lit_lens, dist_lens, tokens, 1)
    h = bz.parse_block_header(w.done())
    assert h["lit_lens"] == lit_lens and h["dist_lens"] == dist_lens


def test_hand_made_illegal_streams_are_refused_by_zlib():
    cases = bz.illegal_cases()
    assert len({c[0] for c in cases}) == len(cases)
    for name, member, raw, level, classes in cases:
        assert capi.bgzf_scan(member + bz.EOF_MARKER) is not None, name  # the container is sound: the stream is what is wrong
        if level == "stream":
            with pytest.raises(zlib.error):
                zlib.decompress(raw, -15)
        else:  # a stream zlib reads, in a member whose ISIZE is one too small
            assert level == "member" and classes == ("OUTPUT_LEN",)
            assert len(zlib.decompress(raw, -15)) == struct.unpack("<I", member[-4:])[0] + 1, name
            with pytest.raises(gzip.BadGzipFile):
                gzip.decompress(member)
        assert all(hasattr(capi, "MK_INFL_" + c) for c in classes)


def test_window_sweep_hits_every_phase():
    f, text, phases = bz.sweep_file(RANDOM)
    assert gzip.decompress(f) == text
    bz.assert_sweep_phases(phases)


def test_hand_encoder_round_trips_a_fastq(tmp_path):
    f = bz.hand_bgzf(RAGGED)
    assert gzip.decompress(f) == RAGGED
    table = capi.bgzf_scan(f)
    assert table is not None and len(table) == (len(RAGGED) + 4095) // 4096 + 1
    member, raw, starts = bz.hand_member(RAGGED[:4096])
    assert zlib.decompress(raw, -15) == RAGGED[:4096]
    heads = [bz.parse_block_header(raw, at) for at in starts]
    assert [h["type"] for h in heads] == [0, 1, 2, 2] and [h["final"] for h in heads] == [0, 0, 0, 1]
    assert all(max(h["lit_lens"]) == 15 for h in heads[2:])  # long-code sets
    if shutil.which("zcat"):
        p = tmp_path / "hand.fq.gz"
        p.write_bytes(f)
        r = subprocess.run(["zcat", "-fc", "--", str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == RAGGED
