"""mk_gzip_scan_stream (host): mk_gzip_scan's header rule without its limits on ISIZE -- every FLG combination against Python's gzip
module, ISIZE 0, truncated headers, BGZF -- and mk_gzip_scan answering as before"""
import gzip
import struct
import zlib

import pytest

import bgzf_util as bu
import test_gzip_host as th
from metakssd_amd import capi

TEXT = th.TEXT


@pytest.mark.parametrize("flg,extra", th.FLAGS)
def test_every_flag_combination(flg, extra, tmp_path):
    f, pay_off = th.gz_file(TEXT, flg, extra)
    assert gzip.decompress(f) == TEXT  # the fixture itself
    want = th.expect(f, pay_off, TEXT)
    assert capi.gzip_scan_stream(f) == want == capi.gzip_scan(f)
    assert zlib.decompress(f[want["pay_off"]:want["pay_off"] + want["pay_len"]], -15) == TEXT
    p = tmp_path / "x.fq.gz"
    p.write_bytes(f)
    assert capi.gzip_scan_stream(path=str(p)) == want  # through the descriptor


def test_isize_is_only_the_length_mod_2_32():
    f, pay_off = th.gz_file(b"")
    assert capi.gzip_scan(f) is None  # as before
    assert capi.gzip_scan_stream(f) == {"pay_off": pay_off, "pay_len": 2, "crc32": 0, "isize": 0}
    g, pay_off = th.gz_file(TEXT)
    for isize in (0, 1, (64 << 20) + 1, 0xffffffff):
        big = bytearray(g); struct.pack_into("<I", big, len(big) - 4, isize)
        assert capi.gzip_scan_stream(bytes(big)) == dict(th.expect(g, pay_off, TEXT), isize=isize)
        assert (capi.gzip_scan(bytes(big)) is None) == (isize == 0 or isize > 64 << 20)


@pytest.mark.parametrize("flg,extra", [(th.FEXTRA | th.FNAME | th.FCOMMENT | th.FHCRC, bytes(300)), (th.FNAME, b""), (0, b"")])
def test_header_cut_at_every_byte(flg, extra):
    f, pay_off = th.gz_file(TEXT, flg, extra)
    for n in range(pay_off + 1):
        assert capi.gzip_scan_stream(f[:n]) is None, n
    for n in range(pay_off):
        cut = f[:n] + struct.pack("<II", 0x12345678, 1000)
        got = capi.gzip_scan_stream(cut)
        assert got == capi.gzip_scan(cut)
        if got is not None:
            assert flg and got["pay_off"] <= n and got["pay_off"] + got["pay_len"] + 8 == len(cut) and got["pay_len"] >= 1


def test_not_one_member():
    f, _ = th.gz_file(TEXT)
    for bit in (0x20, 0x40, 0x80):
        bad = bytearray(f); bad[3] |= bit
        assert capi.gzip_scan_stream(bytes(bad)) is None
    assert capi.gzip_scan_stream(th.gz_file(TEXT, cm=7)[0]) is None
    assert capi.gzip_scan_stream(b"\x1f\x8c" + f[2:]) is None
    assert capi.gzip_scan_stream(b"") is None
    assert capi.gzip_scan_stream(f[:10] + b"\x03" + f[-6:]) is None  # 17 bytes
    assert capi.gzip_scan_stream(b"BZh91AY&SY" + bytes(40)) is None
    assert capi.gzip_scan_stream(TEXT) is None


def test_bgzf_and_concatenations_pass_like_there():
    """a BGZF file is a chain of members: the scan sees the first header and the last trailer, as mk_gzip_scan does; the command line
    asks mk_bgzf_scan first, and the decode says MK_INFL_TRAILING"""
    f, table = bu.write_bgzf(TEXT, payload=3000)
    assert capi.bgzf_scan(f) is not None
    got = capi.gzip_scan_stream(f)
    assert capi.gzip_scan(f) is None  # (the end marker's ISIZE is 0)
    assert got["pay_off"] == 18 and got["pay_off"] + got["pay_len"] + 8 == len(f) and got["isize"] == 0
    g = bu.write_bgzf(TEXT, payload=3000, eof=False)[0]
    assert capi.bgzf_scan(g) is not None and capi.gzip_scan_stream(g) == capi.gzip_scan(g) and capi.gzip_scan(g)["pay_off"] == 18
    a, pa = th.gz_file(TEXT[:1000], th.FNAME)
    b, _ = th.gz_file(TEXT)
    assert capi.gzip_scan_stream(a + b) == capi.gzip_scan(a + b) == {"pay_off": pa, "pay_len": len(a) + len(b) - pa - 8, "crc32": zlib.crc32(TEXT), "isize": len(TEXT)}
