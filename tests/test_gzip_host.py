"""mk_gzip_scan (host): the header and trailer of a plain gzip file against Python's gzip / zlib -- every FLG combination, every
truncation of the header, and everything that must stay on the `zcat -fc` route"""
import gzip
import io
import struct
import zlib

import pytest

from metakssd_amd import capi

TEXT = b">g\n" + b"ACGTTGCA" * 500 + b"\n"
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def gz_file(text, flg=0, extra=b"", name=b"genome.fna", comment=b"a comment", level=6, cm=8):
    """a gzip member written field by field (RFC 1952) -> (file, offset of the payload)"""
    raw = zlib.compressobj(level, zlib.DEFLATED, -15)
    pay = raw.compress(text) + raw.flush()
    head = bytes([0x1f, 0x8b, cm, flg]) + b"\0\0\0\0" + b"\x00\x03"
    if flg & FEXTRA:
        head += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        head += name + b"\0"
    if flg & FCOMMENT:
        head += comment + b"\0"
    if flg & FHCRC:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + pay + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff), len(head)


def expect(f, pay_off, text):
    return {"pay_off": pay_off, "pay_len": len(f) - pay_off - 8, "crc32": zlib.crc32(text), "isize": len(text)}


FLAGS = [(0, b""), (FTEXT, b""), (FEXTRA, b""), (FEXTRA, bytes(range(256)) + bytes(44)), (FNAME, b""), (FCOMMENT, b""), (FHCRC, b""),
         (FNAME | FCOMMENT, b""), (FEXTRA | FHCRC, b"xy"), (FTEXT | FHCRC | FEXTRA | FNAME | FCOMMENT, bytes(300))]


@pytest.mark.parametrize("flg,extra", FLAGS)
def test_every_flag_combination(flg, extra, tmp_path):
    f, pay_off = gz_file(TEXT, flg, extra)
    assert gzip.decompress(f) == TEXT  # the fixture itself
    want = expect(f, pay_off, TEXT)
    assert capi.gzip_scan(f) == want
    assert zlib.decompress(f[want["pay_off"]:want["pay_off"] + want["pay_len"]], -15) == TEXT
    p = tmp_path / "x.fna.gz"
    p.write_bytes(f)
    assert capi.gzip_scan(path=str(p)) == want  # through the descriptor


def test_what_python_gzip_writes(tmp_path):
    for level in (1, 6, 9):
        b = io.BytesIO()
        with gzip.GzipFile("genome.fna", "wb", level, b, mtime=7) as g:  # FNAME set
            g.write(TEXT)
        f = b.getvalue()
        got = capi.gzip_scan(f)
        assert got is not None and got["isize"] == len(TEXT) and got["crc32"] == zlib.crc32(TEXT)
        assert zlib.decompress(f[got["pay_off"]:got["pay_off"] + got["pay_len"]], -15) == TEXT
        assert got["pay_off"] + got["pay_len"] + 8 == len(f)


@pytest.mark.parametrize("flg,extra", [(FEXTRA | FNAME | FCOMMENT | FHCRC, bytes(300)), (FNAME, b""), (0, b"")])
def test_header_cut_at_every_byte(flg, extra):
    f, pay_off = gz_file(TEXT, flg, extra)
    for n in range(pay_off + 1):
        # the header alone, cut anywhere (with the payload's first byte at most): never a file for the device
        assert capi.gzip_scan(f[:n]) is None, n
    for n in range(pay_off):
        # ... and with eight bytes behind the cut that could pass for a trailer: the header still runs past the file, or what
        # is left between it and the trailer is no payload
        cut = f[:n] + struct.pack("<II", 0x12345678, 1000)
        got = capi.gzip_scan(cut)
        if got is not None:  # the cut header parses as a shorter, complete header: then the ranges must still lie inside the file
            assert flg and got["pay_off"] <= n and got["pay_off"] + got["pay_len"] + 8 == len(cut) and got["pay_len"] >= 1


def test_every_truncation_of_a_400_byte_header():
    f, pay_off = gz_file(TEXT, FEXTRA | FNAME | FCOMMENT | FHCRC, bytes(300), name=b"n" * 40, comment=b"c" * 41)
    assert pay_off == 10 + 2 + 300 + 41 + 42 + 2 and pay_off >= 397
    for n in range(pay_off + 9):
        assert capi.gzip_scan(f[:n]) is None or n > pay_off + 8, n
    assert capi.gzip_scan(f) == expect(f, pay_off, TEXT)


def test_not_for_the_device():
    f, pay_off = gz_file(TEXT)
    for bit in (0x20, 0x40, 0x80):
        bad = bytearray(f); bad[3] |= bit
        assert capi.gzip_scan(bytes(bad)) is None, "reserved FLG bit %#x" % bit
    assert capi.gzip_scan(gz_file(TEXT, cm=7)[0]) is None
    assert capi.gzip_scan(b"\x1f\x8b\x09" + f[3:]) is None
    assert capi.gzip_scan(b"\x1f\x8c" + f[2:]) is None
    assert capi.gzip_scan(b"") is None
    assert capi.gzip_scan(gz_file(b"")[0]) is None                      # ISIZE 0
    assert capi.gzip_scan(f[:10] + b"\x03\x00"[:1] + f[-6:]) is None     # 17 bytes
    assert len(f[:10] + b"\x03" + f[-6:]) == 17
    assert capi.gzip_scan(b"BZh91AY&SY" + bytes(40)) is None             # .bz2
    assert capi.gzip_scan(TEXT) is None                                   # plain text
    big = bytearray(f); struct.pack_into("<I", big, len(big) - 4, (64 << 20) + 1)
    assert capi.gzip_scan(bytes(big)) is None                             # ISIZE above MK_BATCH_FILE_MAX
    ok = bytearray(f); struct.pack_into("<I", ok, len(ok) - 4, 64 << 20)
    assert capi.gzip_scan(bytes(ok))["isize"] == 64 << 20


def test_two_members_pass_the_scan_with_the_whole_range():
    """only the decode can tell a concatenation from one member (MK_INFL_TRAILING, tests/test_gpu_gzfasta.py): the scan sees the first
    header and the last trailer"""
    a, pa = gz_file(TEXT[:1000], FNAME)
    b, _ = gz_file(TEXT)
    got = capi.gzip_scan(a + b)
    assert got == {"pay_off": pa, "pay_len": len(a) + len(b) - pa - 8, "crc32": zlib.crc32(TEXT), "isize": len(TEXT)}
