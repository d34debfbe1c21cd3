"""BGZF files written with Python's zlib, for tests/test_bgzf_host.py and tests/test_gpu_bgzf.py: per member the header with the
'BC' subfield, one raw deflate stream, CRC32 and ISIZE; the 28-byte end marker last.  No fixture is committed: the tests
re-compress the committed tests/golden/inputs/*.fq.gz into a temporary directory."""
import gzip
import os
import struct
import zlib

import golden_cases as gc

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member_raw(deflate, data, extra_subfields=b""):
    """one member around a ready-made raw deflate stream of `data`"""
    xlen = 6 + len(extra_subfields)
    total = 12 + xlen + len(deflate) + 8
    assert total - 1 < 65536, "BSIZE is 16 bits"
    head = b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\x00\xff" + struct.pack("<H", xlen)
    return head + extra_subfields + b"BC" + struct.pack("<HH", 2, total - 1) + deflate + struct.pack("<II", zlib.crc32(data), len(data))


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for cut in flush_at:
        out += c.compress(data[at:cut]) + c.flush(zlib.Z_FULL_FLUSH)
        at = cut
    return out + c.compress(data[at:]) + c.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    return member_raw(deflate_raw(data, level, strategy, flush_at), data)


def write_bgzf(data, payload=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True, sizes=None):
    """-> (file bytes, table): table = what mk_bgzf_scan must return, one dict per member (capi.BGZF_FIELDS).  `sizes`: the text
    bytes of the members one by one (0 = an empty member), instead of equal pieces of `payload` bytes."""
    if sizes is None:
        sizes = [min(payload, len(data) - at) for at in range(0, len(data), payload)]
    assert sum(sizes) == len(data)
    out, table, at = b"", [], 0
    for n in list(sizes) + ([None] if eof else []):
        piece = b"" if n is None else data[at:at + n]
        m = EOF_MARKER if n is None else member(piece, level, strategy)
        table.append({"in_off": len(out), "out_off": at, "in_len": len(m), "pay_off": 18, "pay_len": len(m) - 26,
                      "crc32": zlib.crc32(piece), "isize": len(piece)})
        out += m
        at += len(piece)
    return out, table


def golden_text(name):
    """the text of a committed input, e.g. 'fq_ragged_crlf'"""
    return gzip.open(os.path.join(gc.GOLDEN, "inputs", name + ".fq.gz"), "rb").read()


class BitWriter:
    """deflate bit order: values LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def done(self):
        self.align()
        return bytes(self.out)


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_symbol(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xC0 + s - 280, 8)


def fixed_match(w, length, dist):
    ls = max(i for i in range(29) if LBASE[i] <= length and (i == 28 or length < 258))
    fixed_symbol(w, 257 + ls)
    w.bits(length - LBASE[ls], LEXT[ls])
    ds = max(i for i in range(30) if DBASE[i] <= dist)
    w.code(ds, 5)
    w.bits(dist - DBASE[ds], DEXT[ds])


def max_distance_member(first):
    """a member whose second half repeats its first 32768 bytes through matches of distance 32768 -- zlib itself never emits
    that distance, so the stream is written by hand: one stored block, then one fixed-Huffman block of matches"""
    assert len(first) == 32768
    w = BitWriter()
    w.bits(0, 1); w.bits(0, 2); w.align()
    w.bits(32768, 16); w.bits(32768 ^ 0xFFFF, 16)
    w.out += first
    w.bits(1, 1); w.bits(1, 2)
    left = 32768
    while left:
        n = 258 if left >= 258 + 3 or left == 258 else left - 3 if left > 258 else left
        fixed_match(w, n, 32768)
        left -= n
    fixed_symbol(w, 256)
    raw = w.done()
    data = first + first
    assert zlib.decompress(raw, -15) == data
    return member_raw(raw, data), data
