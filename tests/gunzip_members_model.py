"""A model of the device's inflate of a CONCATENATION of gzip members (MK_GUNZIP_MEMBERS), in plain Python, on top
of tests/gunzip_model.py, which stays the model of the route without the flag.  tests/test_gunzip_members_model.py holds it against
zlib; its piece table (start bit, kind, text length) and its status are what tests/test_gpu_gunzip_members.py expects from the device.

Coordinates: bytes and bits of the PAYLOAD, which is the file from the first byte behind the first member's header up to the last
eight bytes: it holds every member's deflate stream and, between two of them, a trailer (CRC32, ISIZE) and the next header.  The
last member's trailer lies behind the payload.
  header      at byte q: 1f 8b 08 FLG with FLG & 0xe0 == 0, MTIME XFL OS, then FEXTRA, FNAME, FCOMMENT, FHCRC (skipped, not verified)
              as FLG says, every field inside the payload and at least one payload byte behind the header
  finder      for every span c > 0 the lowest position of either kind in [8 * c * S, min(8 * (c + 1) * S, 8 * len(payload))):
                BLOCK   gunzip_model's rule: a valid non-final dynamic block header at bit p
                MEMBER  a byte q with a header as above that is at most HDR_MAX bytes long, and at the first bit behind it a dynamic
                        block header, final or not, that passes the same validation.  Members that open with a stored or a fixed
                        block are no candidates
              The two kinds never meet at one position: 0x1f has BFINAL set.
  pieces      piece 0 starts at bit 0 (a block start), every candidate starts another; a MEMBER piece begins by parsing its header
  boundary    behind a final block the decode aligns to the next byte p.  p == len(payload): the stream ends.  Fewer than 8 + 10 + 1
              bytes left: BAD_MEMBER.  Otherwise the 8 bytes at p are the member's trailer and give a member record (symbols of the
              piece so far, CRC32, ISIZE); at q = p + 8 the piece stops when the next piece is a MEMBER piece that starts there,
              is MISSED when it is past the next piece's start, and otherwise parses the header at q (BAD_MEMBER when there is none)
              and decodes on
  stop        before a block header, at == end stops the piece only when the next piece is a BLOCK piece; past end is MISSED
  distances   a piece that has seen the start of the member it is in -- piece 0, a MEMBER piece, any piece behind a boundary --
              holds a distance against that start (BAD_DISTANCE) and gives no markers; a piece that starts inside a member keeps
              gunzip_model's 32768 in front of its first symbol
  check       every member's text length mod 2^32 against its ISIZE (OUTPUT_LEN), then its CRC32 (CRC); the first member in stream
              order that fails gives the status, behind every status a piece gave"""
import struct
import zlib

import gunzip_model as gm
from gunzip_model import (BAD_BLOCK, BAD_CODE, BAD_DISTANCE, CAPACITY, CRC, DBASE, DEXT, FIXED_LENS, INPUT, LBASE, LEXT, MISSED, OK,  # noqa: F401
                          OUTPUT_LEN, TRAILING, WINDOW, Bad, Bits, Code)

BAD_MEMBER = 11
BLOCK, MEMBER = 0, 1
HDR_MAX = 4096  # the longest header the finder takes for a member start; the decode walks a header of any length


def header_end(pay, q):
    """the first byte behind the member header at byte q of the payload; None: no header with a payload byte behind it"""
    n = len(pay)
    if n - q < 10 or pay[q] != 0x1f or pay[q + 1] != 0x8b or pay[q + 2] != 8 or pay[q + 3] & 0xe0:
        return None
    flg, at = pay[q + 3], q + 10
    if flg & 4:
        if n - at < 2:
            return None
        at += 2 + (pay[at] | pay[at + 1] << 8)
        if at > n:
            return None
    for bit in (8, 16):
        if flg & bit:
            z = pay.find(b"\0", at)
            if z < 0:
                return None
            at = z + 1
    if flg & 2:
        at += 2
    return at if at < n else None


def dynamic_valid(pay, p, any_final):
    """gunzip_model.header_valid's full validation at bit p; any_final: BFINAL may be set"""
    b = Bits(pay, p)
    final, kind = b.get(1), b.get(2)
    if kind != 2 or (final and not any_final):
        return False
    try:
        lit, dist = gm.dynamic_header(b)
    except Bad:
        return False
    return not b.past() and lit.kind == 0 and gm.usable(dist)


def member_valid(pay, q):
    """the finder's second rule at byte q"""
    h = header_end(pay, q)
    return h is not None and h - q <= HDR_MAX and dynamic_valid(pay, 8 * h, True)


def magic_offsets(pay, lo, hi):
    """bytes q in [lo, hi) that pass the finder's cheap test for a member: the 32-bit compare"""
    out, q = [], pay.find(b"\x1f\x8b\x08", lo)
    while 0 <= q < hi:
        if q + 3 < len(pay) and not pay[q + 3] & 0xe0:
            out.append(q)
        q = pay.find(b"\x1f\x8b\x08", q + 1)
    return out


def all_member_starts(pay):
    """every byte of the payload at which the member rule holds"""
    return [q for q in magic_offsets(pay, 0, len(pay)) if member_valid(pay, q)]


def find_candidates(pay, span):
    """-> [(bit, kind)]: the candidate of every span c > 0 that has one, ascending"""
    out = []
    for c in range(1, (len(pay) + span - 1) // span):
        lo, hi = 8 * c * span, min(8 * (c + 1) * span, 8 * len(pay))
        best = None
        for p in gm.cheap_survivors(pay, lo, hi):
            if gm.header_valid(pay, p):
                best = (p, BLOCK)
                break
        for q in magic_offsets(pay, lo >> 3, hi >> 3):
            if best is not None and 8 * q > best[0]:
                break
            if member_valid(pay, q):
                best = (8 * q, MEMBER)
                break
        if best is not None:
            out.append(best)
    return out


def decode_piece(pay, start, kind, end, end_kind, cap, first):
    """-> (status, symbols, the bit the piece stopped at, [(symbols so far, crc32, isize)] of the members that ended in it).
    end: the next piece's start (None for the last piece), end_kind its kind"""
    out, records = [], []
    b = Bits(pay, start)
    mstart = 0 if first or kind == MEMBER else None  # the first symbol of the member the piece is in, where it has seen it
    try:
        if kind == MEMBER:
            h = header_end(pay, start >> 3)
            if h is None:
                raise Bad(BAD_MEMBER)
            b = Bits(pay, 8 * h)
        while True:
            if end is not None:
                if b.pos == end and end_kind == BLOCK:
                    return OK, out, b.pos, records
                if b.pos > end:
                    raise Bad(MISSED)
            if b.past():
                raise Bad(INPUT)
            final, btype = b.get(1), b.get(2)
            if btype == 0:
                b.get(-b.pos & 7)
                n, nn = b.get(16), b.get(16)
                if n ^ nn != 0xffff:
                    raise Bad(BAD_BLOCK)
                at = b.pos >> 3
                if b.past() or at + n > len(pay):
                    raise Bad(INPUT)
                if len(out) + n > cap:
                    raise Bad(CAPACITY)
                out += pay[at:at + n]
                b = Bits(pay, 8 * (at + n))
            elif btype == 3:
                raise Bad(BAD_BLOCK)
            else:
                if btype == 1:
                    lit, dist = Code(FIXED_LENS[:288]), Code(FIXED_LENS[288:])
                else:
                    lit, dist = gm.dynamic_header(b)
                if not gm.usable(lit) or not gm.usable(dist):
                    raise Bad(BAD_CODE)
                while True:
                    if b.past():
                        raise Bad(INPUT)
                    s = lit.decode(b)
                    if s < 0:
                        raise Bad(BAD_CODE)
                    if s < 256:
                        if len(out) + 1 > cap:
                            raise Bad(CAPACITY)
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    s -= 257
                    if s >= 29:
                        raise Bad(BAD_CODE)
                    n = LBASE[s] + b.get(LEXT[s])
                    d = dist.decode(b)
                    if d < 0:
                        raise Bad(BAD_CODE)
                    if d >= 30:
                        raise Bad(BAD_DISTANCE)
                    d = DBASE[d] + b.get(DEXT[d])
                    pos = len(out)
                    if d > (pos + WINDOW if mstart is None else pos - mstart):
                        raise Bad(BAD_DISTANCE)
                    if pos + n > cap:
                        raise Bad(CAPACITY)
                    for i in range(n):
                        src = pos - d + i
                        out.append(out[src] if src >= 0 else 0x8000 | (WINDOW + src))
            if final:  # the boundary walk
                if b.past():
                    raise Bad(INPUT)
                p = (b.pos + 7) >> 3
                if p == len(pay):
                    if end is not None:
                        raise Bad(MISSED)  # the payload ends in front of the next piece's start: that start lies nowhere
                    return OK, out, b.pos, records
                if len(pay) - p < 8 + 10 + 1:
                    raise Bad(BAD_MEMBER)
                records.append((len(out),) + struct.unpack_from("<II", pay, p))
                q = p + 8
                b = Bits(pay, 8 * q)
                if end is not None:
                    if 8 * q == end and end_kind == MEMBER:
                        return OK, out, b.pos, records
                    if 8 * q > end:
                        raise Bad(MISSED)
                h = header_end(pay, q)
                if h is None:
                    raise Bad(BAD_MEMBER)
                b = Bits(pay, 8 * h)
                mstart = len(out)
    except Bad as e:
        return e.status, out, b.pos, records


def piece_cap(pay, start, end, ratio):
    return gm.piece_cap(pay, start, end, ratio)


def record_slots(pay, start, end):
    """member records the host gives a piece room for: a member takes at least 20 bytes"""
    stop = 8 * len(pay) if end is None else end
    return ((stop + 7) // 8 - start // 8) // 20 + 2


def run(payload, span, ratio=1 << 20, trailer=None):
    """-> (status, text, pieces, members): status is the first piece's that is not OK (pieces in stream order) or, when every piece
    is OK, the first member's whose check fails; text the resolved text (None with a piece's status); pieces =
    [(start bit, kind, symbols)] as far as they were decoded; members = [(text length, crc32, isize)] of every member whose end was
    met, trailer values as the file states them.  trailer: the (crc32, isize) behind the payload; None leaves the last member unchecked"""
    starts = [(0, BLOCK)] + find_candidates(payload, span)
    window = bytearray(WINDOW)
    text, table, ends = bytearray(), [], []
    for k, (start, kind) in enumerate(starts):
        end, end_kind = starts[k + 1] if k + 1 < len(starts) else (None, BLOCK)
        st, syms, _, recs = decode_piece(payload, start, kind, end, end_kind, piece_cap(payload, start, end, ratio), k == 0)
        table.append((start, kind, len(syms)))
        assert len(recs) <= record_slots(payload, start, end)
        if st:
            return st, None, table, member_list(text, ends)
        ends += [(len(text) + n, crc, isize) for n, crc, isize in recs]
        piece = bytes(s if s < 0x8000 else window[s & 0x7fff] for s in syms)
        text += piece
        window = (window + piece)[-WINDOW:]
    if trailer is not None:
        ends.append((len(text),) + tuple(trailer))
    members = member_list(text, ends)
    at = 0
    for n, crc, isize in members:
        if n & 0xffffffff != isize:
            return OUTPUT_LEN, bytes(text), table, members
        if zlib.crc32(bytes(text[at:at + n])) != crc:
            return CRC, bytes(text), table, members
        at += n
    return OK, bytes(text), table, members


def member_list(text, ends):
    out, at = [], 0
    for e, crc, isize in ends:
        out.append((e - at, crc, isize))
        at = e
    return out


def split_file(f):
    """a gzip file -> (the first header's length, payload, (crc32, isize) of its last eight bytes)"""
    h = header_end(f + b"\0", 0)
    assert h is not None and len(f) - h >= 9
    return h, f[h:-8], struct.unpack("<II", f[-8:])


def run_file(f, span, ratio=1 << 20):
    _, pay, trailer = split_file(f)
    return run(pay, span, ratio, trailer)


# ---- the files both test files use -----------------------------------------------------------------------------------------------------

def gz(raw, text, extra=None, name=None, comment=None, hcrc=False, crc=None, isize=None, cm=8, flg_or=0):
    """one gzip member around a raw deflate stream"""
    flg = (4 if extra is not None else 0) | (8 if name else 0) | (16 if comment else 0) | (2 if hcrc else 0) | flg_or
    head = bytes([0x1f, 0x8b, cm, flg]) + b"\0\0\0\0\x00\x03"
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name:
        head += name + b"\0"
    if comment:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + raw + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) if isize is None else isize) & 0xffffffff)


def cut_members(text, size, level=6, mem=9):
    """the text as members of `size` text bytes each"""
    return b"".join(gz(gm.deflate(text[a:a + size], level, mem), text[a:a + size]) for a in range(0, len(text), size))


def aligned_member(text, k):
    """a member whose final block, a fixed block of k nine-bit literals, ends (2 + k) % 8 bits into its last byte"""
    import bgzf_util as bu
    w = bu.BitWriter()
    w.out += gm.deflate(text, 6, 1, finish=False)  # ends byte-aligned, behind a full flush
    bu.fixed_block(w, [200] * k, 1)
    end_bit = (8 * len(w.out) + w.n) % 8
    raw = w.done()
    return gz(raw, text + bytes([200] * k)), text + bytes([200] * k), end_bit


def empty_dynamic_member(extra=None):
    """a member of one final dynamic block that holds the end-of-block code alone: a member start the finder takes, no text"""
    import bgzf_util as bu
    w = bu.BitWriter()
    bu.dynamic_block(w, bu.spread(257, {65: 2, 66: 2, 67: 2, 256: 2}), [1, 1], [], 1)
    return gz(w.done(), b"", extra=extra)


def missed_file():
    """a stored block whose bytes hold, at payload byte 1030 (just behind the start of span 1 of 1024-byte spans), the image of a
    gzip header and of a valid dynamic block header behind it; then a final block.  The finder takes the image for a member start,
    the piece in front decodes past it"""
    import bgzf_util as bu
    w = bu.BitWriter()
    bu.dynamic_block(w, bu.spread(257, {65: 2, 66: 2, 67: 2, 256: 2}), [1, 1], [], 0, stop="ops")
    image = bytes([0x1f, 0x8b, 8, 0]) + b"\0\0\0\0\x00\x03" + w.done()
    data = bytearray(b"\xff" * 3000)
    at = 1030 - 5  # the stored bytes start at payload byte 5
    data[at:at + len(image)] = image
    w = bu.BitWriter()
    bu.stored_block(w, bytes(data), 0)
    bu.fixed_block(w, list(b"@r\nACGT\n+\nIIII\n"), 1)
    raw = w.done()
    return gz(raw, zlib.decompress(raw, -15)), zlib.decompress(raw, -15)


def zero_symbol_file(text):
    """-> (file, text, span): behind a member of many blocks an empty dynamic member and another member, and a span at which both
    are member-start pieces: the first of the two gives 0 symbols"""
    raw = gm.deflate(text, 6, 1)
    f = gz(raw, text) + empty_dynamic_member(extra=bytes(300)) + gz(raw, text)
    _, pay, trailer = split_file(f)
    q = len(raw) + 8  # the empty member's header in the payload
    for span in range(300, 64, -1):  # a span start a few bytes in front of q: q is the span's first candidate, the third member the next span's
        if 0 <= q - q // span * span < 8:
            st, _, table, _ = run(pay, span, 1040, trailer)
            if st == OK and (8 * q, MEMBER, 0) in table:
                return f, text + text, span
    raise AssertionError("no span gives a member-start piece without symbols")


def legal_files(text):
    """-> [(name, file, text)]: concatenations of members the device must decode with status OK at every span"""
    import bgzf_util as bu
    raw = gm.deflate(text, 6, 1)
    one = gz(raw, text)
    empty = gz(b"\x03\x00", b"")
    out = [("two_l6_m1", one + gz(raw, text, name=b"abcd"), text + text),
           ("m600", cut_members(text, 600), text)]
    for k in range(1, 9):
        f, t, _ = aligned_member(text, k)
        out.append(("align_%d" % k, f + one, t + text))
    for name, kw in (("fextra", dict(extra=b"xy" * 10)), ("fname", dict(name=b"reads.fastq")), ("fcomment", dict(comment=b"a comment")),
                     ("fhcrc", dict(hcrc=True)), ("all_four", dict(extra=b"q", name=b"n", comment=b"c", hcrc=True)),
                     ("fextra_700", dict(extra=b"xy" * 350))):
        out.append((name, one + gz(raw, text, **kw), text + text))
    out.append(("empty_first", empty + one + one, text + text))
    out.append(("empty_middle", one + empty + one, text + text))
    out.append(("empty_last", one + one + empty, text + text))
    out.append(("empty_three", one + empty * 3 + one, text + text))
    f, t, _ = zero_symbol_file(text)
    out.append(("zero_symbols", f, t))
    for name in ("stored_only", "fixed_only"):
        t = text[:60000]
        r = gm.deflate(t, 0) if name == "stored_only" else gm.deflate(t, 6, 9, zlib.Z_FIXED)
        out.append((name, one + gz(r, t) + one, text + t + text))
    assert all(zlib_text(f) == t for _, f, t in out)
    return out


def zlib_text(f):
    """what zlib gives for a concatenation of members (gzip.decompress's loop)"""
    out = b""
    while f:
        d = zlib.decompressobj(31)
        out += d.decompress(f)
        assert d.eof
        f = d.unused_data
    return out


def status_files(text):
    """-> [(name, file, status)]: files whose decode must give exactly this status with the flag"""
    import bgzf_util as bu
    raw = gm.deflate(text, 6, 1)
    one = gz(raw, text)
    out = [("crc_first", gz(raw, text, crc=zlib.crc32(text) ^ 0x8000) + one, CRC),
           ("isize_middle", one + gz(raw, text, isize=len(text) + 1) + one, OUTPUT_LEN),
           ("zeros_512", one + bytes(512), BAD_MEMBER),
           ("zeros_4", one + bytes(4), BAD_MEMBER),
           ("junk", one + b"junk" * 8, BAD_MEMBER),
           ("cm_7", one + gz(raw, text, cm=7), BAD_MEMBER),
           ("flg_0x20", one + gz(raw, text, flg_or=0x20), BAD_MEMBER),
           ("cut_in_fname", one + bytes([0x1f, 0x8b, 8, 8]) + b"\0\0\0\0\x00\x03" + b"n" * 30, BAD_MEMBER)]
    w = bu.BitWriter()
    bu.fixed_block(w, list(b"@r\nACGTACGT\n"), 1)
    a = w.done()
    w = bu.BitWriter()
    bu.fixed_block(w, list(b"ACGT") + [(4, 8)], 1)  # 8 back from the member's fifth byte: four bytes in front of its start
    b = w.done()
    out.append(("reach_in_front", gz(a, zlib.decompress(a, -15)) + gz(b, b"ACGT" + b"GT\nA"), BAD_DISTANCE))
    return out
