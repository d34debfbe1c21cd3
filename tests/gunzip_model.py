"""A model of the device's two-pass inflate of ONE deflate stream, in plain Python: the finder's rule, the decode
to 16-bit symbols with markers, the window chain and the resolve.  tests/test_gunzip_model.py holds it against zlib; its piece table
(start bit, text length) is what tests/test_gpu_gunzip.py expects from the device.

Coordinates: bits of the raw deflate stream `raw` (the gzip payload), bit 0 = the least significant bit of its first byte.
  spans     span c is the bytes [c * S, (c + 1) * S) of raw
  finder    for every span c > 0 the first bit p, 8 * c * S <= p < min(8 * (c + 1) * S, 8 * len(raw)), at which a NON-FINAL DYNAMIC
            block header is valid and lies inside raw: BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29, a complete code length code, the
            lengths decode without overrun (a 16 needs a predecessor), symbol 256 has a code, a complete literal/length code, and a
            distance code that is complete, empty, or one code of one bit
  pieces    piece 0 starts at bit 0, every candidate starts another; a piece ends where the next one starts
  decode    a piece decodes block after block.  Before every block header: at the next piece's start it stops, past it the status is
            MISSED.  The final block ends it: TRAILING unless it is the last piece and the stream ends within the payload's last byte.
            A match source in front of the piece gives the marker 0x8000 | (32768 + source), source < 0 counted from the piece's
            start; more than 32768 in front (piece 0: any) is BAD_DISTANCE.  More than R * (bytes the piece covers) symbols: CAPACITY
  chain     W(c) = the last 32768 bytes of the text up to the end of piece c
  resolve   text[off(c) + i] = sym < 0x8000 ? sym : W(c - 1)[sym & 0x7fff]"""
import zlib

import numpy as np

OK, BAD_BLOCK, BAD_LENGTHS, BAD_CODE, BAD_DISTANCE, INPUT, OUTPUT_LEN, CRC, TRAILING, MISSED, CAPACITY = range(11)
WINDOW = 32768
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32


class Bad(Exception):
    def __init__(self, status):
        self.status = status


class Bits:
    """the stream as one Python integer with zeros behind its end; `pos` may run past the end, past() tells"""

    def __init__(self, raw, pos=0):
        self.n = 8 * len(raw)
        self.raw = raw
        self.pos = pos
        self._load()

    def _load(self):
        b = self.pos >> 3
        self.buf = int.from_bytes(self.raw[b:b + 512], "little") >> (self.pos & 7)
        self.left = 8 * 512 - 8

    def get(self, n):
        if self.left < n:
            self._load()
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.left -= n
        self.pos += n
        return v

    def past(self):
        return self.pos > self.n


class Code:
    """a canonical code from its lengths; kind 0 complete, 1 over-subscribed, 2 incomplete"""

    def __init__(self, lens):
        self.count = [0] * 16
        for n in lens:
            self.count[n] += 1
        self.count[0] = 0
        left = 1
        self.kind = 0
        for n in range(1, 16):
            left = (left << 1) - self.count[n]
            if left < 0:
                self.kind = 1
        if self.kind == 0 and left > 0:
            self.kind = 2
        self.maxlen = max([n for n in range(16) if self.count[n]] + [0])
        self.syms = [s for n in range(1, 16) for s, m in enumerate(lens) if m == n]

    def decode(self, b):
        code = first = index = 0
        for n in range(1, 16):
            code |= b.get(1)
            c = self.count[n]
            if code - c < first:
                return self.syms[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        return -1


def usable(code):
    """what the decoder takes for a literal/length or distance code: complete, or at most one code of one bit"""
    return code.kind == 0 or (code.kind == 2 and code.maxlen <= 1)


def dynamic_header(b):
    """the header behind BFINAL and BTYPE -> (literal/length code, distance code); raises Bad"""
    nl, nd, nc = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
    if nl > 286 or nd > 30:
        raise Bad(BAD_LENGTHS)
    cl = [0] * 19
    for i in range(nc):
        cl[CLORDER[i]] = b.get(3)
    clc = Code(cl)
    if clc.kind:
        raise Bad(BAD_CODE)
    lens = []
    while len(lens) < nl + nd:
        if b.past():
            raise Bad(INPUT)
        s = clc.decode(b)
        if s < 0:
            raise Bad(BAD_CODE)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Bad(BAD_LENGTHS)
            val, rep = lens[-1], 3 + b.get(2)
        elif s == 17:
            val, rep = 0, 3 + b.get(3)
        else:
            val, rep = 0, 11 + b.get(7)
        if len(lens) + rep > nl + nd:
            raise Bad(BAD_LENGTHS)
        lens += [val] * rep
    if lens[256] == 0:
        raise Bad(BAD_LENGTHS)
    return Code(lens[:nl]), Code(lens[nl:])


def header_valid(raw, p):
    """the finder's rule at bit p"""
    v = int.from_bytes(raw[p >> 3:(p >> 3) + 11], "little") >> (p & 7)  # the cheap tests first: they only save work
    if v & 7 != 4 or (v >> 3) & 31 > 29 or (v >> 8) & 31 > 29:
        return False
    if sum(128 >> n for n in ((v >> (17 + 3 * i)) & 7 for i in range(((v >> 13) & 15) + 4)) if n) != 128:
        return False
    b = Bits(raw, p)
    if b.get(3) != 4:  # BFINAL 0, BTYPE 2
        return False
    try:
        lit, dist = dynamic_header(b)
    except Bad:
        return False
    return not b.past() and lit.kind == 0 and usable(dist)


def cheap_survivors(raw, lo, hi):
    """bit offsets in [lo, hi) that pass the three header bits -- the rest of the cheap tests only saves work"""
    bits = np.unpackbits(np.frombuffer(raw[lo >> 3:(hi >> 3) + 2] + b"\0\0", np.uint8), bitorder="little")[(lo & 7):]
    n = hi - lo
    m = (bits[:n] == 0) & (bits[1:n + 1] == 0) & (bits[2:n + 2] == 1)
    return [lo + int(i) for i in np.nonzero(m)[0]]


def find_candidates(raw, span):
    """-> the candidate bit of every span c > 0 that has one, ascending"""
    out = []
    for c in range(1, (len(raw) + span - 1) // span):
        lo, hi = 8 * c * span, min(8 * (c + 1) * span, 8 * len(raw))
        for p in cheap_survivors(raw, lo, hi):
            if header_valid(raw, p):
                out.append(p)
                break
    return out


def all_valid_headers(raw):
    """every bit of the stream at which the finder's rule holds"""
    return [p for p in cheap_survivors(raw, 0, 8 * len(raw)) if header_valid(raw, p)]


def decode_piece(raw, start, end, cap, first, last):
    """-> (status, symbols, the bit the piece stopped at).  end: the next piece's start (None for the last piece)"""
    b = Bits(raw, start)
    out = []
    try:
        while True:
            if not last:
                if b.pos == end:
                    return OK, out, b.pos
                if b.pos > end:
                    raise Bad(MISSED)
            if b.past():
                raise Bad(INPUT)
            final, kind = b.get(1), b.get(2)
            if kind == 0:
                b.get(-b.pos & 7)
                n, nn = b.get(16), b.get(16)
                if n ^ nn != 0xffff:
                    raise Bad(BAD_BLOCK)
                at = b.pos >> 3
                if b.past() or at + n > len(raw):
                    raise Bad(INPUT)
                if len(out) + n > cap:
                    raise Bad(CAPACITY)
                out += raw[at:at + n]
                b = Bits(raw, 8 * (at + n))
            elif kind == 3:
                raise Bad(BAD_BLOCK)
            else:
                if kind == 1:
                    lit, dist = Code(FIXED_LENS[:288]), Code(FIXED_LENS[288:])
                else:
                    lit, dist = dynamic_header(b)
                if not usable(lit) or not usable(dist):
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
                    if d > pos + (0 if first else WINDOW):
                        raise Bad(BAD_DISTANCE)
                    if pos + n > cap:
                        raise Bad(CAPACITY)
                    for i in range(n):
                        src = pos - d + i
                        out.append(out[src] if src >= 0 else 0x8000 | (WINDOW + src))
            if final:
                if b.past():
                    raise Bad(INPUT)
                if not last or (b.pos + 7) >> 3 < len(raw):
                    raise Bad(TRAILING)
                return OK, out, b.pos
    except Bad as e:
        return e.status, out, b.pos


def piece_cap(raw, start, end, ratio):
    stop = 8 * len(raw) if end is None else end
    return ratio * ((stop + 7) // 8 - start // 8)


def run(raw, span, ratio=1 << 20):
    """-> (status, text, pieces): status is the first piece's that is not OK (pieces in stream order), text the resolved text
    (None with a status), pieces = [(start bit, symbols)] as far as they were decoded"""
    starts = [0] + find_candidates(raw, span)
    window = bytearray(WINDOW)
    text, table = bytearray(), []
    for k, start in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else None
        st, syms, _ = decode_piece(raw, start, end, piece_cap(raw, start, end, ratio), k == 0, end is None)
        table.append((start, len(syms)))
        if st:
            return st, None, table
        piece = bytes(s if s < 0x8000 else window[s & 0x7fff] for s in syms)  # resolve against W(k - 1)
        text += piece
        window = (window + piece)[-WINDOW:]                                    # the chain: W(k)
    return OK, bytes(text), table


# ---- the streams both test files use ---------------------------------------------------------------------------------------------------

def deflate(data, level=6, mem=9, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush=zlib.Z_SYNC_FLUSH, finish=True):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    out, at = b"", 0
    for cut in flush_at:
        out += c.compress(data[at:cut]) + c.flush(flush)
        at = cut
    return out + c.compress(data[at:]) + c.flush(zlib.Z_FINISH if finish else zlib.Z_FULL_FLUSH)


def stored_stretch(data, step=40000):
    """non-final stored blocks, byte-aligned at both ends"""
    out = b""
    for a in range(0, len(data), step):
        d = data[a:a + step]
        out += b"\0" + len(d).to_bytes(2, "little") + (len(d) ^ 0xffff).to_bytes(2, "little") + d
    return out


def level0_between(text):
    """dynamic blocks, a stretch of stored blocks, dynamic blocks again (each part a stream of its own, cut at full flushes)"""
    a, b = len(text) // 3, 2 * len(text) // 3
    return deflate(text[:a], 6, 1, finish=False) + stored_stretch(text[a:b], 700) + deflate(text[b:], 6, 1)


def legal_streams(text):
    """-> [(name, raw deflate stream, text)], every stream at most 64 KB"""
    out = [("l%d_m%d" % (lv, m), deflate(text, lv, m), text) for lv in (1, 6, 9) for m in (1, 2, 9)]
    rep = text[:20000] * 10
    out.append(("repeat_20k_x10", deflate(rep, 6, 1), rep))
    cuts = list(range(5000, len(text), 9000))
    out.append(("sync_flush", deflate(text, 6, 1, flush_at=cuts), text))
    out.append(("full_flush", deflate(text, 6, 1, flush_at=cuts, flush=zlib.Z_FULL_FLUSH), text))
    out.append(("level0_between", level0_between(text), text))
    out.append(("fixed_only", deflate(text[:60000], 6, 9, zlib.Z_FIXED), text[:60000]))
    out.append(("stored_only", deflate(text[:60000], 0), text[:60000]))
    out.append(("empty", deflate(b""), b""))
    out.append(("no_complete_record", deflate(b"@r1\nACGT"), b"@r1\nACGT"))
    assert all(len(raw) <= 65536 and zlib.decompress(raw, -15) == t for _, raw, t in out)
    return out
