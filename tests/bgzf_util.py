"""BGZF files written with Python's zlib, for tests/test_bgzf_host.py and tests/test_gpu_bgzf.py: per member the header with the
'BC' subfield, one raw deflate stream, CRC32 and ISIZE; the 28-byte end marker last.  No fixture is committed: the tests
re-compress the committed tests/golden/inputs/*.fq.gz into a temporary directory.  Below: a deflate writer for the streams zlib's
compressor never emits (chosen code lengths, header ops, block layouts, malformed ones) and the cases made with it."""
import gzip
import os
import struct
import zlib

import numpy as np

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


# ---- a deflate writer for streams no compressor emits --------------------------------------------------------------------------------
# Tokens: an int is a literal byte; (length, distance) is a match; (length, distance, symbol) writes the length with the given length
# symbol (258 as 284 + extra 31); ("bits", value, n) puts n raw bits (a code no symbol has).  A block is written from code lengths the
# caller chooses, legal or not: nothing here repairs a set.
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical_codes(lens):
    """RFC 1951 3.2.2: symbol -> (code, length) for the non-zero lengths.  An over-subscribed set gives codes that overflow their
    length; they are masked when written, which is what an illegal stream wants."""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def kraft(lens):
    """sum of 2^-len over the non-zero lengths, in units of 2^-15: 32768 is a complete set"""
    return sum(1 << (15 - n) for n in lens if n)


def complete_lengths(nsym, maxlen):
    """nsym code lengths with Kraft sum exactly 1 whose longest is maxlen, sorted: 1, 2, ..., maxlen, maxlen for nsym == maxlen + 1;
    for more symbols the longest code that can still be split is, so the short codes stay"""
    assert maxlen + 1 <= nsym <= 1 << maxlen
    lens = list(range(1, maxlen + 1)) + [maxlen]
    while len(lens) < nsym:
        i = max(k for k, n in enumerate(lens) if n < maxlen and (k + 1 == len(lens) or lens[k + 1] > n))
        lens[i:i + 1] = [lens[i] + 1, lens[i] + 1]
        lens.sort()
    assert kraft(lens) == 32768 and max(lens) == maxlen
    return lens


def spread(nsym, assign):
    """a length list of nsym entries from {symbol: length}"""
    lens = [0] * nsym
    for s, n in assign.items():
        lens[s] = n
    return lens


def length_symbol(length):
    return max(i for i in range(29) if LBASE[i] <= length and (i == 28 or length < 258))


def distance_symbol(dist):
    return max(i for i in range(30) if DBASE[i] <= dist)


def apply_tokens(tokens, text=b""):
    """the text the tokens give behind `text` (the reference the writer's own output is checked against is zlib, not this)"""
    out = bytearray(text)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] != "bits":
            length, dist = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= dist <= len(out)
            src = bytes(out[len(out) - dist:])
            out += (src * (length // dist + 1))[:length]
    return bytes(out)


def write_tokens(w, tokens, lit, dist, eob=True):
    """lit / dist: symbol -> (code, length)"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        else:
            ls = t[2] - 257 if len(t) > 2 else length_symbol(t[0])
            assert 0 <= t[0] - LBASE[ls] < 1 << LEXT[ls] or (ls == 28 and t[0] == 258)
            w.code(*lit[257 + ls])
            w.bits(t[0] - LBASE[ls], LEXT[ls])
            ds = distance_symbol(t[1])
            w.code(*dist[ds])
            w.bits(t[1] - DBASE[ds], DEXT[ds])
    if eob:
        w.code(*lit[256])


FIXED_LIT = canonical_codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical_codes([5] * 32)


def fixed_block(w, tokens, final, eob=True):
    w.bits(final, 1); w.bits(1, 2)
    write_tokens(w, tokens, FIXED_LIT, FIXED_DIST, eob)


def stored_block(w, data, final, length=None, nlen=None):
    """LEN is `length` if given (then the caller answers for the bytes that follow), NLEN its complement unless given"""
    n = len(data) if length is None else length
    w.bits(final, 1); w.bits(0, 2); w.align()
    w.bits(n, 16); w.bits(n ^ 0xFFFF if nlen is None else nlen, 16)
    w.out += data


def plain_ops(lens):
    return [(n, 0) for n in lens]


def rle_ops(lens):
    """the lengths with runs folded the usual way: 18 / 17 for zeros, 16 for repeats"""
    ops, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]:
            j += 1
        run, v = j - i, lens[i]
        if v:
            ops.append((v, 0)); run -= 1
        while run >= 3:
            r = min(run, 138 if v == 0 else 6)
            if v == 0 and r <= 10:
                ops.append((17, r - 3))
            elif v == 0:
                ops.append((18, r - 11))
            else:
                ops.append((16, r - 3))
            run -= r
        ops += [(v, 0)] * run
        i = j
    return ops


def ops_lengths(ops):
    """what a decoder makes of the ops"""
    out = []
    for s, x in ops:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out


def dynamic_block(w, lit_lens, dist_lens, tokens, final, ops=None, nc=None, cl_lens=None, hlit=None, hdist=None, eob=True, stop=None):
    """one dynamic block.  ops: the code length stream as (symbol, extra) pairs instead of one op per length; nc: 19 forces all
    HCLEN triples, None trims trailing zeros; cl_lens: the 19 code length code lengths instead of a complete set over the symbols the
    ops use; hlit / hdist: the header fields instead of len(lens) - 257 / - 1; stop: 'hclen' / 'ops' ends the block there."""
    if ops is None:
        ops = plain_ops(list(lit_lens) + list(dist_lens))
    if cl_lens is None:
        used = sorted({s for s, _ in ops})
        if len(used) < 2:
            used = sorted(set(used) | {0, 18})[:2]
        m = 1
        while (1 << m) < len(used):
            m += 1
        cl = sorted(complete_lengths(len(used), max(m, min(7, len(used) - 1))))
        cl_lens = spread(19, dict(zip(used, cl)))
    if nc is None:
        nc = max([4] + [i + 1 for i, s in enumerate(CLORDER) if cl_lens[s]])
    w.bits(final, 1); w.bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
    w.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
    w.bits(nc - 4, 4)
    for s in CLORDER[:nc]:
        w.bits(cl_lens[s], 3)
    if stop == "hclen":
        return
    cl = canonical_codes(cl_lens)
    for s, x in ops:
        w.code(*cl[s])
        if s >= 16:
            w.bits(x, {16: 2, 17: 3, 18: 7}[s])
    if stop == "ops":
        return
    write_tokens(w, tokens, canonical_codes(lit_lens), canonical_codes(dist_lens), eob)


# ---- a reader for the headers: what a test claims about a stream is read back from its bits -----------------------------------------
class BitReader:
    def __init__(self, raw, pos=0):
        self.raw, self.pos = raw, pos

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= (self.raw[self.pos >> 3] >> (self.pos & 7) & 1) << i
            self.pos += 1
        return v

    def symbol(self, codes):
        """codes: (code, length) -> symbol"""
        c = 0
        for n in range(1, 16):
            c = c << 1 | self.bits(1)
            if (c, n) in codes:
                return codes[(c, n)]
        raise ValueError("no such code")


def parse_block_header(raw, pos=0):
    """the deflate block that starts at bit `pos`: dict with final, type and, for a dynamic block, nl, nd, nc, cl_lens, ops (each
    with the index it starts at), lit_lens, dist_lens and `pos`, the bit the tokens start at"""
    r = BitReader(raw, pos)
    h = {"final": r.bits(1), "type": r.bits(2)}
    if h["type"] != 2:
        return h
    nl, nd, nc = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
    cl_lens = [0] * 19
    for s in CLORDER[:nc]:
        cl_lens[s] = r.bits(3)
    codes = {v: s for s, v in canonical_codes(cl_lens).items()}
    lens, ops = [], []
    while len(lens) < nl + nd:
        s = r.symbol(codes)
        x = r.bits({16: 2, 17: 3, 18: 7}[s]) if s >= 16 else 0
        ops.append((s, x, len(lens)))
        lens += [lens[-1]] * (3 + x) if s == 16 else ops_lengths([(s, x)])
    assert len(lens) == nl + nd
    h.update(nl=nl, nd=nd, nc=nc, cl_lens=cl_lens, ops=ops, lit_lens=lens[:nl], dist_lens=lens[nl:], pos=r.pos)
    return h


# ---- hand-made streams: the cases of tests/test_bgzf_host.py (against zlib) and tests/test_gpu_bgzf.py (against the kernel) ----------
def used_symbols(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif t[0] != "bits":
            lit.add(t[2] if len(t) > 2 else 257 + length_symbol(t[0]))
            dist.add(distance_symbol(t[1]))
    return lit, dist


def fit_lengths(nsym, used, maxlen, flip=False):
    """a complete set over the used symbols (a second symbol joins a single one), the shortest code on the lowest symbol"""
    used = sorted(used)
    if len(used) == 1:
        used = sorted(used + [used[0] + 1 if used[0] + 1 < nsym else used[0] - 1])
    m = 1
    while (1 << m) < len(used):
        m += 1
    lens = complete_lengths(len(used), max(m, min(maxlen, len(used) - 1)))
    return spread(nsym, dict(zip(used, lens[::-1] if flip else lens)))


def dynamic_for(w, tokens, final, maxlen=15, flip=False, **kw):
    """a dynamic block with sets made for its tokens"""
    lit, dist = used_symbols(tokens)
    lit_lens = fit_lengths(286, lit, maxlen, flip)
    dist_lens = fit_lengths(30, dist, maxlen, flip) if dist else [0]
    while len(lit_lens) > 257 and not lit_lens[-1]:
        lit_lens.pop()
    while len(dist_lens) > 1 and not dist_lens[-1]:
        dist_lens.pop()
    dynamic_block(w, lit_lens, dist_lens, tokens, final, **kw)


def chain_case(maxl, maxd, seed, flip=False):
    """-> (lit_lens, dist_lens, tokens): both sets are 1, 2, ..., max, max; the tokens decode a literal or length symbol and a
    distance symbol at every code length, in 3-4 KB of text"""
    rs = np.random.RandomState(seed)
    lsyms = [257, 265, 273, 281, 284, 285][-(6 if maxl >= 13 else 5):]
    lits = list(b"ACGTN\n@+I"[:maxl - len(lsyms)])
    order = lits + lsyms + [256]
    ll = complete_lengths(maxl + 1, maxl)
    lit_lens = spread(286, dict(zip(order, ll[::-1] if flip else ll)))
    dsyms = sorted({round(i * 23 / maxd) for i in range(maxd + 1)})
    assert len(dsyms) == maxd + 1
    dl = complete_lengths(maxd + 1, maxd)
    dist_lens = spread(24, dict(zip(dsyms, dl[::-1] if flip else dl)))
    tokens, pos = list(lits), len(lits)
    for _ in range(80):
        tokens.append(lits[rs.randint(len(lits))]); pos += 1

    def match(ls, ds):
        nonlocal pos
        length = LBASE[ls - 257] + rs.randint(1 << LEXT[ls - 257]) if ls != 285 else 258
        dist = min(pos, DBASE[ds] + rs.randint(1 << DEXT[ds]))
        assert distance_symbol(dist) == ds
        tokens.append((length, dist, ls)); pos += length
        tokens.append(lits[rs.randint(len(lits))]); pos += 1
    for i, ds in enumerate(dsyms):
        while pos < DBASE[ds]:
            match(285, dsyms[i - 1])
        match(lsyms[i % len(lsyms)], ds)
    for ls in lsyms:
        match(ls, dsyms[rs.randint(len(dsyms))])
    return lit_lens, dist_lens, tokens


def one_block_member(tokens, writer, **kw):
    w = BitWriter()
    writer(w, tokens, 1, **kw)
    return w.done(), apply_tokens(tokens)


def legal_long_codes():
    """-> [(name, raw, text)]: code lengths 1..15 in both alphabets, and the two sides of each look-up table's edge"""
    out = []
    for name, maxl, maxd in (("long15", 15, 15), ("edge_in", 10, 8), ("edge_out", 11, 9)):
        for flip in (False, True):
            lit_lens, dist_lens, tokens = chain_case(maxl, maxd, maxl + flip, flip)
            w = BitWriter()
            dynamic_block(w, lit_lens, dist_lens, tokens, 1)
            out.append((name + "_flip" * flip, w.done(), apply_tokens(tokens)))
    return out


def legal_degenerate():
    """one member: a block without any distance code, a block of nothing but the end-of-block symbol (its set: the single code of
    length 1), a block whose one distance code has length 1; and the same three as members of their own"""
    lits = [b"ACGT\n"[i % 5] for i in range(300)]
    ones = []
    for i in range(40):
        ones += [b"ACGTN"[i % 5], (3 + 7 * i % 256, 1)]
    only_eob = spread(257, {256: 1})
    blocks = [lambda w, f: dynamic_block(w, fit_lengths(257, used_symbols(lits)[0], 15), [0], lits, f),
              lambda w, f: dynamic_block(w, only_eob, [0], [], f),
              lambda w, f: dynamic_block(w, fit_lengths(286, used_symbols(ones)[0], 15), [1], ones, f)]
    texts = [bytes(lits), b"", apply_tokens(ones)]
    out = []
    w = BitWriter()
    for i, b in enumerate(blocks):
        b(w, i == 2)
    out.append(("three_blocks", w.done(), b"".join(texts)))
    for name, b, t in zip(("no_distance_code", "only_end_of_block", "one_distance_code"), blocks, texts):
        w = BitWriter()
        b(w, 1)
        out.append((name, w.done(), t))
    return out


def legal_header_ops():
    """-> [(name, raw, text, claim)]: claim(header) is what the name says, read back from the stream's bits"""
    out = []

    def add(name, lit_lens, dist_lens, tokens, claim, **kw):
        w = BitWriter()
        dynamic_block(w, lit_lens, dist_lens, tokens, 1, **kw)
        out.append((name, w.done(), apply_tokens(tokens), claim))
    body = [65, 65, 65, (3, 1), 65, (4, 2), 65, (5, 3), (3, 4), 65]
    # 16 from nl - 2 into the distance lengths: symbols 257..259 and distances 1..4 all have length 2
    lit = spread(260, {65: 3, 256: 3, 257: 2, 258: 2, 259: 2})
    ops = plain_ops(lit[:258]) + [(16, 3)]
    add("rep16_across", lit, [2, 2, 2, 2], body, lambda h: h["ops"][-1] == (16, 3, h["nl"] - 2) and h["nd"] == 4, ops=ops)
    # 18: zeros from symbol 258 to distance symbol 9; distance symbols 10 and 11 (33..64) have one bit each
    lit = spread(286, {65: 2, 66: 2, 256: 2, 257: 2})
    far = [65, 66] * 40 + [(3, 33), 66, (3, 49), (3, 64), 65]
    ops = plain_ops(lit[:258]) + [(18, 28 + 10 - 11), (1, 0), (1, 0)]
    add("rep18_across", lit, [0] * 10 + [1, 1], far, lambda h: h["ops"][-3] == (18, 27, 258) and h["nl"] == 286, ops=ops)
    # 17: zeros over symbols 258, 259 and distance symbols 0..3; distance symbols 4 and 5 (5..8) have one bit each
    lit = spread(260, {65: 2, 66: 2, 256: 2, 257: 2})
    mid = [65, 66] * 5 + [(3, 5), 66, (3, 8), (3, 7), 65]
    ops = plain_ops(lit[:258]) + [(17, 3), (1, 0), (1, 0)]
    add("rep17_across", lit, [0, 0, 0, 0, 1, 1], mid, lambda h: h["ops"][-3] == (17, 3, 258) and h["nl"] == 260, ops=ops)
    # 16 behind 17: it repeats the zero.  Symbols 0..9 by 17, 10..15 by 16, then the rest one by one
    lit = spread(260, {65: 2, 66: 2, 256: 2, 257: 2})
    ops = [(17, 7), (16, 3)] + plain_ops(lit[16:] + [1, 1])
    add("rep16_after_17", lit, [1, 1], [65, 66, 65, (3, 2), (3, 1)], lambda h: h["ops"][:2] == [(17, 7, 0), (16, 3, 10)], ops=ops)
    # every one of the 286 + 30 lengths non-zero
    lit, dist = complete_lengths(286, 15), complete_lengths(30, 15)[::-1]
    rs = np.random.RandomState(3)
    full = [int(x) for x in rs.randint(0, 256, 700)]
    for i in range(29):
        full += [(LBASE[i] + LEXT[i], 1 + 23 * i)] + [int(x) for x in rs.randint(0, 256, 3)]
    add("all_316_lengths", lit, dist, full, lambda h: h["nl"] == 286 and h["nd"] == 30 and 0 not in h["lit_lens"] + h["dist_lens"])
    # all 19 HCLEN triples although the last ones are zero; and the fewest a legal block can have: 4 reach only 16, 17, 18 and 0,
    # which spell nothing but zeros, the fifth is 8 -- 256 symbols of 8 bits are a complete set
    lit = spread(286, {65: 1, 66: 2, 256: 3, 257: 3})
    add("hclen19", lit, [1, 1], [65, 66, 65, (3, 2), (3, 1)], lambda h: h["nc"] == 19 and h["cl_lens"][15] == 0, nc=19, ops=rle_ops(lit + [1, 1]))
    lit = [8] * 10 + [0] + [8] * 246
    add("hclen5", lit, [0], bytes_without(10, 400), lambda h: h["nc"] == 5, cl_lens=spread(19, {0: 1, 8: 1}))
    return out


def bytes_without(byte, n):
    return [int(x) + (int(x) >= byte) for x in np.random.RandomState(9).randint(0, 255, n)]


def legal_length_258():
    """258 as symbol 285, and as symbol 284 with extra bits 31, in fixed and in dynamic blocks"""
    out = []
    for name, sym in (("len258_as_285", 285), ("len258_as_284", 284)):
        tokens = [71, 65, 84, (258, 3, sym), 67, (258, 1, sym), (258, 200, sym), (227, 5, 284), (257, 7, 284)]
        for kind, writer in (("fixed", fixed_block), ("dynamic", dynamic_for)):
            out.append((name + "_" + kind,) + one_block_member(tokens, writer))
    return out


def legal_literal_runs():
    """runs of 63..129 literals (the kernel keeps up to 64 pending), each followed at once by a match"""
    out = []
    rs = np.random.RandomState(21)
    for run in (63, 64, 65, 127, 128, 129):
        for k, kind in enumerate(("dist1", "dist_run", "dist_pos", "ends_at_isize")):
            tokens = [120, 121, 122, 123, 124, (4, 5)] + [int(x) for x in rs.randint(0, 256, run)]
            pos = 9 + run
            tokens.append({"dist1": (70, 1), "dist_run": (run, run), "dist_pos": (pos + 5 if pos + 5 <= 258 else 258, pos),
                           "ends_at_isize": (run + 9, run - 1)}[kind])
            if kind != "ends_at_isize":
                tokens += [int(x) for x in rs.randint(0, 256, 70)] + [(3, 1)]
            writer = fixed_block if (run + k) % 2 else dynamic_for
            out.append(("run%d_%s" % (run, kind),) + one_block_member(tokens, writer))
    return out


def hand_literals(data, maxlen, seed):
    """all 256 byte values and the end-of-block symbol in one dynamic block: a flat set (255 codes of 8 bits, two of 9) or, for
    maxlen 15, lengths 1..15 dealt out at random"""
    lens = [8] * 255 + [9, 9] if maxlen == 9 else complete_lengths(257, maxlen)
    np.random.RandomState(seed).shuffle(lens)
    w = BitWriter()
    dynamic_block(w, lens, [0], list(data), 1, ops=rle_ops(lens + [0]))
    return w.done()


def first_block_type(raw):
    return parse_block_header(raw)["type"]


def legal_random(random):
    """random bytes through Huffman tables: zlib's own stream where its first block is dynamic, else the hand writer's"""
    out = []
    for name, data, strategy, level, maxlen in (("huffman_only", random[:60000], zlib.Z_HUFFMAN_ONLY, 6, 9),
                                                ("filtered9", random[:60000], zlib.Z_FILTERED, 9, 9),
                                                ("long_codes", random[:20000], None, 0, 15)):
        raw = deflate_raw(data, level, strategy) if strategy is not None else b"\0"
        if first_block_type(raw) != 2:
            raw = hand_literals(data, maxlen, len(name))
        out.append((name, raw, data))
    return out


# the window sweep: [fixed block: 67 literals, then matches of distance 67 up to 25 KB of text, in ~300 bytes] [stored block of n
# bytes] [dynamic block: k literals of one bit, then tokens of 15 + 5 + 15 + 13 bits].  A distance with 13 extra bits lies at least
# 16385 back, so the text in front of it cannot come from the stored block alone.
SWEEP_LIT = spread(285, dict(zip([65, 67, 71, 84, 10, 78, 64, 43, 73, 257, 265, 273, 281, 283, 284, 256], complete_lengths(16, 15))))
SWEEP_DIST = spread(29, dict(zip([0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 27, 28], complete_lengths(16, 15))))
SWEEP_MAX = [(227 + 31, 16385 + 0x1FFF, 284), (227 + 10, 16385 + 0x0AAA, 284), (227 + 21, 16385 + 0x1555, 284), (227, 16385, 284),
             (227 + 17, 16385 + 4097, 284), (227 + 30, 16385 + 1, 284)]
assert SWEEP_LIT[284] == 15 and SWEEP_DIST[28] == 15


def sweep_prefix():
    rs = np.random.RandomState(67)
    tokens = [int(x) for x in rs.randint(0, 256, 67)] + [(258, 67)] * 97
    w = BitWriter()
    fixed_block(w, tokens, 0)
    return w, apply_tokens(tokens)


def sweep_member(prefix, at_bit, stored, extra):
    """the member whose first maximal token starts `at_bit` bits behind the payload's first byte -> (member, text, the bit found)"""
    w0, text0 = prefix
    w = BitWriter()
    w.acc, w.n, w.out = w0.acc, w0.n, bytearray(w0.out)
    t = BitWriter()
    dynamic_block(t, SWEEP_LIT, SWEEP_DIST, [], 0, ops=rle_ops(SWEEP_LIT + SWEEP_DIST), stop="ops")
    head = 8 * len(t.out) + t.n                       # the dynamic block starts on a byte: behind the stored bytes
    start = 8 * (len(w.out) + (1 if w.n <= 5 else 2) + 4)  # the stored block's bytes start here
    k = (at_bit - start - head) % 8
    n = (at_bit - start - head - k) // 8
    assert 0 <= n <= len(stored)
    stored_block(w, stored[:n], 0)
    assert 8 * len(w.out) + w.n == start + 8 * n
    tokens = [65] * k + SWEEP_MAX + [67, 10]
    dynamic_block(w, SWEEP_LIT, SWEEP_DIST, [], 1, ops=rle_ops(SWEEP_LIT + SWEEP_DIST), stop="ops")
    found = 8 * len(w.out) + w.n + k
    write_tokens(w, tokens, canonical_codes(SWEEP_LIT), canonical_codes(SWEEP_DIST))
    text = apply_tokens(tokens, text0 + stored[:n])
    raw = w.done()
    assert parse_block_header(raw, start + 8 * n)["pos"] + k == found  # read back from the bits: the header ends where the writer says
    sub = b"XY" + struct.pack("<H", extra) + bytes(range(extra))
    return member_raw(raw, text, sub), text, found


def sweep_file(random, offsets=range(-40, 41), boundaries=(1024, 2048), passes=2):
    """-> (file, text, phases): every member's first maximal token placed by its offset from a window boundary, the window counted
    from the payload's address rounded down to 16; phases = per member (boundary, offset in bits, pay_off, in_off), measured"""
    prefix = sweep_prefix()
    dummy = b"odd\n" * 5 + b"x"
    f, text, phases, i = member(dummy, 6), dummy, [], 0
    assert len(f) % 2 == 1
    for p in range(passes):
        for bnd in boundaries:
            for off in offsets:
                extra = (i * 7 + p * 5) % 16
                pay_off = 18 + 4 + extra
                shift = (len(f) + pay_off) % 16
                m, t, found = sweep_member(prefix, 8 * (bnd - shift) + off, random[i:i + 2000], extra)
                phases.append((bnd, 8 * shift + found - 8 * bnd, pay_off, len(f)))
                f += m; text += t; i += 1
    return f + EOF_MARKER, text, phases


def assert_sweep_phases(phases, offsets=range(-40, 41), boundaries=(1024, 2048)):
    """every bit offset at every boundary, every residue of pay_off and of the payload's address, several of in_off"""
    assert {(b, o) for b, o, _, _ in phases} == {(b, o) for b in boundaries for o in offsets}
    assert {p % 16 for _, _, p, _ in phases} == set(range(16))
    assert {(p + i) % 16 for _, _, p, i in phases} == set(range(16))
    assert len({i % 16 for _, _, _, i in phases}) >= 4 and any(i % 2 for _, _, _, i in phases)


# ---- malformed streams -----------------------------------------------------------------------------------------------------------------
def illegal_cases():
    """-> [(name, member, raw, level, classes)]: level 'stream': zlib refuses raw; level 'member': raw is a good stream and the
    member's ISIZE is wrong.  classes: the MK_INFL_* names include/metakssd_hip.h documents for the case."""
    out = []
    lit0 = spread(286, {65: 2, 66: 2, 256: 2, 257: 2})
    body = [65, 66, 65, (3, 2), (3, 1)]

    def add(name, classes, build, text=b"", level="stream"):
        w = BitWriter()
        build(w)
        raw = w.done()
        out.append((name, member_raw(raw, text), raw, level, classes))

    def dyn(lit=lit0, dist=(1, 1), tokens=body, **kw):
        return lambda w: dynamic_block(w, list(lit), list(dist), tokens, 1, **kw)
    code, lens, dista, inp = ("BAD_CODE",), ("BAD_LENGTHS",), ("BAD_DISTANCE",), ("INPUT", "BAD_CODE", "BAD_LENGTHS", "BAD_DISTANCE", "OUTPUT_LEN")
    add("lit_oversubscribed", code, dyn(lit=spread(286, {65: 1, 66: 1, 256: 1, 257: 2})))
    add("lit_oversubscribed_by_one_15_bit_code", code, dyn(lit=spread(286, dict(list(zip(range(100, 117), complete_lengths(17, 15))) + [(256, 15)])),
                                                          tokens=[]))
    add("dist_oversubscribed", code, dyn(dist=(1, 1, 1)))
    add("codelen_oversubscribed", code, dyn(cl_lens=spread(19, {0: 1, 1: 1, 2: 1})))
    add("lit_incomplete_two_codes", code, dyn(lit=spread(286, {65: 2, 256: 2}), tokens=[65, 65]))
    add("lit_incomplete_one_code_of_two_bits", code, dyn(lit=spread(257, {256: 2}), dist=(0,), tokens=[]))
    add("dist_incomplete_two_codes", code, dyn(dist=(2, 2)))
    add("dist_incomplete_one_code_of_two_bits", code, dyn(dist=(2,), tokens=[65, 66, 65]))
    add("codelen_incomplete", code, dyn(cl_lens=spread(19, {0: 1, 1: 2, 2: 3})))
    add("codelen_single_code", code, dyn(lit=spread(257, {}), dist=(0,), tokens=[], eob=False, cl_lens=spread(19, {0: 1}),
                                         ops=[(0, 0)] * 258))
    add("dist_single_code_other_bit", code, lambda w: (dynamic_block(w, lit0, [1], [65, 66, 65], 0, eob=False),
                                                     w.code(*canonical_codes(lit0)[257]), w.bits(1, 1)))
    add("dist_no_code_but_a_match", code, lambda w: (dynamic_block(w, lit0, [0], [65, 66, 65], 0, eob=False),
                                                   w.code(*canonical_codes(lit0)[257]), w.bits(0, 8)))
    add("no_end_of_block_code", lens, dyn(lit=spread(286, {65: 1, 66: 2, 257: 2}), eob=False))
    add("rep16_first", lens, dyn(ops=[(16, 0)] + plain_ops(lit0[3:] + [1, 1])))
    add("run_overruns", lens, dyn(ops=plain_ops(lit0) + [(1, 0), (17, 0)]))
    add("run18_overruns_from_the_literals", lens, dyn(ops=plain_ops(lit0[:258]) + [(18, 127)]))
    add("hlit_287", lens, dyn(hlit=30))
    add("hlit_288", lens, dyn(hlit=31))
    add("hdist_31", lens, dyn(hdist=30))
    add("hdist_32", lens, dyn(hdist=31))
    add("hclen4_spells_only_zeros", lens, dyn(lit=[0] * 257, dist=(0,), tokens=[], eob=False, cl_lens=spread(19, {0: 1, 18: 1}),
                                              ops=[(18, 127), (18, 109)]))
    for s in (286, 287):
        add("fixed_length_symbol_%d" % s, code, lambda w, s=s: (fixed_block(w, [65, 66], 1, eob=False), fixed_symbol(w, s), w.bits(0, 16)))
    for d in (30, 31):
        add("fixed_distance_symbol_%d" % d, dista, lambda w, d=d: (fixed_block(w, [65] * 40, 1, eob=False), fixed_symbol(w, 257), w.code(d, 5),
                                                                  w.bits(0, 16)), b"A" * 43)
    far = lambda w: (w.code(*FIXED_LIT[257]), w.code(3, 5), w.code(*FIXED_LIT[256]))  # length 3, distance 4
    # (ISIZE is what the stream would give were the distance one smaller: nothing but the distance is wrong)
    add("distance_beyond_start_first_block", dista, lambda w: (fixed_block(w, [65, 66, 67], 1, eob=False), far(w)), b"ABCABC")
    add("distance_beyond_start_second_block", dista, lambda w: (stored_block(w, b"ACG", 0), fixed_block(w, [], 1, eob=False), far(w)), b"ACGACG")
    good = [65, 66, 67, 68, (10, 4), 69]
    text = apply_tokens(good)
    add("literal_overruns_isize", ("OUTPUT_LEN",), lambda w: fixed_block(w, good, 1), text[:-1], "member")
    add("match_overruns_isize", ("OUTPUT_LEN",), lambda w: dynamic_for(w, good[:-1], 1), text[:-2], "member")
    # the payload ends early; what the kernel then reads is the member's trailer and its neighbour
    lit_lens, dist_lens, tokens = chain_case(15, 15, 4)
    cut_text = apply_tokens(tokens)

    def cut(stop=None, upto=None, more=0):
        def build(w):
            if stop:
                dynamic_block(w, lit_lens, dist_lens, [], 1, stop=stop)
                keep = len(w.out) - (3 if stop == "hclen" else 40)
            else:
                dynamic_block(w, lit_lens, dist_lens, tokens[:upto], 1, eob=False)
                ls = 281
                w.code(*canonical_codes(lit_lens)[ls]); w.bits(9, 5)
                w.align()
                keep = len(w.out)
                if more:
                    w.code(*canonical_codes(dist_lens)[23]); w.bits(0, more)
                    w.align()
                    keep = len(w.out)
            w.n, w.acc = 0, 0
            del w.out[keep:]
        return build
    add("ends_in_hclen_triples", inp, cut("hclen"), cut_text)
    add("ends_in_code_length_stream", inp, cut("ops"), cut_text)
    add("ends_between_length_and_distance", inp, cut(upto=60), cut_text)
    add("ends_in_distance_extra_bits", inp, cut(upto=60, more=2), cut_text)
    return out


# ---- an encoder for whole texts: greedy matches, block types taking turns ----------------------------------------------------------------
def lz_tokens(data, start, end):
    """tokens for data[start:end]; matches may reach back to byte 0"""
    last, tokens, i = {}, [], 0
    for j in range(0, max(0, start - 3)):
        last[data[j:j + 4]] = j
    i = start
    while i < end:
        key = data[i:i + 4]
        j = last.get(key, -1)
        n = 0
        if j >= 0 and i + 4 <= end:
            while n < 258 and i + n < end and data[j + n] == data[i + n]:
                n += 1
        if n >= 4:
            tokens.append((n, i - j))
        else:
            tokens.append(data[i]); n = 1
        for q in range(i, i + n):
            last[data[q:q + 4]] = q
        i += n
    return tokens


def hand_member(data):
    """one member of a stored, a fixed and two dynamic blocks (long-code sets, the second with the long codes on the low
    symbols) -> (member, raw, the bit each block starts at)"""
    cuts = [0, len(data) // 7, len(data) // 3, 2 * len(data) // 3, len(data)]
    w, starts = BitWriter(), [0]
    here = lambda: starts.append(8 * len(w.out) + w.n)
    stored_block(w, data[:cuts[1]], 0); here()
    fixed_block(w, lz_tokens(data, cuts[1], cuts[2]), 0); here()
    dynamic_for(w, lz_tokens(data, cuts[2], cuts[3]), 0); here()
    t = lz_tokens(data, cuts[3], cuts[4])
    lit, dist = used_symbols(t)
    lit_lens, dist_lens = fit_lengths(286, lit, 15, flip=True), fit_lengths(30, dist or {0}, 15)
    dynamic_block(w, lit_lens, dist_lens, t, 1, ops=rle_ops(lit_lens + dist_lens))
    raw = w.done()
    return member_raw(raw, data), raw, starts


def hand_bgzf(data, payload=4096):
    return b"".join(hand_member(data[a:a + payload])[0] for a in range(0, len(data), payload)) + EOF_MARKER
