"""numpy restatement of `dist --byread` (reads2mco(), iseq2comem.c:88-214) and of `reverse` / `reverse -b`
(co_reverse2kmer() / co_rvs2kmer_byreads(), command_reverse.c:148-368), for tests/test_byread_model.py,
tests/test_gpu_byread.py and tools/bench_byread.py.

The byte walk: '\\n' and '\\r' are skipped without resetting the window; a '>' starts a record, skips to the end of its line and
resets the window; any other byte that is no base resets it.  Every full window whose canonical k-mer passes the .shuf test emits
drtuple >> comp_code_bits to component drtuple % component_num, in text order, repeats and key 0 kept.  combco.index.<c> holds,
for records 0..readn (record 0 = what precedes the first '>'), the cumulative count of the component's ids.

`reverse -b` prints, for read n = 1..readn, index[n] - index[n-1] ids per component FROM A CURSOR THAT STARTS AT THE BEGINNING of
the component's file: with a non-zero entry 0 the ids are shifted and the tail is never printed (reproduced, not repaired).
"""
import os
import struct

import numpy as np

COMPONENT_SZ = 8            # global_basic.h:35-37
MIN_SMP = 4096              # MIN_SUBCTX_DIM_SMP_SZ
PATHLEN = 256


class Params:
    """seq2co_global_var_initial(), iseq2comem.c:54-86"""

    def __init__(self, shuf_id, k, subk, drlevel, table):
        self.shuf_id, self.k, self.subk, self.drlevel = int(shuf_id), int(k), int(subk), int(drlevel)
        self.table = np.asarray(table, dtype=np.int64)
        assert self.table.size == 16 ** subk
        self.out = k - subk
        self.TL = 2 * k
        d = k - drlevel - COMPONENT_SZ
        self.component_num = 16 ** d if d > 0 else 1
        self.comp_code_bits = 4 * d if d > 0 else 0
        self.dim_start = 0
        self.dim_end = max(16 ** (subk - drlevel), MIN_SMP)
        self.domask = ((1 << (4 * subk)) - 1) << (2 * self.out)
        self.undomask = ((1 << (2 * self.out)) - 1) << (2 * (k + subk))

    @classmethod
    def from_shuf(cls, shuf):
        """shuf: metakssd_amd.capi.Shuf"""
        return cls(shuf.c.id, shuf.c.k, shuf.c.subk, shuf.c.drlevel, np.array(shuf.table))

    @classmethod
    def from_file(cls, path):
        b = open(path, "rb").read()
        sid, k, subk, drl = struct.unpack_from("<iiii", b, 0)
        return cls(sid, k, subk, drl, np.frombuffer(b, dtype="<i4", offset=16))


def base_stream(text):
    """the bytes the walk looks at, in order: line ends and header lines dropped, a header's '>' kept as one byte.
    ValueError when the text ends inside a '>' line (the reference gives up there)."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    if t.size == 0:
        return t
    nl = t == 10
    line = np.concatenate(([0], np.cumsum(nl)[:-1]))      # line number of every byte (a '\n' belongs to the line it ends)
    gt = np.nonzero(t == 62)[0]
    first = np.full(int(line[-1]) + 1, t.size, dtype=np.int64)  # the line's first '>'
    if gt.size:
        np.minimum.at(first, line[gt], gt)
    pos = np.arange(t.size)
    in_header = pos > first[line]
    if in_header[-1] and not nl[-1]:
        raise ValueError("the text ends inside a '>' line")
    if t[-1] == 62 and first[line[-1]] == t.size - 1:
        raise ValueError("the text ends inside a '>' line")
    keep = ~in_header & ~nl & (t != 13)
    return t[keep]


def emissions(text, P):
    """(drtuple uint64[n], record int64[n]) of every accepted window in text order, and readn"""
    s = base_stream(text)
    readn = int(np.count_nonzero(s == 62))
    if s.size < P.TL:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), readn
    u = s | 0x20
    isb = (u == 97) | (u == 99) | (u == 103) | (u == 116)
    code = np.zeros(s.size, np.uint64)
    code[u == 99] = 1
    code[u == 103] = 2
    code[u == 116] = 3
    n = s.size - P.TL + 1                                   # windows, window w = s[w .. w + TL - 1]
    bad = np.concatenate(([0], np.cumsum(~isb)))
    full = (bad[P.TL:] - bad[:n]) == 0
    w = np.nonzero(full)[0]
    fwd = np.zeros(w.size, np.uint64)
    rc = np.zeros(w.size, np.uint64)
    for j in range(P.TL):
        c = code[w + j]
        fwd = (fwd << np.uint64(2)) | c
        rc |= (c ^ np.uint64(3)) << np.uint64(2 * j)
    uni = np.minimum(fwd, rc)
    dim = ((uni & np.uint64(P.domask)) >> np.uint64(2 * P.out)).astype(np.int64)
    pf = P.table[dim]
    acc = (pf >= P.dim_start) & (pf < P.dim_end)
    uni, pf, w = uni[acc], pf[acc], w[acc]
    low = uni & np.uint64((1 << (2 * P.out)) - 1)
    dr = (((uni & np.uint64(P.undomask)) + (low << np.uint64(2 * P.TL - 4 * P.out))) >> np.uint64(4 * P.drlevel)) \
        + (pf - P.dim_start).astype(np.uint64)
    rec = np.cumsum(s == 62)[w + P.TL - 1]
    return dr, rec.astype(np.int64), readn


def byread(text, P):
    """-> (ids: list of uint32 arrays per component, index: list of uint64 arrays of readn + 1 entries per component)"""
    dr, rec, readn = emissions(text, P)
    comp = (dr % np.uint64(P.component_num)).astype(np.int64)
    ids, index = [], []
    for c in range(P.component_num):
        m = comp == c
        ids.append((dr[m] >> np.uint64(P.comp_code_bits)).astype(np.uint32))
        index.append(np.cumsum(np.bincount(rec[m], minlength=readn + 1)).astype(np.uint64))
    return ids, index


def stat_header(P, infile_num=1, all_ctx_ct=0, koc=0):
    """co_dstat_t, global_basic.h:116-126 (padding written as zero)"""
    return struct.pack("<IB3xiiiiQ", P.shuf_id & 0xFFFFFFFF, koc, 2 * P.k, 2 * P.drlevel, P.component_num, infile_num, all_ctx_ct)


def write_byread_dir(out, text, P, path_name):
    """the directory `dist --byread` leaves (the ctx_ct word as 0)"""
    os.makedirs(out, exist_ok=True)
    ids, index = byread(text, P)
    for c in range(P.component_num):
        ids[c].tofile(os.path.join(out, "combco.%d" % c))
        index[c].tofile(os.path.join(out, "combco.index.%d" % c))
    name = os.fsencode(path_name)
    with open(os.path.join(out, "cofiles.stat"), "wb") as f:
        f.write(stat_header(P) + struct.pack("<I", 0) + name + b"\0" * (PATHLEN - len(name)))


def parse_stat(path):
    b = open(path, "rb").read()
    shuf_id, koc = struct.unpack_from("<IB", b, 0)
    kmerlen, dim_rd_len, comp_num, infile_num, all_ctx = struct.unpack_from("<iiiiQ", b, 8)
    cts = list(struct.unpack_from("<%dI" % infile_num, b, 32))
    o = 32 + 4 * infile_num
    names = [b[o + PATHLEN * i: o + PATHLEN * (i + 1)].split(b"\0", 1)[0].decode() for i in range(infile_num)]
    return dict(shuf_id=shuf_id, koc=koc, kmerlen=kmerlen, dim_rd_len=dim_rd_len, comp_num=comp_num, infile_num=infile_num,
                all_ctx_ct=all_ctx, ctx_ct=cts, names=names)


# ---- reverse ----------------------------------------------------------------------------------------------------------------

def rev_table(P):
    """rev_shuf_arr (command_reverse.c:152-160); None when the table does not have exactly 4096 entries below 4096"""
    small = np.nonzero((P.table >= 0) & (P.table < MIN_SMP))[0]
    if small.size != MIN_SMP:
        return None
    rev = np.zeros(MIN_SMP, np.uint64)
    rev[P.table[small]] = small.astype(np.uint64)
    return rev


def unituples(ids, comp, P, rev=None):
    """core_reverse2unituple(), command_reverse.c:355-368"""
    rev = rev_table(P) if rev is None else rev
    u64 = np.uint64
    pf_bits, inner, hob = 4 * (P.subk - P.drlevel), 4 * P.subk, 2 * (P.k - P.subk)
    dr = (np.asarray(ids, dtype=np.uint64) << u64(P.comp_code_bits)) + u64(comp)
    ind = rev[(dr % u64(MIN_SMP)).astype(np.int64)]
    tup = ((dr >> u64(pf_bits)) << u64(inner)) + ind
    hom = ((1 << hob) - 1) << inner
    return (tup & u64((hom << hob) & 0xFFFFFFFFFFFFFFFF)) + ((tup & u64(hom)) >> u64(inner)) + ((tup & u64((1 << inner) - 1)) << u64(hob))


def kmer_lines(ids, comp, P, rev=None):
    """the text `reverse` prints for these ids: lines of 2k letters + '\\n', as bytes"""
    uni = unituples(ids, comp, P, rev)
    out = np.empty((uni.size, P.TL + 1), np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(P.TL):
        out[:, P.TL - 1 - i] = letters[(uni & np.uint64(3)).astype(np.int64)]
        uni = uni >> np.uint64(2)
    out[:, P.TL] = 10
    return out.tobytes()


def _load_dir(d, comp_num):
    ids = [np.fromfile(os.path.join(d, "combco.%d" % c), dtype="<u4") for c in range(comp_num)]
    index = [np.fromfile(os.path.join(d, "combco.index.%d" % c), dtype="<u8") for c in range(comp_num)]
    return ids, index


def reverse_byread(d, P):
    """stdout of `reverse -b <d>` (co_rvs2kmer_byreads(), command_reverse.c:148-232)"""
    st = parse_stat(os.path.join(d, "cofiles.stat"))
    ids, index = _load_dir(d, st["comp_num"])
    rev = rev_table(P)
    readn = index[0].size - 1
    cur = [0] * st["comp_num"]
    out = []
    for n in range(readn):
        out.append(b">read %d\n" % (n + 1))
        for c in range(st["comp_num"]):
            k = int(index[c][n + 1]) - int(index[c][n])
            out.append(kmer_lines(ids[c][cur[c]:cur[c] + k], c, P, rev))
            cur[c] += k
    return b"".join(out)


def reverse_dir(d, P):
    """files of `reverse -o outdir <d>` (co_reverse2kmer(), command_reverse.c:237-353): {file name: bytes}, one per sketch with
    a non-zero ctx_ct, named after the basename of the recorded path with ' ' -> '_'"""
    st = parse_stat(os.path.join(d, "cofiles.stat"))
    ids, index = _load_dir(d, st["comp_num"])
    rev = rev_table(P)
    out = {}
    for k in range(st["infile_num"]):
        if st["ctx_ct"][k] == 0:
            continue
        name = st["names"][k].rsplit("/", 1)[-1].replace(" ", "_")
        parts = [kmer_lines(ids[c][int(index[c][k]):int(index[c][k + 1])], c, P, rev) for c in range(st["comp_num"])]
        out[name] = b"".join(parts)[: st["ctx_ct"][k] * (P.TL + 1)]
    return out


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------

def random_fasta(rs, nrec, min_len, max_len, width=60, lower=0.0, n_rate=0.0, crlf=False, lead=0):
    """a FASTA text: `lead` bases in front of the first '>', nrec records of min_len..max_len bases in lines of `width`"""
    eol = b"\r\n" if crlf else b"\n"
    out = []

    def seq(n):
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, size=n)].copy()
        if lower:
            m = rs.random_sample(n) < lower
            a[m] |= 0x20
        if n_rate:
            a[rs.random_sample(n) < n_rate] = ord("N")
        b = a.tobytes()
        return eol.join(b[i:i + width] for i in range(0, n, width))
    if lead:
        out.append(seq(lead) + eol)
    for i in range(nrec):
        out.append(b">r%d some text" % i + eol)
        n = int(rs.randint(min_len, max_len + 1))
        if n:
            out.append(seq(n) + eol)
    return b"".join(out)


def synthetic_text():
    """the hand-built case of tests/golden/byread: bases in front of the first '>', CRLF, lower case, N runs, a '>' in the middle
    of a line, a record shorter than 2k, two headers in a row, no final newline (a few KB: no header near a 65 536-byte cut)"""
    rs = np.random.RandomState(77)

    def b(n):
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, size=n)].tobytes()
    parts = [b(70) + b"\n" + b(41) + b"\n",                          # record 0: in front of the first '>'
             b">one first\r\n" + b(60) + b"\r\n" + b(60) + b"\r\n" + b(17) + b"\r\n",
             b">two lower\n" + b(80).lower() + b"\n" + b(33) + b(30).lower() + b"\n",
             b">three N runs\n" + b(50) + b"NNNNN" + b(45) + b"\n" + b(20) + b"n" + b(64) + b"\n",
             b">four mid\n" + b(55) + b">not a header start of line" + b"\n" + b(58) + b"\n",
             b">five short\n" + b(9) + b"\n",
             b">six\n>seven after an empty record\n" + b(300) + b"\n",
             b">eight\n" + b(700) + b"\n" + b(123)]                  # no final newline
    return b"".join(parts)
