"""the wide k-mer cases (k 12-16): geometries, seeded inputs with PLANTED k-mers, and a numpy model of the accepted windows.

From k = 13 on the key needs more than 32 bits before the shift; with k - drlevel <= 9 every geometry but (12,6,3) is CLAMPED
(16^(subk-drlevel) < 4096: the 12-bit pf is ADDED onto outer-context bits the shift did not vacate, keys carry and collide by
design, oracle/kssd_oracle.c:86-90); subk 7 is the only way to k = 16.  Shared by tests/golden/make_golden_widek.py (runs the real
reference), tests/test_widek_golden.py (oracle, no GPU) and tests/test_gpu_widek.py.

Random text gives about 750 keys per 3 Mbases at subk 6, so the inputs plant k-mers: inner substrings d with table[d] < 4096 in
random outer halves, drawn until the k-mer is its own canonical form, half of them written as their reverse complement, joined by
random spacers of 0-40 bases.  The same rows serve as text rows (<= 150 bases), as a multi-record FASTA and as a FASTQ.
"""
import functools

import numpy as np

import byread_model as bm
import util_inputs as ui

# name -> (k, subk, drlevel, seed)
GEOMS = {
    "W12S6D6": (12, 6, 6, 1266),  # table 131 071: probe chains; 48-bit unituple; pf over 0 vacated bits
    "W12S5D5": (12, 5, 5, 1255),  # table 2 097 143; 1/256 accepted on random text
    "W12S4D4": (12, 4, 4, 1244),  # table 33 554 393; 1/16 accepted: additive pf overlap on almost every key
    "W13S6D5": (13, 6, 5, 1365),  # first k with key bits >= 48 after the shift; 4 vacated bits for 12 of pf
    "W14S6D6": (14, 6, 6, 1466),  # 56-bit unituple
    "W12S6D3": (12, 6, 3, 1263),  # 16 components; the only UNCLAMPED k >= 12: `reverse` gives the k-mers back
    "W15S6D6": (15, 6, 6, 1566),  # 16 components; the only k = 15 without subk 7
    "W16S7D7": (16, 7, 7, 1677),  # 16 components; 64-bit unituple, 1 GiB .shuf, 2^28 accept bits
}
LIGHT = ["W12S6D6", "W12S5D5", "W12S4D4", "W13S6D5", "W14S6D6"]
HEAVY = ["W12S6D3", "W15S6D6", "W16S7D7"]  # 536 870 909 slots: a 4.3 GB oracle table each
BYREAD = ["W12S6D3", "W13S6D5", "W16S7D7"]  # the geometries with reference-made by-read / reverse fixtures
SATURATE = "W12S6D6"                       # one planted k-mer 70 000 times: its count stops at 65 535
PLANTED = {"W12S6D6": 30000}               # load 0.2-0.46 of 131 071 slots; everywhere else:
PLANTED_DEFAULT = 3000
# the `dist` fixtures of every geometry: flavour -> (input kind, flags)
FLAVOURS = {"fa": ("fa", []), "fa_u": ("fa", ["-u"]), "fq_A": ("fq", ["-A"]), "fq_n2Q53": ("fq", ["-n", "2", "-Q", "53"])}
TINY = b">tiny\nACGTAC\n"  # shorter than any 2k: a sketch without ids, for which `reverse` writes no file


def fixture_name(f):
    """the name a file of a sketch directory has among the fixtures: the reference's 16-bit count files combco.N.a are kept as
    combco.N.a.u16, so that no fixture carries the suffix of a static library"""
    return f + ".u16" if f.endswith(".a") else f


MIN_KEYS = {n: (2000 if n in LIGHT else 300) for n in GEOMS}

_shufs = {}


def get_shuf(name):
    """the geometry's .shuf from the product's seeded generator, made once per process ((16,7,7): 1 GiB, some seconds)"""
    if name not in _shufs:
        from metakssd_amd import capi
        _shufs[name] = capi.Shuf.generate(*GEOMS[name])
    return _shufs[name]


def clamped(name):
    k, subk, drl, _ = GEOMS[name]
    return 16 ** (subk - drl) < bm.MIN_SMP


@functools.lru_cache(maxsize=None)
def params(name):
    """byread_model.Params of the geometry (holds an int64 copy of the table: 2 GiB at subk 7, made once)"""
    return bm.Params.from_shuf(get_shuf(name))


@functools.lru_cache(maxsize=None)
def rev_table(name):
    return bm.rev_table(params(name))


def _revcomp_u64(u, TL):
    """reverse complement of k-mers held in the low 2*TL bits of uint64"""
    out = np.zeros_like(u)
    for j in range(TL):
        out |= (((u >> np.uint64(2 * (TL - 1 - j))) & np.uint64(3)) ^ np.uint64(3)) << np.uint64(2 * j)
    return out


def _letters(u, TL):
    """uint64 k-mers -> (n, TL) uint8 matrix of ACGT"""
    out = np.empty((u.size, TL), np.uint8)
    for i in range(TL):
        out[:, TL - 1 - i] = ui.ACGT[((u >> np.uint64(2 * i)) & np.uint64(3)).astype(np.int64)]
    return out


def planted_unituples(rs, P, n):
    """n canonical k-mers (u < revcomp(u)) whose inner substring the .shuf accepts below 4096; first and last base from all four
    letters, so that top bits occur on both strands"""
    small = np.nonzero((P.table >= 0) & (P.table < bm.MIN_SMP))[0].astype(np.uint64)
    got = np.zeros(0, np.uint64)
    while got.size < n:
        m = 4 * (n - got.size) + 64
        d = small[rs.randint(0, small.size, size=m)]
        left = rs.randint(0, 1 << (2 * P.out), size=m).astype(np.uint64)
        right = rs.randint(0, 1 << (2 * P.out), size=m).astype(np.uint64)
        u = (left << np.uint64(2 * (P.k + P.subk))) | (d << np.uint64(2 * P.out)) | right
        got = np.concatenate((got, u[u < _revcomp_u64(u, P.TL)]))
    return got[:n]


def keys_of(P, uni, pf=None):
    """the keys of accepted canonical k-mers (uint64 unituples): the outer halves joined, shifted by the dimension reduction, plus
    the .shuf value pf of the inner substring (looked up when not given)"""
    if pf is None:
        pf = P.table[((uni & np.uint64(P.domask)) >> np.uint64(2 * P.out)).astype(np.int64)]
    low = uni & np.uint64((1 << (2 * P.out)) - 1)
    return (((uni & np.uint64(P.undomask)) + (low << np.uint64(2 * P.TL - 4 * P.out))) >> np.uint64(4 * P.drlevel)) + pf.astype(np.uint64)


def colliding_partners(rs, P, uni):
    """for canonical accepted k-mers of a clamped geometry, DIFFERENT canonical accepted k-mers with the same key: another inner
    substring, whose pf differs by a multiple of 2^v (v = 4(subk - drlevel), the bits the shift vacated), and the outer context
    moved by the difference (key = (outer << v) + pf).  Random k-mers meet like this far too rarely in a 2^28 key space."""
    v = 4 * (P.subk - P.drlevel)
    rev = bm.rev_table(P)
    assert rev is not None and v < 12
    d = ((uni & np.uint64(P.domask)) >> np.uint64(2 * P.out)).astype(np.int64)
    pf = P.table[d]
    outer = ((uni >> np.uint64(2 * (P.k + P.subk))) << np.uint64(2 * P.out)).astype(np.int64) | (uni & np.uint64((1 << (2 * P.out)) - 1)).astype(np.int64)
    pf2 = (pf + (rs.randint(1, bm.MIN_SMP >> v, size=uni.size) << v)) % bm.MIN_SMP
    outer2 = outer + ((pf - pf2) >> v)
    ok = (outer2 >= 0) & (outer2 < (1 << (4 * P.out)))
    o2, d2 = outer2[ok].astype(np.uint64), rev[pf2[ok]]
    u2 = ((o2 >> np.uint64(2 * P.out)) << np.uint64(2 * (P.k + P.subk))) | (d2 << np.uint64(2 * P.out)) | (o2 & np.uint64((1 << (2 * P.out)) - 1))
    return u2[u2 < _revcomp_u64(u2, P.TL)]


class Input:
    """rows: every read / line (<= 150 bases); body: rows without the 70 000 repeats (one kept)"""

    def __init__(self, name):
        k, subk, drl, seed = GEOMS[name]
        P = params(name)
        rs = np.random.RandomState(seed * 7 + 1)
        TL = P.TL
        n = PLANTED.get(name, PLANTED_DEFAULT)
        uni = planted_unituples(rs, P, n)
        if clamped(name):
            uni = np.concatenate((uni, colliding_partners(rs, P, uni[:400])))
            n = uni.size
        again = uni[rs.randint(0, n, size=n * 3 // 10)]       # some k-mers a second time: counts above 1, -n 2 keeps something
        often = np.repeat(uni[rs.randint(0, n, size=100)], 16)  # and a hundred of them sixteen times: -n 7 keeps some, also behind -Q 53
        order = np.concatenate((uni, again, often))
        order = order[rs.permutation(order.size)]
        flip = rs.rand(order.size) < 0.5                      # half of them as their reverse complement
        mat = _letters(np.where(flip, _revcomp_u64(order, TL), order), TL)
        kmers = [mat[i].tobytes() for i in range(order.size)]
        gaps = rs.randint(0, 41, size=order.size)
        filler = ui.rand_seq(rs, int(gaps.sum()) + 64)
        rows, cur, at = [], b"", 0
        for km, g in zip(kmers, gaps):
            sp = filler[at:at + int(g)]
            at += int(g)
            if len(cur) + len(sp) + TL > 150:
                rows.append(cur)
                cur = km
            else:
                cur += sp + km
        rows.append(cur)
        rows = [r.lower() if i % 5 == 3 else r for i, r in enumerate(rows)]
        x = kmers[0]
        edge = [x[:-1], x, x + b"G"]                                                      # 2k-1, 2k, 2k+1 bases
        fl = ui.rand_seq(rs, 20)
        edge += [fl[:10] + x[:i] + b"N" + x[i + 1:] + fl[10:] for i in range(TL)]         # an N at each of the 2k positions
        edge += [b"A" * 150, b"C" * 150, b"G" * 150, b"T" * 150, b"AC" * 75, kmers[1].lower() + b"n" + kmers[2]]
        self.name, self.P = name, P
        self.planted = uni
        self.body = edge[:3] + rows[:len(rows) // 2] + edge[3:] + rows[len(rows) // 2:] + [x]
        self.rows = self.body + ([x] * 69999 if name == SATURATE else [])
        self.quals = ui.random_quals(np.random.RandomState(seed * 7 + 2), self.rows)

    def row_array(self, stride):
        return ui.rows_from_seqs(self.rows, stride)

    @staticmethod
    def _records(rows):
        return [b">rec%d wide k\n" % (i // 40) + b"\n".join(rows[i:i + 40]) + b"\n" for i in range(0, len(rows), 40)]

    @functools.lru_cache(maxsize=None)
    def fasta(self):
        """records of 40 rows, one row per line (windows also run across the line ends inside a record)"""
        return b"".join(self._records(self.rows))

    def fasta_files(self, n=6):
        """the FASTA text without the 70 000 repeats, cut at header lines into n files of growing sizes"""
        recs = self._records(self.body)
        cuts = [len(recs) * (i * i + i) // (n * n + n) for i in range(n + 1)]
        assert all(a < b for a, b in zip(cuts, cuts[1:]))
        return [b"".join(recs[cuts[i]:cuts[i + 1]]) for i in range(n)]

    @functools.lru_cache(maxsize=None)
    def fastq(self):
        return ui.fastq_bytes(self.rows, quals=self.quals)

    @functools.lru_cache(maxsize=None)
    def model(self):
        """the accepted windows of the rows, each row walked alone (what -A and push_reads see): dict of
        keys (distinct, sorted), top_bit (accepted unituples with bit 4k-1 set), fwd_canonical / rc_canonical (accepted windows whose
        text is / is not the canonical strand), collisions (distinct accepted unituples minus distinct keys)"""
        P = self.P
        s = np.frombuffer(b"N".join(self.body), dtype=np.uint8)
        u = s | 0x20
        isb = (u == 97) | (u == 99) | (u == 103) | (u == 116)
        code = np.zeros(s.size, np.uint64)
        code[u == 99], code[u == 103], code[u == 116] = 1, 2, 3
        n = s.size - P.TL + 1
        bad = np.concatenate(([0], np.cumsum(~isb)))
        w = np.nonzero((bad[P.TL:] - bad[:n]) == 0)[0]
        fwd, rc = np.zeros(w.size, np.uint64), np.zeros(w.size, np.uint64)
        for j in range(P.TL):
            c = code[w + j]
            fwd = (fwd << np.uint64(2)) | c
            rc |= (c ^ np.uint64(3)) << np.uint64(2 * j)
        uni = np.minimum(fwd, rc)
        pf = P.table[((uni & np.uint64(P.domask)) >> np.uint64(2 * P.out)).astype(np.int64)]
        acc = (pf >= P.dim_start) & (pf < P.dim_end)
        uni, pf, fwd, rc = uni[acc], pf[acc], fwd[acc], rc[acc]
        key = keys_of(P, uni, pf)
        du, dk = np.unique(uni), np.unique(key)
        return {"keys": dk, "top_bit": int(np.count_nonzero(du >> np.uint64(4 * P.k - 1))), "fwd_canonical": int(np.count_nonzero(fwd < rc)),
                "rc_canonical": int(np.count_nonzero(rc < fwd)), "collisions": int(du.size - dk.size)}


@functools.lru_cache(maxsize=None)
def get_input(name):
    return Input(name)


def sketch_keys(comps, P):
    """the keys of a sketch given as one uint32 id array per component: (id << comp_code_bits) + component, sorted"""
    parts = [(np.asarray(ids, dtype=np.uint64) << np.uint64(P.comp_code_bits)) + np.uint64(c) for c, ids in enumerate(comps)]
    return np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)


def beyond_44_bits(P):
    """the largest key a 44-bit unituple (k = 11) could give in this geometry"""
    return ((1 << 44) >> (4 * P.drlevel)) + bm.MIN_SMP


def check_conditions(name, koc_ids, koc_counts, set_ids):
    """what the inputs were built for, asserted on a sketch of the rows (-A: ids and counts per component) and of the FASTA text
    (set: ids per component; None: not looked at).  Returns the counts the manifest records."""
    inp, P = get_input(name), params(name)
    m = inp.model()
    keys = sketch_keys(koc_ids, P)
    assert np.array_equal(keys, m["keys"]), "%s: the model's accepted keys are not the sketch's" % name
    nk = int(keys.size)
    ns = int(sum(len(x) for x in set_ids)) if set_ids is not None else nk
    lo, hi = (26000, 60000) if name == SATURATE else (MIN_KEYS[name], 1 << 62)
    assert lo <= nk <= hi and lo <= ns <= hi, (name, nk, ns)
    if P.k >= 13:
        assert m["top_bit"] > 0, name
        assert int(keys[-1]) > beyond_44_bits(P), name
    assert m["fwd_canonical"] > 0 and m["rc_canonical"] > 0, name
    cmax = max(int(c.max()) for c in koc_counts if len(c))
    assert cmax > 1 and (name != SATURATE or cmax == 65535), (name, cmax)
    if clamped(name):
        assert m["collisions"] > 0, name
    else:
        assert m["collisions"] == 0, name
    if name in HEAVY:
        assert P.component_num == 16 and all(len(x) > 0 for x in koc_ids) and all(len(x) > 0 for x in set_ids or []), name
    return {"distinct_keys_A": nk, "distinct_keys_fasta": ns, "planted": int(inp.planted.size), "top_bit_unituples": m["top_bit"],
            "keys_beyond_44_bit_unituple": int(np.count_nonzero(keys > np.uint64(beyond_44_bits(P)))),
            "fwd_canonical_windows": m["fwd_canonical"], "rc_canonical_windows": m["rc_canonical"], "max_count": cmax,
            "colliding_unituples": m["collisions"]}
