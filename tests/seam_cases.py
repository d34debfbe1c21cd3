"""inputs that pin the TUNED scan kernels (k 9, 10, 11 with subk 6; k 11 with subk 5) at every row pitch: ragged rows with a PLANTED
accepted k-mer ending at every column a column-block seam can touch.

mk_scan_kernel's tuned instantiations have no byte-wise path: whatever is not "150 clean bases" goes through pair body B and through
the state carried from one column block to the next (run, flo, hh, pa[], step / urun, done).  At drlevel 3 random text has one accepted
k-mer in 4 096, so random ragged rows put next to nothing beside a seam or behind an N.  Here every anchor -- an end position j of a
k-mer in the row -- gets its own canonical accepted k-mer (widek_cases.planted_unituples), written on a seeded strand, in seven rows
(a = j - TL + 1, Lmax = the most bases a row of the pitch holds, filler = seeded random ACGT):

  positive   a  filler + k-mer + filler to Lmax          b  row a in lower case          c  filler + k-mer, the newline right behind it
             d  N at a - 1, then the k-mer (a >= 1)      e  the k-mer, then N at j + 1 (j + 1 <= Lmax - 1)
  negative   f  filler + the first TL - 1 bases of the k-mer, the newline one base early
             g  row a with one base of the k-mer replaced by N

Anchors: every j in TL-1 .. Lmax-1 for pitches up to 528 (no seam can be missed whatever block width the launch picks); beyond,
TL-1 .. TL+15, Lmax-17 .. Lmax-1 and s-TL-8 .. s+TL+8 around the seams s (every multiple of 128; at pitch 4096: 128, 256, 2048, 3968).

The rows of a case lie in one array, in two orders behind one another:
  1  grouped by kind (all a, all b, ...; a kind with fewer than 64 rows is padded with row a of anchor 0): whole tiles of 64 live
     lanes pass every seam in body A, with hits at different columns.  Padded with row a of anchor 0 to a tile bound.
  2  one tile of 64 rows of kind a (anchors in seeded order), then ALL rows in a seeded shuffle, every ninth followed by an empty
     row, the last tile short of 64 rows: body B, lanes that are done, re-entry of in_step.
The expected -A count of a planted key is the number of positive rows of its anchor in the whole array, padding included.

Shared by tests/test_seam_cases.py (the oracle, no GPU), tests/test_gpu_seams.py and tests/golden/make_golden_seams.py (the real
reference on the FASTQ form of five of the inputs).  launch_plan() restates the geometry choice of mk_launch_scan_ex (mk_engine.hip)
so that the table beside test_gpu_seams.py's pitch list can be checked without a GPU.
"""
import functools
import json
import os

import numpy as np

import byread_model as bm
import util_inputs as ui
import widek_cases as wk
from conftest import SHUF_SPECS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seams")
GEOMS = {n: SHUF_SPECS[n] for n in ("L3K11", "L3K10", "L3K9", "L2K11")}  # the geometries with a tuned scan kernel
KINDS = "abcdefg"
POSITIVE = "abcde"
SEAMS = {4096: (128, 256, 2048, 3968)}  # pitch -> seams with anchors around them (default beyond 528: every multiple of 128)
RESEED = {}  # (geometry, pitch, lmax) -> extra seed word, should a planted key ever meet a stray key of the filler

# what the golden recipe runs the reference on: fixture name -> (geometry, pitch, lmax); the reference's fgets() takes lines of at
# most 4 094 characters whole (iseq2comem.c:656,673)
GOLDEN = {"L3K11_p272": ("L3K11", 272, None), "L3K10_p272": ("L3K10", 272, None), "L3K9_p272": ("L3K9", 272, None),
          "L2K11_p272": ("L2K11", 272, None), "L3K11_p4096": ("L3K11", 4096, 4094)}


@functools.lru_cache(maxsize=None)
def get_shuf(geom):
    from metakssd_amd import capi
    return capi.Shuf.generate(*GEOMS[geom])


@functools.lru_cache(maxsize=None)
def params(geom):
    return bm.Params.from_shuf(get_shuf(geom))


def anchors(pitch, TL, lmax=None):
    """the end positions j at which a k-mer is planted"""
    lmax = pitch - 1 if lmax is None else lmax
    lo, hi = TL - 1, lmax - 1
    if pitch <= 528:
        return list(range(lo, hi + 1))
    js = set(range(lo, TL + 16)) | set(range(lmax - 17, lmax))
    for s in SEAMS.get(pitch, range(128, pitch, 128)):
        js |= set(range(s - TL - 8, s + TL + 9))
    return sorted(j for j in js if lo <= j <= hi)


def launch_plan(pitch, offset=0, subk=6):
    """mk_launch_scan_ex for rows side by side of a tuned geometry (the shipped library: blocks of at most 128 bytes, 1024 threads
    wanted, one-pass staging on): column block CB, number of blocks, width of the last one, the instantiation's
    <VEC16, THREADS, NPIECES, ONEPASS> and whether it is a tuned one"""
    vec = pitch % 16 == 0 and offset % 16 == 0
    g = 16 if vec else (8 if pitch % 8 == 0 else 4)

    def width(n):
        return ((pitch + n - 1) // n + g - 1) // g * g
    ncb = (pitch + 127) // 128
    CB = width(ncb)
    if CB > 128:
        ncb += 1
        CB = width(ncb)
    ncb = (pitch + CB - 1) // CB
    ppr = CB // (16 if vec else 4)
    wave = ((64 * ((CB // 4) | 1) + 1) & ~1) + 2
    tuned = pitch % 8 == 0 and CB % 8 == 0
    mt = 256 if tuned and subk == 6 else 0
    fwords = 16384 if tuned else 1 << min(14, 4 * subk - 10)
    threads = 1024
    while True:
        lds = (mt + fwords + threads // 64 * wave) * 4 + (2 * (5 if ppr <= 5 else 8) * 64 * 4 if vec else 0)
        if lds <= 160 * 1024 or threads <= 512:
            break
        threads -= 256
    assert lds <= 160 * 1024
    onepass = vec and ncb == 2 and pitch == 2 * CB and ppr <= 5
    small = ppr <= (5 if vec else 20)
    npieces = (5 if small else 8) if vec else (20 if small else 32)
    return {"CB": CB, "ncb": ncb, "last": pitch - (ncb - 1) * CB, "vec16": vec, "threads": threads, "npieces": npieces,
            "onepass": onepass, "tuned": tuned}


class Case:
    """rows: the array (nrows * pitch bytes); seqs: the rows' texts; kinds / anchor_of: kind letter ('-' for an empty row) and anchor
    index (-1) of every row; second: the row the second order starts at; planted / flip / keys: per anchor the canonical k-mer,
    whether it is written as its reverse complement, its key; expected: key -> the -A count"""

    def __init__(self, geom, pitch, lmax=None):
        k, subk, drl, seed = GEOMS[geom]
        P = params(geom)
        TL = P.TL
        lmax = pitch - 1 if lmax is None else lmax
        assert TL <= lmax <= pitch - 1
        rs = np.random.RandomState([seed, pitch, lmax] + ([RESEED[(geom, pitch, lmax)]] if (geom, pitch, lmax) in RESEED else []))
        js = anchors(pitch, TL, lmax)
        n = len(js)
        # one canonical accepted k-mer per anchor, no two with the same key
        cand = wk.planted_unituples(rs, P, 2 * n + 64)
        _, first = np.unique(wk.keys_of(P, cand), return_index=True)
        uni = cand[np.sort(first)][:n]
        assert uni.size == n
        flip = rs.rand(n) < 0.5
        mat = wk._letters(np.where(flip, wk._revcomp_u64(uni, TL), uni), TL)

        def fill(m):
            return ui.ACGT[rs.randint(0, 4, size=m)]

        base = []  # (kind, anchor index, row text as uint8)
        for i, j in enumerate(js):
            a, km = j - TL + 1, mat[i]
            ra = np.concatenate((fill(a), km, fill(lmax - j - 1)))
            base.append(("a", i, ra))
            base.append(("b", i, ra | 0x20))
            base.append(("c", i, np.concatenate((fill(a), km))))
            if a >= 1:
                rd = np.concatenate((fill(a), km, fill(lmax - j - 1)))
                rd[a - 1] = ord("N")
                base.append(("d", i, rd))
            if j + 1 <= lmax - 1:
                re_ = np.concatenate((fill(a), km, fill(lmax - j - 1)))
                re_[j + 1] = ord("N")
                base.append(("e", i, re_))
            base.append(("f", i, np.concatenate((fill(a), km[:TL - 1]))))
            rg = ra.copy()
            rg[a + int(rs.randint(0, TL))] = ord("N")
            base.append(("g", i, rg))
        pad = ("a", 0, base[0][2])
        order = []
        for kind in KINDS:  # 1: grouped by kind
            grp = [r for r in base if r[0] == kind]
            order += grp + [pad] * max(0, 64 - len(grp))
        order += [pad] * (-len(order) % 64)
        self.second = len(order)
        a_rows = [r for r in base if r[0] == "a"]  # 2: a tile of kind a, then everything shuffled
        order += [a_rows[int(t)] for t in rs.randint(0, n, size=64)]
        empty = ("-", -1, np.zeros(0, np.uint8))
        for t, r in enumerate(rs.permutation(len(base))):
            order.append(base[int(r)])
            if t % 9 == 8:
                order.append(empty)
        if len(order) % 64 == 0:
            order.append(empty)
        nrows = len(order)
        M = np.zeros((nrows, pitch), np.uint8)
        for t, (_, _, r) in enumerate(order):
            M[t, :r.size] = r
            M[t, r.size] = 10
        self.geom, self.pitch, self.lmax, self.P, self.TL = geom, pitch, lmax, P, TL
        self.anchors, self.planted, self.flip = js, uni, flip
        self.keys = wk.keys_of(P, uni)
        self.rows, self.nrows = M.reshape(-1), nrows
        self.seqs = [r.tobytes() for _, _, r in order]
        self.kinds = np.array([r[0] for r in order])
        self.anchor_of = np.array([r[1] for r in order])
        pos = np.isin(self.kinds, list(POSITIVE))
        cnt = np.bincount(self.anchor_of[pos], minlength=n)
        self.expected = {int(key): int(c) for key, c in zip(self.keys, cnt)}

    def fastq(self):
        return ui.fastq_bytes(self.seqs)

    def tiles_of_kind_a(self):
        """tiles of 64 rows that are all of kind a: (in the first order, in the second)"""
        full = self.nrows // 64
        t = (self.kinds[:full * 64].reshape(full, 64) == "a").all(axis=1)
        return int(t[:self.second // 64].sum()), int(t[self.second // 64:].sum())

    def counts_of_planted(self, koc):
        """the counts a sketch ([(ids, counts)] per component) holds for the planted keys, in anchor order; 0 where a key is absent"""
        P = self.P
        out = []
        for key in self.keys:
            ids, cnt = koc[int(key) % P.component_num]
            at = np.nonzero(ids == np.uint32(int(key) >> P.comp_code_bits))[0]
            assert at.size <= 1
            out.append(int(cnt[at[0]]) if at.size else 0)
        return out


@functools.lru_cache(maxsize=4)
def _get_case(geom, pitch, lmax):
    return Case(geom, pitch, lmax)


def get_case(geom, pitch, lmax=None):
    """the case, rebuilt from its seeds when it is not one of the last four asked for"""
    return _get_case(geom, pitch, pitch - 1 if lmax is None else lmax)


# ---- the fixtures the compiled reference made (tests/golden/make_golden_seams.py) -------------------------------------------------
@functools.lru_cache(maxsize=None)
def manifest():
    return json.load(open(os.path.join(GOLD, "manifest.json")))


def load_dir(d, comp_num, suffix=""):
    """[(ids, counts)] per component of a sketch directory written with -A (suffix ".u16": the fixtures' name for combco.N.a)"""
    return [(np.fromfile(os.path.join(d, "combco.%d" % c), dtype="<u4"), np.fromfile(os.path.join(d, "combco.%d.a%s" % (c, suffix)), dtype="<u2"))
            for c in range(comp_num)]


def fixture(name):
    return load_dir(os.path.join(GOLD, name), manifest()["cases"][name]["stat"]["comp_num"], ".u16")


def check_conditions(case, koc):
    """what the inputs were built for, asserted on the oracle's sketch of the rows: every planted key with exactly its expected count, no two
    planted k-mers with one key, both strands, and in both orders a tile of 64 rows of kind a.  Returns what a manifest records."""
    tag = "%s pitch %d" % (case.geom, case.pitch)
    assert len(set(case.expected)) == len(case.anchors) == case.planted.size, tag
    assert np.unique(case.planted).size == case.planted.size, tag
    got = case.counts_of_planted(koc)
    want = [case.expected[int(k)] for k in case.keys]
    bad = [(j, g, w) for j, g, w in zip(case.anchors, got, want) if g != w]
    assert not bad, "%s: planted keys with another count (anchor, got, want): %s" % (tag, bad[:8])
    assert min(want) >= 8, tag  # four positive kinds at the least (d or e is missing at a row's two ends), in both orders
    assert case.flip.any() and not case.flip.all(), tag
    t1, t2 = case.tiles_of_kind_a()
    assert t1 >= 1 and t2 >= 1, tag
    assert case.nrows % 64 != 0 and (case.kinds == "-").sum() >= 1, tag
    return {"rows": case.nrows, "planted": len(case.anchors), "planted_counts": want, "distinct_keys": int(sum(len(c[0]) for c in koc))}
