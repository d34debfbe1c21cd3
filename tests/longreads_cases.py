"""the inputs of the long-read route (`dist -A --long-reads`, mk_sketch_push_fastq_long), regenerated from seeds.

Shared by tests/golden/make_golden_longreads.py (runs the real reference on the CHOPPED files, in the build container only), by
tests/test_longreads_model.py (CPU: the oracle on chopped files and on wide rows against those fixtures) and by
tests/test_gpu_longreads.py.  A case is a list of reads; from it come
    fastq(case)     the file as a sequencer would write it: reads of any length, headers padded so that the line ends fall where the
                    device kernels change paths
    wide_rows(case) one row per read at stride = longest read + 1: Oracle.koc_from_rows walks a row of any width with the reference's
                    per-read loop (iseq2comem.c:682-720), which gives the sketch wanted
    chopped(case)   every read cut into pieces of at most 4 094 characters that start every 4 094 - (TL - 1) characters: every
                    TL-window lies in exactly one piece, in file order, so the reference (whose fgets() width is 4 096,
                    iseq2comem.c:656,673) at -p 1 writes the wanted directory for this file
"""
import functools

import numpy as np

import util_inputs as ui

FQ_MAX = 4094  # characters of a line the reference's fgets(…, 4096, …) takes whole

# name -> (k, subk, drlevel, seed): tests/conftest.py's
GEOMS = {"L3K11": (11, 6, 3, 11), "L1K7": (7, 4, 1, 7), "L0K6": (6, 3, 0, 6)}
# bases the reads are cut from: large where few k-mers are accepted (1/4096 at L3K11), small where all are (131 071 slots at L0K6)
POOL = {"L3K11": 90000, "L1K7": 90000, "L0K6": 16000}
# distinct keys every expected sketch must reach, asserted by the tests and by the recipe: a `lengths` case covers most of its pool
# (about pool / 16^drlevel keys), a `dirty` case at least the 9 000 bases of its first read
MIN_KEYS = {"lengths_L3K11": 12, "lengths_L1K7": 3000, "lengths_L0K6": 12000, "dirty_L1K7": 450, "dirty_L0K6": 8000}

# case -> (kind, geometry).  The reference made a fixture for each (tests/golden/longreads/<case>/)
CASES = {
    "lengths_L3K11": ("lengths", "L3K11"),
    "lengths_L1K7": ("lengths", "L1K7"),
    "lengths_L0K6": ("lengths", "L0K6"),
    "dirty_L1K7": ("dirty", "L1K7"),
    "dirty_L0K6": ("dirty", "L0K6"),
}


def TL(geom):
    return 2 * GEOMS[geom][0]


@functools.lru_cache(maxsize=None)
def get_shuf(geom):
    from metakssd_amd import capi
    return capi.Shuf.generate(*GEOMS[geom])


def lengths(tl):
    return [0, 1, tl - 1, tl, tl + 1, 63, 64, 65, 111, 112, 113, 527, 528, 529, 549, 550, 1023, 1024, 1025, 4094, 4095, 4096, 8193, 70001]


def _cut(pool, at, n):
    """n bases of the (circular) pool from `at`"""
    reps = (at % len(pool) + n) // len(pool) + 1
    return (pool * reps)[at % len(pool): at % len(pool) + n]


@functools.lru_cache(maxsize=None)
def reads(case):
    """the sequence lines of the case's records, in file order"""
    kind, geom = CASES[case]
    rs = np.random.RandomState({"lengths": 1801, "dirty": 1802}[kind] + GEOMS[geom][3])
    pool = ui.rand_seq(rs, POOL[geom])
    tl = TL(geom)
    if kind == "lengths":
        # every length once, then the short ones again until there are 68 records (64 line-end offsets mod 64 + 4 at segment bounds);
        # the cuts overlap in the pool, so k-mers repeat across reads (counts above 1), some on the other strand
        ls = lengths(tl)
        short = [n for n in ls if n <= 1025]
        ls = ls + [short[i % len(short)] for i in range(68 - len(ls))]
        out = []
        for i, n in enumerate(ls):
            s = _cut(pool, int(rs.randint(0, len(pool))), n)
            out.append(ui.revcomp(s) if i % 3 == 1 else s)
        return tuple(out)
    # dirty: what a sequencer does not write but the reference's loop sees
    a = _cut(pool, 100, 9000)
    out = [
        a[:3000] + b"N" * 40 + a[3000:6000] + b"NNN" + a[6000:],            # runs of N inside a long read: no base, the window starts anew
        a[:5000].lower() + a[5000:],                                          # lower case: bases like capitals (Basemap, global_basic.c:62-69)
        _cut(pool, 4000, 4500) + b"\r",                                       # a CRLF file's sequence line keeps its '\r'
        _cut(pool, 200, 300) + b"\r",
        a[2000:2100] + b"n" + a[2100:2200] + b"-*." + a[2200:6500],           # an n, and bytes that are no base
        b"N" * 5000,                                                          # nothing but N
        b"",                                                                  # an empty sequence line
        _cut(pool, 7000, 4096) + b"X" + _cut(pool, 7000, 4096),               # the same 4 096 bases twice: counts above 1
        ui.revcomp(a),                                                        # the other strand of the first read
        b"ACGT" * 3 + b">" + _cut(pool, 50, 200) + b"@" + _cut(pool, 300, 5000),  # '>' and '@' inside a sequence are no bases either
    ]
    return tuple(out)


# header and quality lines of the dirty case, by record index: '>' and '@' in both, a quality line that starts with '@', CRLF ends
_DIRTY_HEADERS = [b"@r0 >not a fasta header", b"@r1 @@ twice", b"@r2 crlf\r", b"@r3 crlf\r", b"@>", b"@r5", b"@", b"@r7 " + b">" * 70, b"@r8", b"@r9"]


def _dirty_qual(i, n):
    q = bytearray(b"I" * n)
    if n:
        q[0] = ord("@")  # a quality line starting with '@' is no header
    for j in range(7, n, 97):
        q[j] = ord(">") if (i + j) % 2 else ord("@")
    return bytes(q)


@functools.lru_cache(maxsize=None)
def fastq(case):
    kind, _ = CASES[case]
    rd = reads(case)
    if kind == "dirty":
        out = []
        for i, s in enumerate(rd):
            crlf = s.endswith(b"\r")
            body = s[:-1] if crlf else s
            plus, qual = (b"+\r", _dirty_qual(i, len(body)) + b"\r") if crlf else (b"+", _dirty_qual(i, len(s)))
            out.append(b"\n".join([_DIRTY_HEADERS[i], s, plus, qual]) + b"\n")
        return b"".join(out)
    # lengths: the header of record i is padded so that the '\n' behind its sequence line falls on offset i mod 64 (records 0..63: every
    # offset of a 64-byte step), and for the last four on offsets 1022, 1023, 0 and 1 mod 1024 (both sides of a segment bound)
    out, pos = [], 0
    for i, s in enumerate(rd):
        head = b"@r%d " % i
        mod, want = (64, i) if i < 64 else (1024, (1022, 1023, 0, 1)[i - 64])
        pad = (want - (pos + len(head) + 1 + len(s))) % mod
        rec = head + b"h" * pad + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n"
        out.append(rec)
        pos += len(rec)
    return b"".join(out)


def line_end_offsets(text):
    return np.flatnonzero(np.frombuffer(text, np.uint8) == 10)


def rows_of(seqs):
    """one row per read, as wide as the longest: (rows, stride)"""
    stride = max([len(s) for s in seqs] + [0]) + 1
    return ui.rows_from_seqs(list(seqs), stride), stride


def wide_rows(case):
    return rows_of(reads(case))


def truncated_rows(case):
    """the same reads cut at the reference's line width: what a framer that truncates would sketch"""
    return rows_of([s[:FQ_MAX] for s in reads(case)])


def chop(seqs, tl):
    """pieces of at most FQ_MAX characters starting every FQ_MAX - (tl - 1): a window of tl characters lies in exactly one piece"""
    step = FQ_MAX - (tl - 1)
    out = []
    for s in seqs:
        at = 0
        while True:
            out.append(s[at:at + FQ_MAX])
            if at + FQ_MAX >= len(s):
                break
            at += step
    return out


def chopped_fastq(seqs, tl):
    return b"".join(b"@c%d\n" % i + p + b"\n+\n" + b"I" * len(p) + b"\n" for i, p in enumerate(chop(seqs, tl)))


def chopped(case):
    return chopped_fastq(reads(case), TL(CASES[case][1]))


def records(text):
    """the sequence lines of the records the reference would take from `text` if its lines were unbounded: four lines a record, the
    last record only when its fourth line has at least one byte (iseq2comem.c:673)"""
    lines = text.split(b"\n")  # the last element is what follows the last '\n' (empty when the text ends in one)
    out = []
    for i in range(0, len(lines) - 3, 4):
        last = i + 3 == len(lines) - 1  # the fourth line has no '\n' behind it
        if last and not lines[i + 3]:
            break
        out.append(lines[i + 1])
    return out
