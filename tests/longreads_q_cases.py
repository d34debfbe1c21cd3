"""the inputs of the long route of the other FASTQ reader (`dist -n N -Q q --long-reads-q`, mk_sketch_push_fastq_long_q; DESIGN.md
4.21), regenerated from seeds.  Builds on tests/longreads_cases.py: the same reads and header padding, with quality lines that mask.

Shared by tests/golden/make_golden_longreads_q.py (runs the real reference on the CHOPPED files), by tests/test_longreads_q_model.py
(CPU: oracle, Python model and fixtures) and by tests/test_gpu_longreads_q.py.
    quals(case)      one quality line a read, about one byte in a hundred below Q = 53
    fastq(case)      the file: lc.fastq's layout with those quality lines
    chop_q           sequence and quality lines cut at the same places as lc.chop
    chopped(case)    the file the reference reads (its fgets() width for this reader is 20 000, iseq2comem.c:319; the pieces are kept
                     at lc.FQ_MAX so that both recipes cut alike)
    masked(text, q)  the Python model of the rule: the sequence lines of the records that count, masked column by column
"""
import functools

import numpy as np

import longreads_cases as lc
import util_inputs as ui

Q = 53  # the threshold the quality lines are built around: 53 is kept, 52 is masked
MQ = [(1, 0), (1, 53), (2, 53)]  # (M, Q) of the fixtures: -n M -Q Q

CASES = {
    "lengths_q_L3K11": ("lengths_q", "L3K11"),
    "lengths_q_L1K7": ("lengths_q", "L1K7"),
    "lengths_q_L0K6": ("lengths_q", "L0K6"),
    "dirty_q_L1K7": ("dirty_q", "L1K7"),
    "dirty_q_L0K6": ("dirty_q", "L0K6"),
}
FIXTURE_CASES = [c for c in CASES if CASES[c][0] == "lengths_q"]  # the reference made these (dirty_q is pinned to the host framer)
# distinct keys every directory of a case must reach (the smallest is -n 2 -Q 53), asserted by the recipe on the reference's output
MIN_KEYS = {"lengths_q_L3K11": 3, "lengths_q_L1K7": 1000, "lengths_q_L0K6": 12000}

LOW = (Q - 1, 0x80, 33, 0xFF, Q - 1, 0x8A)  # what a masked byte holds: one below Q, '!' and bytes that are negative as signed char
HIGH = (Q, 0x7F, Q + 1)                     # sprinkled among the 'I': kept, Q itself among them


def base_case(case):
    kind, geom = CASES[case]
    return ("lengths_" if kind == "lengths_q" else "dirty_") + geom


def TL(case):
    return lc.TL(CASES[case][1])


@functools.lru_cache(maxsize=None)
def reads(case):
    rd = lc.reads(base_case(case))
    if CASES[case][0] == "dirty_q":
        return tuple(s[:-1][: lc.FQ_MAX - 1] + b"\r" if s.endswith(b"\r") else s[: lc.FQ_MAX] for s in rd)
    return rd


def _layout(case):
    """(header line, text offset of the quality line) per record of the lengths file: lc.fastq's padding"""
    out, pos = [], 0
    for i, s in enumerate(reads(case)):
        head = b"@r%d " % i
        mod, want = (64, i) if i < 64 else (1024, (1022, 1023, 0, 1)[i - 64])
        head += b"h" * ((want - (pos + len(head) + 1 + len(s))) % mod)
        qpos = pos + len(head) + 1 + len(s) + 1 + 2
        out.append((head, qpos))
        pos = qpos + len(s) + 1
    return out


@functools.lru_cache(maxsize=None)
def quals(case):
    kind, geom = CASES[case]
    rd, tl = reads(case), TL(case)
    rs = np.random.RandomState(2101 + lc.GEOMS[geom][3])
    if kind == "dirty_q":
        return _dirty_quals(rd)
    lay = _layout(case)
    step = lc.FQ_MAX - (tl - 1)
    longest = max(range(len(rd)), key=lambda i: len(rd[i]))
    out = []
    for i, s in enumerate(rd):
        n = len(s)
        q = bytearray(b"I" * n)
        for j in rs.randint(0, max(n, 1), size=n // 40):  # kept bytes that are not 'I'
            q[j] = HIGH[j % len(HIGH)]
        low = [int(j) for j in rs.randint(0, max(n, 1), size=n // 150)]  # single low bytes
        for at in range(step, n, step):  # runs of low quality across both ends of every piece the chopping makes
            low += [c for c in range(at - 2, at + 3) if c < n]
            low += [c for c in range(at - step + lc.FQ_MAX - 2, at - step + lc.FQ_MAX + 3) if c < n]
        if i == longest:  # a low byte on every offset of a 64-byte step of the file, and a run across a segment bound
            qpos = lay[i][1]
            low += [900 * r + ((r - (qpos + 900 * r)) % 64) for r in range(64)]
            at = 60000 + ((1023 - (qpos + 60000)) % 1024)
            low += [at - 1, at, at + 1, at + 2]
        for c in low:
            q[c] = LOW[(c + i) % len(LOW)]
        out.append(q)
    # Where every k-mer of the pool occurs many times (L0K6) chance never removes a key.  Sixteen windows of the longest read, away from
    # the marks above: the first eight lose their middle column wherever they occur, on either strand -- gone at Q = 53, there at Q = 0;
    # the other eight keep one clean occurrence -- there at -n 1, gone at -n 2.
    for t in range(16):
        at = 62000 + 150 * t  # (between the chopping boundaries of all three geometries)
        w = rd[longest][at:at + tl]
        for i, s in enumerate(rd):
            for pat in (w, ui.revcomp(w)):
                pos = s.find(pat)
                while pos >= 0:
                    if t >= 8 and i == longest and pos == at and pat == w:
                        out[i][pos:pos + tl] = b"I" * tl
                    else:
                        out[i][pos + tl // 2] = Q - 1
                    pos = s.find(pat, pos + 1)
    return tuple(bytes(q) for q in out)


def _dirty_quals(rd):
    """quality lines the sequencer does not write: shorter than the sequence by 1, by 65, empty, longer, '@' and '>' inside; low bytes
    every 89 columns.  A CRLF record's quality line ends in '\\r' like its sequence line."""
    out = []
    for i, s in enumerate(rd):
        crlf = s.endswith(b"\r")
        n = len(s) - 1 if crlf else len(s)
        q = bytearray(b"I" * n)
        if n:
            q[0] = ord("@")
        for j in range(7, n, 97):
            q[j] = ord(">") if (i + j) % 2 else ord("@")
        for j in range(11 + i, n, 89):
            q[j] = LOW[(i + j) % len(LOW)]
        q = bytes(q)
        if i == 0:
            q = q[:-1]          # one short: the '\n' is the last column's quality
        elif i == 1:
            q = q[:-65]         # 65 short: more than a step of the walk
        elif i == 4:
            q = b""             # empty: '\n' for column 0, 0 behind it
        elif i == 7:
            q = q + b"I" * 70   # longer than the sequence: ignored
        elif i == 8:
            q = q + b"#"
        out.append(q + b"\r" if crlf else q)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fastq(case):
    rd, ql = reads(case), quals(case)
    if CASES[case][0] == "dirty_q":
        return b"".join(b"\n".join([lc._DIRTY_HEADERS[i], s, b"+\r" if s.endswith(b"\r") else b"+", ql[i]]) + b"\n" for i, s in enumerate(rd))
    return b"".join(head + b"\n" + s + b"\n+\n" + q + b"\n" for (head, _), s, q in zip(_layout(case), rd, ql))


def chop_q(seqs, quals_, tl):
    """lc.chop on sequence and quality lines alike: [(piece of the sequence, piece of the quality line)]"""
    step = lc.FQ_MAX - (tl - 1)
    out = []
    for s, q in zip(seqs, quals_):
        at = 0
        while True:
            out.append((s[at:at + lc.FQ_MAX], q[at:at + lc.FQ_MAX]))
            if at + lc.FQ_MAX >= len(s):
                break
            at += step
    return out


def chopped_fastq(seqs, quals_, tl):
    return b"".join(b"@c%d\n" % i + p + b"\n+\n" + q + b"\n" for i, (p, q) in enumerate(chop_q(seqs, quals_, tl)))


def chopped(case):
    return chopped_fastq(reads(case), quals(case), TL(case))


# ---- the rule in Python (mk_fastq_frame_q) ----------------------------------------------------------------------------
def mask(seq, qline, qmin):
    """column i of `seq` as 'N' when the signed byte at column i of `qline` (the fourth line WITH its '\\n' if it has one; 0 behind it)
    is below qmin"""
    s = np.frombuffer(seq, np.uint8).copy()
    q = np.zeros(len(s), np.int16)
    m = min(len(s), len(qline))
    q[:m] = np.frombuffer(qline[:m], np.int8)
    if qmin > -128:
        s[q < qmin] = ord("N")
    return s.tobytes()


def masked(text, qmin):
    """the masked sequence lines of the records of `text` that count: records whose four lines all end in '\\n'; when there is none,
    the first record's second line if it exists, masked by the fourth line as far as that exists"""
    lines = text.split(b"\n")  # the last element is what follows the last '\n'
    whole = (len(lines) - 1) // 4
    out = [mask(lines[4 * r + 1], lines[4 * r + 3] + b"\n", qmin) for r in range(whole)]
    if whole == 0 and (len(lines) > 2 or (len(lines) == 2 and lines[1])):
        out.append(mask(lines[1], lines[3] if len(lines) == 4 else b"", qmin))
    return out


def masked_rule_A(text):
    """what -A's record rule (lc.records) would take from the same text, unmasked: the two rules differ on a last quality line
    without '\\n'"""
    return lc.records(text)
