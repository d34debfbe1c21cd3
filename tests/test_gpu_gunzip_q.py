"""Single-member gzip FASTQ on the device for the -n / -Q reader (mk_sketch_push_gzip_q, `dist -n / -Q --device-gunzip`; DESIGN.md
4.17): the engine against the host stream over batch boundaries that cut records, the record shapes of fastq2co's rule, the
first-record exception of a file that reaches its last slice through the carry, member concatenations, the long-line error, and the
command line against the golden directories and the `zcat -fc` route.  Streams are tests/gunzip_model.py's deflate(text, 6, 1) in
one gzip member, spans are 1024 compressed bytes, and the model says which status to expect."""
import filecmp
import functools
import gzip
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_util as bu
import golden_cases as gc
import gunzip_model as gm
import gunzip_members_model as mm
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
MANIFEST = json.load(open(os.path.join(gc.GOLDEN, "manifest.json")))
SPAN = 1024


def gz(raw, text, name=None):
    """one gzip member around a raw deflate stream"""
    head = bytes([0x1f, 0x8b, 8, 8 if name else 0]) + b"\0\0\0\0\x00\x03" + (name + b"\0" if name else b"")
    return head + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)


def member(text):
    raw = gm.deflate(text, 6, 1)
    return raw, gz(raw, text)


def nspans(raw):
    return (len(raw) + SPAN - 1) // SPAN


def batches_of(pieces, batch):
    """batches that hold a piece: a piece belongs to the batch whose spans hold its first bit"""
    return len({start // (8 * SPAN * batch) for start, _ in pieces}) if batch else 1


@pytest.fixture(scope="module")
def shuf():
    return capi.Shuf.generate(*gc.SHUF_SPECS["L1K7"])


@pytest.fixture
def eng(shuf):
    e = capi.Engine(shuf, 0)
    yield e
    e.close()


def host(eng, text, qmin, occ_min):
    eng.begin_occ(occ_min)
    eng.push_fastq(text, nthreads=2, occ=True, TL=int(eng.params.TL), qmin=qmin)
    return eng.finish()


def nids(res):
    return sum(len(ids) for ids, _ in res)


def same(got, want, what):
    assert len(got) == len(want), what
    for (gi, gcnt), (wi, wcnt) in zip(got, want):
        assert np.array_equal(gi, wi) and (gcnt is None) == (wcnt is None), what


def device(eng, path, qmin, occ_min, **kw):
    eng.begin_occ(occ_min)
    st = eng.push_gzip_q(path, qmin=qmin, span_bytes=SPAN, **kw)
    return st, eng.finish()


# ---- 1. the engine against the host stream ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lowcov():
    text = bu.golden_text("fq_lowcov")
    raw, f = member(text)
    mst, mtext, pieces = gm.run(raw, SPAN, 16)
    assert mst == gm.OK and mtext == text
    return text, raw, f, pieces


@pytest.mark.parametrize("qmin", [-128, 0, 53, 74])
def test_engine_push_gzip_q_equals_host_stream(eng, tmp_path, qmin):
    """batch_spans = 1 puts about 15 records in a batch, so nearly every batch boundary cuts a record: the carry through d_carry and
    the per-slice qinfo index.  Every quality byte of this text is 73: at qmin 74 every base is masked, and the want is empty on
    both sides by the rule itself; at every other qmin it must hold ids."""
    text, raw, f, pieces = lowcov()
    want = host(eng, text, qmin, 2)
    assert (nids(want) > 0) == (qmin < 74)
    inp = str(tmp_path / "lowcov.fq.gz")
    open(inp, "wb").write(f)
    assert len(pieces) == nspans(raw) > 60  # a piece a span: every batch has pieces
    for batch in (1, 3, 0):
        st, got = device(eng, inp, qmin, 2, batch_spans=batch)
        same(got, want, (qmin, batch))
        assert st.rows == text.count(b"\n") // 4 and st.text_bytes == len(text) and st.pieces == len(pieces)
        assert st.batches == batches_of(pieces, batch) == ((nspans(raw) + batch - 1) // batch if batch else 1)
        assert st.bad_status == 0 and st.bad_piece == -1 and st.members == 1


# ---- 2. record shapes across batch boundaries ------------------------------------------------------------------------------------------
RECS = [b"@r0 x\nACGTACGTAC\n+\nIIIIIIIII\n",        # quality line one byte shorter than its sequence: its '\n' is quality 10
        b"@r1\nACGTACGT\n+r1\nII\n",                  # several bytes shorter; a +name third line
        b"@r2\n\n+\n\n",                              # empty sequence, empty quality line
        b"@r3\r\nACGTTT\r\n+\r\nIIIIII\r\n",         # CRLF: the '\r' stays in the row
        b"@r4\nACGT\n+\nIIIIIIII\n",                  # quality line longer than its sequence
        b"@r5\nACGTAC\n+\n\n",                        # empty quality line behind a sequence
        b"@r6\nACGTACG\n+\n\x80I\xff\x05I~\x7f\n"]  # bytes >= 0x80 are negative qualities
TAILS = (b"", b"@r7\nACG\n+\nII", b"@r7\nACG\n+\n", b"@r7\nACG", b"@r7\nACG\n+", b"\n", b"\n\n\n\nX")


def shapes_text():
    """The shapes above, each followed by the same shape around a 40-base read cut from a small pool (the short ones hold no
    k-mer of 14 bases, so they alone would show equal empty results), with random read names so that 20 KB stay above four spans."""
    rs = np.random.RandomState(11)
    pool = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 400))
    name = lambda: b"@" + bytes(rs.choice(np.frombuffer(b"0123456789abcdef", dtype=np.uint8), 12))
    out = []
    while sum(len(x) for x in out) < 20000:
        for k, rec in enumerate(RECS):
            out.append(name() + rec[rec.index(b"r%d" % k) + 2:])
            a = rs.randint(0, len(pool) - 40)
            s, good = pool[a:a + 40], bytes(rs.randint(50, 75, 40, dtype=np.uint8))
            q = [good[:39], good[:20], b"", good, good + b"IIII", b"", good[:10] + b"\x80\xff\x05~\x7f" + good[15:]][k]
            nl = b"\r\n" if k == 3 else b"\n"
            out.append(name() + nl + (b"" if k == 2 else s) + nl + b"+" + nl + q + nl)
    return b"".join(out)


@pytest.mark.parametrize("tail", range(len(TAILS)))
def test_record_shapes_across_batch_boundaries(eng, tmp_path, tail):
    text = shapes_text() + TAILS[tail]
    raw, f = member(text)
    assert nspans(raw) >= 4 and gm.run(raw, SPAN, 16)[0] == gm.OK
    inp = str(tmp_path / "shapes.fq.gz")
    open(inp, "wb").write(f)
    for qmin in (-128, 53):
        want = host(eng, text, qmin, 1)
        assert nids(want) > 0
        for batch in (1, 0):
            st, got = device(eng, inp, qmin, 1, batch_spans=batch)
            same(got, want, (tail, qmin, batch))
            assert st.rows == text.count(b"\n") // 4 and st.text_bytes == len(text)
            assert st.batches > 3 if batch else st.batches == 1
    assert nids(host(eng, text, 53, 1)) != nids(host(eng, text, -128, 1))  # the mask shows


# ---- 3. the first-record exception at file level ---------------------------------------------------------------------------------------
def partial_record(rs, n=3000, qn=2500):
    """three lines and a part of the fourth, each below 4095 characters, that stay above three spans when compressed"""
    seq = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))
    return b"@first\n" + seq + b"\n+\n" + bytes(rs.randint(33, 74, qn, dtype=np.uint8))


def test_first_record_exception_reaches_the_last_slice_through_the_carry(eng, tmp_path):
    rs = np.random.RandomState(3)
    part = partial_record(rs)
    assert part.count(b"\n") == 3 and max(len(x) for x in part.split(b"\n")) < 4095
    whole = partial_record(rs, 3000, 3000).replace(b"@first", b"@whole") + b"\n"
    lone = bytes(rs.randint(65, 91, 3000, dtype=np.uint8))
    # (text, rows): (a) the incomplete record alone is walked; (b) behind a complete record it is not; (c) one line is no record
    for name, text, rows in (("a", part, 1), ("b", whole + part, 1), ("c", b"@only a header", 0), ("c_long", lone, 0)):
        raw, f = member(text)
        mst, _, pieces = gm.run(raw, SPAN, 16)
        assert mst == gm.OK and (name == "c" or (nspans(raw) >= 3 and batches_of(pieces, 1) >= 3)), name
        inp = str(tmp_path / (name + ".fq.gz"))
        open(inp, "wb").write(f)
        for qmin in (-128, 40):
            want = host(eng, text, qmin, 1)
            assert (nids(want) > 0) == (rows > 0), (name, qmin)
            for batch in (1, 0):
                st, got = device(eng, inp, qmin, 1, batch_spans=batch)  # MK_OK: no exception raised
                same(got, want, (name, qmin, batch))
                assert st.rows == rows and st.text_bytes == len(text), (name, qmin, batch)
                assert st.batches == batches_of(pieces, batch)
    # (b)'s row is the complete record: the same ids as that record alone
    same(host(eng, whole + part, 40, 1), host(eng, whole, 40, 1), "b")
    assert nids(host(eng, part, 40, 1)) != nids(host(eng, part, -128, 1))  # (a)'s quality line, as far as it goes, masks


# ---- 4. members ---------------------------------------------------------------------------------------------------------------------
def test_members(eng, tmp_path):
    text = bu.golden_text("fq_ragged")
    lines = text.split(b"\n")
    at = np.cumsum([0] + [len(x) + 1 for x in lines])  # at[j]: where line j starts
    nrec = (len(lines) - 1) // 4
    in_seq = int(at[4 * (nrec // 3) + 1]) + len(lines[4 * (nrec // 3) + 1]) // 2
    in_qual = int(at[4 * (2 * nrec // 3) + 3]) + len(lines[4 * (2 * nrec // 3) + 3]) // 2
    cuts = sorted([int(at[4 * (nrec // 6)]), in_seq, int(at[4 * (nrec // 2)]), in_qual, int(at[4 * (5 * nrec // 6)])])
    assert len(set(cuts)) == 5 and text[in_seq:in_seq + 1] in b"ACGTNacgtn" and lines[4 * (2 * nrec // 3) + 3]
    parts = [text[a:b] for a, b in zip([0] + cuts, cuts + [len(text)])]
    parts = parts[:3] + [b""] + parts[3:] + [b""]
    f = b"".join(mm.gz(gm.deflate(p, 6, 1), p) for p in parts)
    assert gzip.decompress(f) == text
    res = mm.run_file(f, SPAN, 16)
    assert res[0] == mm.OK and res[1] == text and len(res[3]) == 8
    inp = str(tmp_path / "members.fq.gz")
    open(inp, "wb").write(f)
    for qmin in (0, 74):
        want = host(eng, text, qmin, 1)
        assert (nids(want) > 0) == (qmin < 74)  # every quality byte of this text is 73
        for batch in (1, 0):
            st, got = device(eng, inp, qmin, 1, batch_spans=batch, members=True)
            same(got, want, (qmin, batch))
            assert st.members == 8 and st.rows == nrec and st.text_bytes == len(text)
    eng.begin_occ(1)
    with pytest.raises(capi.MkError) as ei:
        eng.push_gzip_q(inp, qmin=0, span_bytes=SPAN)
    assert ei.value.code == capi.MK_ERR_FORMAT and ei.value.stats.bad_status == capi.MK_INFL_TRAILING
    eng.finish()


# ---- 5. a long line ------------------------------------------------------------------------------------------------------------------
def late_long_text():
    """reads cut from a 10 kb pool (30x coverage) with mostly passing qualities, the 3 001st of 6 000 bases"""
    rs = np.random.RandomState(5)
    pool = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 10000))

    def rec(i, n):
        a = rs.randint(0, len(pool) - n + 1)
        return b"@r%d\n" % i + pool[a:a + n] + b"\n+\n" + bytes(rs.randint(50, 75, n, dtype=np.uint8)) + b"\n"
    short = [rec(i, 100) for i in range(3000)]
    return b"".join(short), b"".join(short) + rec(3000, 6000) + b"".join(rec(i, 100) for i in range(3001, 3101))


def test_long_line_is_a_format_error_and_the_engine_goes_on(eng, tmp_path):
    good, text = late_long_text()
    want = host(eng, good, 53, 2)
    assert nids(want) > 0
    inp = str(tmp_path / "late_long.fq.gz")
    open(inp, "wb").write(member(text)[1])
    eng.begin_occ(2)
    with pytest.raises(capi.MkError) as ei:
        eng.push_gzip_q(inp, qmin=53, span_bytes=SPAN, batch_spans=8)
    st = ei.value.stats
    assert ei.value.code == capi.MK_ERR_FORMAT and st.bad_status == 0 and st.bad_piece == -1
    assert 0 < st.rows <= 3000
    eng.finish()  # what was pushed is dropped
    same(host(eng, good, 53, 2), want, "after the error")
    ok = str(tmp_path / "good.fq.gz")
    open(ok, "wb").write(member(good)[1])
    st, got = device(eng, ok, 53, 2)
    same(got, want, "the device route after the error")
    assert st.rows == 3000


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuf_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shuf")
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = str(d / (name + ".shuf"))
            gc.make_shuf(name, cache[name])
        return cache[name]
    return get


def run_cli(shuf, flags, out, inputs, extra=(), env=None, threads=4):
    inputs = [inputs] if isinstance(inputs, str) else list(inputs)
    r = subprocess.run([CLI, "dist", "-L", shuf] + list(flags) + ["-p", str(threads), "--quiet", "--timing", "-o", out] + list(extra) + inputs,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    routes = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return r, routes


def same_dir(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and "cofiles.stat" in fa
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def text_name_of(case):
    kind, base, *variant = gc.CASES[case]["input"].split(":")
    v = variant[0] if variant else ""
    return "fq_%s%s" % (base, "_" + v if v in ("crlf", "trunc", "nonl") else "")


@functools.lru_cache(maxsize=None)
def modelled(name, ratio=16):
    """the committed input `name` as this file compresses it -> (text, raw, model status, model pieces)"""
    text = bu.golden_text(name)
    raw = gm.deflate(text, 6, 1)
    mst, _, pieces = gm.run(raw, SPAN, ratio)
    return text, raw, mst, pieces


FQ_Q = sorted(c for c, e in gc.CASES.items() if "-A" not in e["flags"] and e["input"].startswith("fq:") and c in MANIFEST["cases"])
FALL_BACK = ["key0_n2_L0K6z", "long_n2_L0K6", "long_set_L1K7"]
GUNZIP = ["--device-gunzip", "--gunzip-span-bytes", str(SPAN)]


def status_text(st):
    return capi.lib.mk_gunzip_status_text(st).decode()


def test_case_selection():
    """fifteen cases take the device route with more than one piece each; three meet the capacity rule of R = 16"""
    assert len(FQ_Q) == 18 and all(c in FQ_Q for c in FALL_BACK)
    fam = {}
    for c in FQ_Q:
        text, raw, mst, pieces = modelled(text_name_of(c))
        if c in FALL_BACK:
            assert mst == gm.CAPACITY, c
            assert (len(raw) <= SPAN) == (c == "key0_n2_L0K6z")
        else:
            assert mst == gm.OK and len(pieces) > 1, c
            fam.setdefault(c.split("_")[0], []).append(len(pieces))
    assert {k: len(v) for k, v in fam.items()} == {"lowcov": 6, "qual": 5, "ragged500": 4}
    assert set(fam["lowcov"]) == {72} and set(fam["qual"]) == {102} and all(p >= 20 for p in fam["ragged500"])


@pytest.mark.parametrize("case", FQ_Q)
def test_cli_gunzip_q_equals_zcat_route_and_reference(case, shuf_files, tmp_path):
    entry = MANIFEST["cases"][case]
    assert not entry["aborted"]
    text, raw, mst, want = modelled(text_name_of(case))
    inp = str(tmp_path / (case + ".fq.gz"))
    open(inp, "wb").write(gz(raw, text, name=b"reads.fq"))
    shuf = shuf_files(entry["shuf"])
    base = str(tmp_path / "zcat")
    r, routes = run_cli(shuf, entry["flags"], base, inp, ["--no-device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    plain = str(tmp_path / "plain")
    r, routes = run_cli(shuf, entry["flags"], plain, inp)  # without the switch: today's route
    assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    same_dir(base, plain)
    exp = os.path.join(gc.GOLDEN, "expected", case)
    runs = [(GUNZIP, mst, want, status_text(mst))]
    if mst:
        assert case in FALL_BACK and mst == gm.CAPACITY
        _, _, mst64, want64 = modelled(text_name_of(case), 64)
        long = max(len(x) for x in text.split(b"\n")) >= 4095
        assert (case.startswith("long_")) == long
        fb = status_text(mst64) if mst64 else "long line" if long else None  # a text the inflate accepts still has its long lines
        runs.append((GUNZIP + ["--gunzip-ratio", "64"], mst64, want64, fb))
        assert case != "key0_n2_L0K6z" or fb is None
    else:
        assert case not in FALL_BACK
        runs[0] = (GUNZIP, 0, want, None)
    for k, (flags, status, pieces, fb) in enumerate(runs):
        out = str(tmp_path / ("dev%d" % k))
        r, routes = run_cli(shuf, entry["flags"], out, inp, flags)
        assert r.returncode == 0, r.stderr.decode()
        if fb is not None:
            assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", fb)]  # never silent
        else:
            assert [x["route"] for x in routes] == ["device-gunzip"], "the device route was not taken: %s" % routes
            assert routes[0]["rows"] == text.count(b"\n") // 4
            assert routes[0]["pieces"] == len(pieces) and routes[0]["text_bytes"] == len(text)
            assert len(pieces) > 1 or len(raw) <= SPAN
        same_dir(base, out)
        for f in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), "%s: %s differs from the reference" % (case, f)


def five_members(text):
    """cut where no record starts: a record straddles every boundary"""
    cuts = [len(text) * k // 5 for k in range(6)]
    for k in range(1, 5):
        while text[cuts[k] - 1:cuts[k]] == b"\n":
            cuts[k] += 1
    parts = [text[a:b] for a, b in zip(cuts, cuts[1:])]
    assert b"".join(parts) == text and all(parts)
    return b"".join(mm.gz(gm.deflate(p, 6, 1), p) for p in parts)


def test_cli_batches_and_poison(shuf_files, tmp_path):
    case = "qual_Q54_n2_L0K6"
    entry = MANIFEST["cases"][case]
    text, raw, mst, pieces = modelled(text_name_of(case))
    assert mst == gm.OK and len(pieces) > 100
    inp = str(tmp_path / "qual.fq.gz")
    open(inp, "wb").write(gz(raw, text))
    exp = os.path.join(gc.GOLDEN, "expected", case)
    shuf = shuf_files(entry["shuf"])
    env = dict(os.environ, MK_POISON="0xA5")
    half = (nspans(raw) + 1) // 2
    for k, (batch, e) in enumerate(((8, None), (half, env), (0, env))):
        flags = GUNZIP + (["--gunzip-batch-spans", str(batch)] if batch else [])
        out = str(tmp_path / ("out%d" % k))
        r, routes = run_cli(shuf, entry["flags"], out, inp, flags, env=e)
        assert r.returncode == 0, r.stderr.decode()
        assert [x["route"] for x in routes] == ["device-gunzip"] and routes[0]["pieces"] == len(pieces)
        assert routes[0]["batches"] == batches_of(pieces, batch) and (batches_of(pieces, batch) > 1) == (batch > 0)
        assert routes[0]["rows"] == text.count(b"\n") // 4 and "members" not in routes[0]
        for f in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), f
    f5 = five_members(text)
    assert gzip.decompress(f5) == text
    inp5 = str(tmp_path / "qual5.fq.gz")
    open(inp5, "wb").write(f5)
    out = str(tmp_path / "out5")
    r, routes = run_cli(shuf, entry["flags"], out, inp5, GUNZIP + ["--gunzip-members"], env=env)
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["device-gunzip"] and routes[0]["members"] == 5 and routes[0]["text_bytes"] == len(text)
    for f in entry["files"]:
        assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), f


def test_cli_two_inputs_one_falls_back(shuf_files, tmp_path):
    """-p 1: with several inputs and more than one thread the prefetch workers read the files ahead, and their path keeps zcat
    for every file (it names no route); one thread takes the inputs one after the other through the readers tested here"""
    ta, tb = bu.golden_text("fq_ragged"), bu.golden_text("fq_qual")
    fa, fb = member(ta)[1], member(tb)[1]
    a, b = str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq.gz")
    open(a, "wb").write(fa + fa)  # two members without --gunzip-members
    open(b, "wb").write(fb)
    shuf = shuf_files("L1K7")
    flags = ["-n", "2", "-Q", "53"]
    base, out = str(tmp_path / "zcat"), str(tmp_path / "dev")
    r, routes = run_cli(shuf, flags, base, [a, b], ["--no-device-inflate"], threads=1)
    assert r.returncode == 0, r.stderr.decode()
    assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", None), ("zcat", None)]
    r, routes = run_cli(shuf, flags, out, [a, b], GUNZIP, threads=1)
    assert r.returncode == 0, r.stderr.decode()
    assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", "more members behind the first"), ("device-gunzip", None)]
    assert routes[1]["rows"] == tb.count(b"\n") // 4
    same_dir(base, out)
    assert os.path.getsize(os.path.join(out, "combco.0")) > 0


def test_cli_damaged_file_fails_with_zcats_message(shuf_files, tmp_path):
    text, raw, mst, _ = modelled("fq_ragged")
    bad = bytearray(gz(raw, text))
    bad[10 + len(raw) // 2] ^= 0x04  # one payload bit
    inp = str(tmp_path / "bad.fq.gz")
    open(inp, "wb").write(bytes(bad))
    outs = []
    for k, extra in enumerate(([], GUNZIP)):
        out = str(tmp_path / ("out%d" % k))
        r, routes = run_cli(shuf_files("L1K7"), ["-n", "2"], out, inp, extra)
        err = r.stderr.decode()
        assert r.returncode != 0 and "bad.fq.gz" in err and "zcat" in err, err
        assert not os.path.exists(os.path.join(out, "cofiles.stat"))
        outs.append((r.returncode, err))
    assert outs[0] == outs[1]  # today's message and exit status
