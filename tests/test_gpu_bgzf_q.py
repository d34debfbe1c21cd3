"""BGZF-compressed FASTQ on the device for the -n / -Q reader (dist without -A): the quality-aware device framer against
mk_fastq_frame_q, mk_sketch_push_bgzf_q against the host stream, and `metakssd dist --device-inflate` on re-compressed golden
inputs against the `zcat -fc` route and the committed reference output"""
import filecmp
import json
import os
import subprocess

import numpy as np
import pytest

import bgzf_util as bz
import golden_cases as gc
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
MANIFEST = json.load(open(os.path.join(gc.GOLDEN, "manifest.json")))
TL = 22


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


def pitch(need):
    p = (need + 15) & ~15
    return p + (16 if p % 128 == 0 and p < 4096 else 0)  # MK_ROW_PITCH


def longest_line(text):
    parts = text.split(b"\n")
    return max([len(x) + 1 for x in parts[:-1]] + [len(parts[-1])])  # a terminated line counts its '\n', as mk_line() does


def lines_of(rows, stride, n):
    """rows -> their lines up to the '\\n'; what follows a line must be zeros"""
    out = []
    for k in range(n):
        r = rows[k * stride:(k + 1) * stride].tobytes()
        line = r[:r.index(b"\n") + 1]
        assert r[len(line):] == b"\0" * (stride - len(line))
        out.append(line)
    return out


def host_lines(text, qmin, records_before=0):
    """mk_fastq_frame_q over the whole text, final, at a stride that holds every line (and is wide enough for the host framer's TL)"""
    stride = max(48, pitch(longest_line(text) + 1))
    rows, n, nrec, used, rc = capi.fastq_frame_q(text, stride, TL, qmin=qmin, final=True, records_before=records_before)
    assert rc == 0 and n == nrec
    return lines_of(rows, stride, n), used


def device_lines(infl, pieces, qmin):
    """the pieces framed one after the other: the unconsumed tail is carried, the records so far are passed on"""
    out, carry, records = [], b"", 0
    for i, piece in enumerate(pieces):
        buf = carry + piece
        rows, stride, n, nrec, used, longest, rc = infl.frame_q(buf, qmin=qmin, final=i + 1 == len(pieces), records_before=records)
        assert rc == 0 and used <= len(buf) and n == nrec
        got = lines_of(rows, stride, n)
        if n:
            assert stride == pitch(max(len(x) for x in got))
        out += got
        records += nrec
        carry = buf[used:]
    return out, sum(len(p) for p in pieces) - len(carry)


FRAME_TEXTS = ["fq_ragged", "fq_ragged_nonl", "fq_ragged_trunc", "fq_ragged_crlf", "fq_qual", "fq_lowcov", "fq_homo"]
QMINS = [-128, 0, 53, 54, 74]


@pytest.fixture(scope="module")
def texts():
    return {name: bz.golden_text(name) for name in FRAME_TEXTS}


@pytest.fixture(scope="module")
def host_framed(texts):
    return {(name, q): host_lines(texts[name], q) for name in FRAME_TEXTS for q in QMINS}


# ---- the framer against the host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FRAME_TEXTS)
def test_framer_q_whole_text_equals_host(infl, texts, name):
    text = texts[name]
    for qmin in QMINS:
        rows, stride, n, nrec, consumed, longest, rc = infl.frame_q(text, qmin=qmin)
        assert rc == 0
        hrows, hn, hrec, hused, hrc = capi.fastq_frame_q(text, stride, TL, qmin=qmin)  # the same stride: byte for byte, padding included
        assert hrc == 0, (name, qmin, stride)
        assert (n, nrec, consumed) == (hn, hrec, hused) and consumed == len(text), (name, qmin)
        assert np.array_equal(hrows, rows), (name, qmin)
        parts = text.split(b"\n")
        assert longest == max([len(x) + 1 for x in parts[:-1]] + [len(parts[-1])])
        assert stride == pitch(max(len(x) + 1 for x in parts[1:4 * n:4]))  # the longest sequence line among the rows


@pytest.mark.parametrize("name", FRAME_TEXTS)
@pytest.mark.parametrize("chunk", [1024, 4097])
def test_framer_q_chunked_equals_host(infl, texts, host_framed, name, chunk):
    text = texts[name]
    if len(text) > 120000:  # (the tile and piece boundaries repeat: a part of the large texts is enough)
        text = text[:120000]
    for qmin in QMINS:
        want, used = host_lines(text, qmin) if len(text) != len(texts[name]) else host_framed[(name, qmin)]
        got, total = device_lines(infl, [text[a:a + chunk] for a in range(0, len(text), chunk)], qmin)
        assert got == want and total == used, (name, qmin)


RECS = [b"@r0 x\nACGTACGTAC\n+\nIIIIIIIII\n",        # quality line one byte shorter than its sequence: its '\n' is quality 10
        b"@r1\nACGTACGT\n+r1\nII\n",                  # several bytes shorter; a +name third line
        b"@r2\n\n+\n\n",                              # empty sequence, empty quality line
        b"@r3\r\nACGTTT\r\n+\r\nIIIIII\r\n",         # CRLF: the '\r' stays in the row
        b"@r4\nACGT\n+\nIIIIIIII\n",                  # quality line longer than its sequence
        b"@r5\nACGTAC\n+\n\n",                        # empty quality line behind a sequence
        b"@r6\nACGTACG\n+\n\x80I\xff\x05I~\x7f\n"]  # bytes >= 0x80 are negative qualities
TAILS = (b"", b"@r7\nACG\n+\nII", b"@r7\nACG\n+\n", b"@r7\nACG", b"@r7\nACG\n+", b"\n", b"\n\n\n\nX")


def test_framer_q_every_cut_of_a_short_file(infl):
    body = b"".join(RECS)
    for tail in TAILS:
        text = body + tail
        for qmin in (10, 11):
            want, used = host_lines(text, qmin)
            assert used == len(text)
            whole, total = device_lines(infl, [text], qmin)
            assert whole == want and total == used, (tail, qmin)
            # every cut of the whole file for one tail; for the others the first two records and everything from the last record on
            cuts = range(len(text) + 1) if tail == TAILS[1] else list(range(len(RECS[0]) + len(RECS[1]) + 2)) + list(range(len(body) - len(RECS[-1]), len(text) + 1))
            for cut in cuts:
                got, total = device_lines(infl, [text[:cut], text[cut:]], qmin)
                assert got == want and total == used, (tail, qmin, cut)
    # the terminator-as-quality-10 rule shows between 10 and 11: base 9 of r0 and base 2 of r1 sit on their quality lines' '\n'
    assert host_lines(body, 10)[0][:2] == [b"ACGTACGTAC\n", b"ACGNNNNN\n"] and host_lines(body, 11)[0][:2] == [b"ACGTACGTAN\n", b"ACNNNNNN\n"]
    # not final: only complete records count, the rest is left for the next call
    text = body + b"@r7\nACG\n+\nII"
    rows, stride, n, nrec, consumed, longest, rc = infl.frame_q(text, qmin=0, final=False)
    assert rc == 0 and n == nrec == len(RECS) and consumed == len(body)
    assert infl.frame_q(b"@r\nAC", final=False)[2:5] == (0, 0, 0)


def test_framer_q_first_record_exception(infl):
    """the first record of a file is walked although it is not complete (iseq2comem.c:343-349), later ones are not"""
    for text in (b"@r\nACGT", b"@r\nACGT\n", b"@r\nACGT\n+\n", b"@r\nACGT\n+\nIII"):
        for qmin in (0, 1):
            want, used = host_lines(text, qmin)
            assert len(want) == 1 and used == len(text)
            got, total = device_lines(infl, [text], qmin)
            assert got == want and total == used, (text, qmin)
            for cut in range(len(text) + 1):
                got, total = device_lines(infl, [text[:cut], text[cut:]], qmin)
                assert got == want and total == used, (text, qmin, cut)
            rows, stride, n, nrec, consumed, longest, rc = infl.frame_q(text, qmin=qmin, records_before=1)
            assert (rc, n, nrec, consumed) == (0, 0, 0, len(text)) and host_lines(text, qmin, records_before=1) == ([], len(text))
    assert host_lines(b"@r\nACGT\n+\nIII", 1)[0] == [b"ACGN\n"] and host_lines(b"@r\nACGT\n+\n", 1)[0] == [b"NNNN\n"]
    for text in (b"", b"@r\n", b"@r"):
        assert host_lines(text, 0) == ([], len(text))
        assert infl.frame_q(text, qmin=0)[2:5] == (0, 0, len(text))
    assert infl.frame_q(b"@r\nACGT\n+\nIII", final=False)[2:5] == (0, 0, 0)  # not final: still arriving


def test_framer_q_long_lines(infl):
    rec = lambda n: b"@long\n" + b"ACGT" * (n // 4) + b"ACGT"[:n % 4] + b"\n+\n" + b"I" * (n - 7) + b"5" * 7 + b"\n"
    short = b"@s\nACGT\n+\nIII5\n"
    text = short * 50 + rec(4094) + short * 50  # the widest row there is
    rows, stride, n, nrec, consumed, longest, rc = infl.frame_q(text, qmin=54)
    assert rc == 0 and stride == 4096 and n == nrec == 101 and longest == 4095 and consumed == len(text)
    hrows, hn, hrec, hused, hrc = capi.fastq_frame_q(text, 4096, TL, qmin=54)
    assert hrc == 0 and hn == n and np.array_equal(hrows, rows)
    assert rows[50 * 4096:51 * 4096].tobytes()[4080:] == b"ACGTACGNNNNNNN\n\0"
    # the device cuts no windows: a read the host framer would window is refused, and so is any other line of that length
    for bad in (short * 50 + rec(4095) + short, short + b"@" + b"h" * 4094 + b"\nACGT\n+\nIIII\n", short + b"@h\nACGT\n+\n" + b"I" * 4095 + b"\n" + short,
                rec(5000) * 3):
        assert capi.fastq_frame_q(bad, 4096, TL)[4] == 0  # inside fastq2co's contract on the host
        assert infl.frame_q(bad)[6] == capi.MK_ERR_FORMAT


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
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


def test_engine_push_bgzf_q_equals_host_stream(tmp_path):
    text = bz.golden_text("fq_lowcov")
    shuf = capi.Shuf.generate(*gc.SHUF_SPECS["L1K7"])
    eng = capi.Engine(shuf, 0)
    try:
        tl = int(eng.params.TL)
        eng.begin_occ(2)
        eng.push_fastq(text, nthreads=2, occ=True, TL=tl, qmin=0)
        want = eng.finish()
        assert sum(len(ids) for ids, _ in want) > 0
        for payload in (100, 65280):
            inp = str(tmp_path / ("lowcov_%d.fq.gz" % payload))
            open(inp, "wb").write(bz.write_bgzf(text, payload=payload, level=6)[0])
            for chunk_bytes in (64 << 10, 0):
                eng.begin_occ(2)
                st = eng.push_bgzf_q(inp, qmin=0, chunk_bytes=chunk_bytes)
                got = eng.finish()
                assert st.text_bytes == len(text) and st.rows == text.count(b"\n") // 4 and st.bad_block == -1
                assert st.chunks > 1 if chunk_bytes else st.chunks == 1
                assert len(got) == len(want)
                for (gi, gcnt), (wi, wcnt) in zip(got, want):
                    assert np.array_equal(gi, wi) and (gcnt is None) == (wcnt is None), (payload, chunk_bytes)
    finally:
        eng.close()


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def run_cli(shuf, flags, out, inp, extra=(), env=None):
    r = subprocess.run([CLI, "dist", "-L", shuf] + list(flags) + ["-p", "4", "--quiet", "--timing", "-o", out] + list(extra) + [inp],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    routes = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return r, routes


def same_dir(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and "cofiles.stat" in fa
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def golden_text_of(case):
    kind, base, *variant = gc.CASES[case]["input"].split(":")
    v = variant[0] if variant else ""
    return bz.golden_text("fq_%s%s" % (base, "_" + v if v in ("crlf", "trunc", "nonl") else ""))


FQ_Q = sorted(c for c, e in gc.CASES.items() if "-A" not in e["flags"] and e["input"].startswith("fq:") and c in MANIFEST["cases"])
FQ_Q_CASES = [c for c in FQ_Q if longest_line(golden_text_of(c)) < 4096]  # (a terminated line of 4095 characters is 4096 bytes)
FQ_Q_LONG = [c for c in FQ_Q if c not in FQ_Q_CASES]


def test_case_selection():
    fam = lambda cs: sorted({c.split("_")[0] for c in cs})
    assert fam(FQ_Q_CASES) == ["key0", "lowcov", "qual", "ragged500"] and len(FQ_Q_CASES) >= 16
    assert FQ_Q_LONG == ["long_n2_L0K6", "long_set_L1K7"]


def check_case(case, payload, shuf_files, tmp_path, env=None, chunks=(["--inflate-chunk-kib", "64"], [])):
    entry = MANIFEST["cases"][case]
    assert not entry["aborted"]
    text = golden_text_of(case)
    inp = str(tmp_path / (case + ".fq.gz"))
    open(inp, "wb").write(bz.write_bgzf(text, payload=payload, level=6)[0])
    shuf = shuf_files(entry["shuf"])
    base = str(tmp_path / "zcat")
    r, routes = run_cli(shuf, entry["flags"], base, inp, ["--no-device-inflate"], env=env)
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    exp = os.path.join(gc.GOLDEN, "expected", case)
    for chunk in chunks:
        out = str(tmp_path / ("dev%d" % len(chunk)))
        r, routes = run_cli(shuf, entry["flags"], out, inp, ["--device-inflate"] + chunk, env=env)
        assert r.returncode == 0, r.stderr.decode()
        assert [x["route"] for x in routes] == ["device-inflate"] and "fallback" not in routes[0], "the device route was not taken"
        assert routes[0]["text_bytes"] == len(text) and routes[0]["blocks"] == (len(text) + payload - 1) // payload + 1
        assert routes[0]["rows"] == text.count(b"\n") // 4
        if chunk and len(text) > 65536:
            assert routes[0]["chunks"] > 1
        same_dir(base, out)
        for f in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), "%s: %s differs from the reference" % (case, f)
    return shuf, inp


@pytest.mark.parametrize("payload", [100, 65280])
@pytest.mark.parametrize("case", FQ_Q_CASES)
def test_cli_bgzf_q_equals_zcat_route_and_reference(case, payload, shuf_files, tmp_path):
    shuf, inp = check_case(case, payload, shuf_files, tmp_path)
    if payload == 100:  # opt-in: without the switch the same file still takes the zcat pipe
        r, routes = run_cli(shuf, MANIFEST["cases"][case]["flags"], str(tmp_path / "plain"), inp)
        assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]


def test_cli_bgzf_q_poisoned_allocations(shuf_files, tmp_path):
    """MK_POISON fills every allocation before use (read once per process: the command line is a process of its own)"""
    check_case("qual_Q54_n2_L0K6", 100, shuf_files, tmp_path, env=dict(os.environ, MK_POISON="0xA5"))


@pytest.mark.parametrize("case", FQ_Q_LONG)
def test_cli_long_reads_fall_back_to_zcat(case, shuf_files, tmp_path):
    entry = MANIFEST["cases"][case]
    text = golden_text_of(case)
    inp = str(tmp_path / (case + ".fq.gz"))
    open(inp, "wb").write(bz.write_bgzf(text, payload=65280, level=6)[0])
    out = str(tmp_path / "dev")
    r, routes = run_cli(shuf_files(entry["shuf"]), entry["flags"], out, inp, ["--device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", "long line")]  # never silent
    exp = os.path.join(gc.GOLDEN, "expected", case)
    for f in entry["files"]:
        assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), "%s: %s differs from the reference" % (case, f)


def test_cli_long_read_behind_pushed_chunks_falls_back(shuf_files, tmp_path):
    # reads cut from a 10 kb pool (30x coverage) with mostly passing qualities: -n 2 -Q 53 must keep keys, or equal directories show nothing
    rs = np.random.RandomState(5)
    pool = bytes(rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 10000))
    def rec(i, n):
        a = rs.randint(0, len(pool) - n + 1)
        return b"@r%d\n" % i + pool[a:a + n] + b"\n+\n" + bytes(rs.randint(50, 75, n, dtype=np.uint8)) + b"\n"
    text = b"".join(rec(i, 100) for i in range(3000)) + rec(3000, 6000) + b"".join(rec(i, 100) for i in range(3001, 3101))
    assert len(text) > 5 * 65536
    inp = str(tmp_path / "late_long.fq.gz")
    open(inp, "wb").write(bz.write_bgzf(text, payload=65280, level=1)[0])
    shuf = shuf_files("L1K7")
    base, out = str(tmp_path / "zcat"), str(tmp_path / "dev")
    flags = ["-n", "2", "-Q", "53"]
    r, routes = run_cli(shuf, flags, base, inp, ["--no-device-inflate"])
    assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"] and "fallback" not in routes[0]
    r, routes = run_cli(shuf, flags, out, inp, ["--device-inflate", "--inflate-chunk-kib", "64"])
    assert r.returncode == 0, r.stderr.decode()
    assert [(x["route"], x.get("fallback")) for x in routes] == [("zcat", "long line")]
    same_dir(base, out)
    assert os.path.getsize(os.path.join(out, "combco.0")) > 0


def test_cli_damaged_bgzf_q_fails_loudly(shuf_files, tmp_path):
    text = bz.golden_text("fq_ragged")
    f, table = bz.write_bgzf(text, payload=20000, level=6)
    bad = bytearray(f)
    t = table[2]
    bad[t["in_off"] + 18 + t["pay_len"] // 2] ^= 0x04
    inp = str(tmp_path / "bad.fq.gz")
    open(inp, "wb").write(bytes(bad))
    assert capi.bgzf_scan(path=inp) is not None
    out = str(tmp_path / "out")
    r, routes = run_cli(shuf_files("L1K7"), ["-n", "2"], out, inp, ["--device-inflate"])
    err = r.stderr.decode()
    assert r.returncode != 0 and routes == []  # a damaged member is no fall-back
    assert "bad.fq.gz" in err and "block 2" in err, err
    assert not os.path.exists(os.path.join(out, "cofiles.stat"))
