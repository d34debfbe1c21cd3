"""BGZF-compressed FASTQ on the device: the inflate kernel against zlib byte for byte, the device framer against mk_fastq_frame,
and `metakssd dist -A` on re-compressed golden inputs against the `zcat -fc` route and the committed reference output"""
import filecmp
import gzip
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bgzf_util as bz
import golden_cases as gc
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
MANIFEST = json.load(open(os.path.join(gc.GOLDEN, "manifest.json")))
RS = np.random.RandomState(77)
RANDOM = bytes(RS.randint(0, 256, 200000, dtype=np.uint8))


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


def check_inflate(infl, f, table, want):
    assert gzip.decompress(f) == want  # the fixture itself
    got, st = infl.blocks(f, table)
    assert st == [0] * len(table), [(i, capi.lib.mk_inflate_status_text(s).decode()) for i, s in enumerate(st) if s]
    assert got == want


# ---- inflate against zlib ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level,strategy", [("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED),
                                                 ("dynamic1", 1, zlib.Z_DEFAULT_STRATEGY), ("dynamic9", 9, zlib.Z_DEFAULT_STRATEGY),
                                                 ("huffman_only", 6, zlib.Z_HUFFMAN_ONLY)])
@pytest.mark.parametrize("text", ["fq_dense", "fq_homo"])
def test_inflate_block_types(infl, name, level, strategy, text):
    data = bz.golden_text(text)
    for payload in (65280, 1000):
        f, table = bz.write_bgzf(data, payload=payload, level=level, strategy=strategy)
        assert capi.bgzf_scan(f) == table
        check_inflate(infl, f, table, data)


def test_inflate_several_deflate_blocks_in_one_member(infl):
    data = bz.golden_text("fq_ragged")[:60000]
    members = [bz.member(data, 6, flush_at=(1, 777, 20000, 20000, 50001)), bz.member(data[:5000], 0, flush_at=(100, 2500)),
               bz.member(data[:30000], 6, zlib.Z_FIXED, flush_at=(15000,)), bz.EOF_MARKER]
    f = b"".join(members)
    table = capi.bgzf_scan(f)
    assert [t["isize"] for t in table] == [60000, 5000, 30000, 0]
    check_inflate(infl, f, table, data + data[:5000] + data[:30000])


def test_inflate_overlapping_and_far_matches(infl):
    one = b"Q" * 65536                                        # distance 1, length 258: every copy overlaps itself
    pat = (b"ACGTTGCAAT" * 7000)[:65536]                      # distance 10 below the length
    two = bytes(RS.randint(0, 256, 3, dtype=np.uint8)) * 20000  # distance 3
    far, far_data = bz.max_distance_member(RANDOM[:32768])    # distance 32768, the largest there is
    half = RANDOM[:32000] + RANDOM[:32000]                    # the farthest zlib itself reaches
    members = [bz.member(one, 6), bz.member(pat, 9), bz.member(two, 1), far, bz.member(half, 9), bz.EOF_MARKER]
    f = b"".join(members)
    table = capi.bgzf_scan(f)
    assert table is not None and table[0]["isize"] == 65536
    check_inflate(infl, f, table, one + pat + two + far_data + half)


def test_inflate_random_bytes_tiny_and_empty_members(infl):
    sizes = [65280, 1, 0, 2, 3, 63, 64, 65, 255, 256, 257, 4097, 0, 65280]
    data = RANDOM[:sum(sizes)]
    for level in (6, 0):
        f, table = bz.write_bgzf(data, sizes=sizes, level=level)
        check_inflate(infl, f, table, data)
    # text of every size around the CRC's serial / parallel switch and the slice padding, in one launch
    sizes = list(range(250, 330)) + [4 * 64 + k for k in range(5)] + [1000, 1023, 1024, 1025]
    text = (bz.golden_text("fq_ragged") * 2)[:sum(sizes)]
    f, table = bz.write_bgzf(text, sizes=sizes, level=6)
    check_inflate(infl, f, table, text)


def test_inflate_many_members_more_than_one_workgroup(infl):
    data = bz.golden_text("fq_mix")[:300000]
    f, table = bz.write_bgzf(data, payload=997, level=6)  # 301 members + the end marker: no multiple of the waves per workgroup
    assert len(table) % 4 != 0
    check_inflate(infl, f, table, data)


def test_inflate_damaged_members_give_a_status_not_a_fault(infl):
    data = bz.golden_text("fq_ragged")[:40000]
    f, table = bz.write_bgzf(data, payload=10000, level=6)
    # one payload bit flipped in member 1, CRC field of member 2 altered, ISIZE of member 3 one smaller
    bad = bytearray(f)
    bad[table[1]["in_off"] + 18 + 700] ^= 0x10
    t = [dict(x) for x in table]
    t[2]["crc32"] ^= 1
    t[3]["isize"] -= 1
    got, st = infl.blocks(bytes(bad), t)
    assert st[0] == 0 and st[4] == 0
    assert st[1] != 0
    assert st[2] == capi.MK_INFL_CRC
    assert st[3] == capi.MK_INFL_OUTPUT_LEN
    assert got[:10000] == data[:10000] and got[20000:30000] == data[20000:30000]
    # a payload cut short: the stream runs out of input
    t = [dict(x) for x in table]
    t[0]["pay_len"] //= 2
    _, st = infl.blocks(f, t)
    assert st[0] in (capi.MK_INFL_INPUT, capi.MK_INFL_BAD_CODE, capi.MK_INFL_BAD_DISTANCE, capi.MK_INFL_OUTPUT_LEN, capi.MK_INFL_BAD_LENGTHS,
                     capi.MK_INFL_BAD_BLOCK) and st[1:] == [0] * (len(table) - 1)
    # reserved block type 3, and a stored block whose NLEN is wrong
    raw3 = bytes([0x07, 0x00])
    stored = bytearray(bz.deflate_raw(b"ACGT" * 8, 0))
    stored[3] ^= 0xFF
    f2 = bz.member_raw(raw3, b"") + bz.member_raw(bytes(stored), b"ACGT" * 8)
    _, st = infl.blocks(f2, capi.bgzf_scan(f2))
    assert st == [capi.MK_INFL_BAD_BLOCK, capi.MK_INFL_BAD_BLOCK]


# ---- hand-made deflate streams: what no zlib compressor emits (tests/test_bgzf_host.py holds every one of them against zlib) ------------
def check_cases(infl, cases):
    """one launch: a member per case, the end marker last; a failing member is named"""
    f = b"".join(bz.member_raw(c[1], c[2]) for c in cases) + bz.EOF_MARKER
    table = capi.bgzf_scan(f)
    assert table is not None and [t["isize"] for t in table] == [len(c[2]) for c in cases] + [0]
    got, st = infl.blocks(f, table)
    bad = [(c[0], capi.lib.mk_inflate_status_text(s).decode()) for c, s in zip(cases, st) if s]
    bad += [c[0] for c, t in zip(cases, table) if got[t["out_off"]:t["out_off"] + t["isize"]] != c[2]]
    assert not bad, bad
    check_inflate(infl, f, table, b"".join(c[2] for c in cases))


def test_inflate_code_lengths_1_to_15_and_both_sides_of_the_tables(infl):
    check_cases(infl, bz.legal_long_codes())


def test_inflate_degenerate_distance_sets_and_an_empty_block(infl):
    check_cases(infl, bz.legal_degenerate())


def test_inflate_code_length_runs_across_the_alphabets_and_hclen(infl):
    check_cases(infl, bz.legal_header_ops())


def test_inflate_length_258_as_symbol_285_and_as_284(infl):
    check_cases(infl, bz.legal_length_258())


def test_inflate_literal_runs_around_the_register_then_a_match(infl):
    check_cases(infl, bz.legal_literal_runs())


def test_inflate_random_bytes_through_huffman_tables(infl):
    cases = bz.legal_random(RANDOM)
    assert [bz.first_block_type(c[1]) for c in cases] == [2, 2, 2]
    check_cases(infl, cases)


def test_inflate_maximal_tokens_at_every_phase_of_the_window(infl):
    f, text, phases = bz.sweep_file(RANDOM)
    bz.assert_sweep_phases(phases)  # computed from the written bits, whatever the kernel does
    table = capi.bgzf_scan(f)
    assert table is not None and len(table) == len(phases) + 2
    assert [(t["pay_off"], t["in_off"]) for t in table[1:-1]] == [(p, i) for _, _, p, i in phases]
    got, st = infl.blocks(f, table)
    bad = [(ph, s) for ph, s, t in zip(phases, st[1:], table[1:]) if s or got[t["out_off"]:t["out_off"] + t["isize"]] != text[t["out_off"]:t["out_off"] + t["isize"]]]
    assert not bad, bad[:8]
    check_inflate(infl, f, table, text)


def test_inflate_malformed_streams_give_their_status_and_spare_the_neighbours(infl):
    cases = bz.illegal_cases()
    goods = [bz.golden_text("fq_ragged")[300 * i:300 * i + 250 + i] for i in range(len(cases) + 1)]
    f = bz.member(goods[0])
    for c, g in zip(cases, goods[1:]):
        f += c[1] + bz.member(g, 1 + len(g) % 9)
    f += bz.EOF_MARKER
    table = capi.bgzf_scan(f)
    assert table is not None and len(table) == 2 * len(cases) + 2
    got, st = infl.blocks(f, table)
    for i, g in enumerate(goods):
        t = table[2 * i]
        assert st[2 * i] == 0 and got[t["out_off"]:t["out_off"] + t["isize"]] == g, "the good member %d" % i
    wrong = []
    for i, (name, member, raw, level, classes) in enumerate(cases):
        s = st[2 * i + 1]
        if s == 0 or s not in [getattr(capi, "MK_INFL_" + c) for c in classes]:
            wrong.append((name, capi.lib.mk_inflate_status_text(s).decode(), classes))
    assert not wrong, wrong


# ---- the framer against the host ---------------------------------------------------------------------------------------------------
def host_rows(text):
    """mk_fastq_frame over the whole text, final: the sequence lines with their '\\n', and the bytes consumed"""
    rows, n, used, rc = capi.fastq_frame(text, 4096, final=True)
    assert rc == 0
    out = []
    for i in range(n):
        r = rows[i * 4096:(i + 1) * 4096].tobytes()
        out.append(r[:r.index(b"\n") + 1])
    return out, used


def device_rows(infl, pieces):
    """the pieces framed one after the other, what lies behind a piece's last complete record carried in front of the next"""
    out, carry = [], b""
    for i, piece in enumerate(pieces):
        buf = carry + piece
        rows, stride, n, used, longest, rc = infl.frame(buf, final=i + 1 == len(pieces))
        assert rc == 0 and used <= len(buf)
        want = 0
        for k in range(n):
            r = rows[k * stride:(k + 1) * stride].tobytes()
            line = r[:r.index(b"\n") + 1]
            assert r[len(line):] == b"\0" * (stride - len(line))
            out.append(line)
            want = max(want, len(line))
        if n:
            need = (want + 15) & ~15
            assert stride == need + (16 if need % 128 == 0 and need < 4096 else 0)  # MK_ROW_PITCH(longest sequence line)
        carry = buf[used:]
    return out, sum(len(p) for p in pieces) - len(carry)


FRAME_TEXTS = ["fq_ragged", "fq_ragged_nonl", "fq_ragged_trunc", "fq_ragged_crlf", "fq_mix", "fq_homo"]


@pytest.fixture(scope="module")
def host_framed():
    return {name: host_rows(bz.golden_text(name)) for name in FRAME_TEXTS}


@pytest.mark.parametrize("name", FRAME_TEXTS)
def test_framer_whole_text_equals_host(infl, host_framed, name):
    text = bz.golden_text(name)
    want, used = host_framed[name]
    rows, stride, n, consumed, longest, rc = infl.frame(text, final=True)
    assert rc == 0 and n == len(want) and consumed == used == len(text)
    hrows, hn, hused, hrc = capi.fastq_frame(text, stride, final=True)  # the same stride: the rows byte for byte, padding included
    assert hrc == 0 and hn == n and np.array_equal(hrows, rows)
    parts = text.split(b"\n")
    assert longest == max([len(x) + 1 for x in parts[:-1]] + [len(parts[-1])])  # a terminated line counts its '\n', as mk_line() does


@pytest.mark.parametrize("name", FRAME_TEXTS)
@pytest.mark.parametrize("chunk", [1024, 4097])
def test_framer_chunked_equals_host(infl, host_framed, name, chunk):
    text = bz.golden_text(name)
    if name == "fq_mix":
        text = text[:200000]
        want, used = host_rows(text)
    else:
        want, used = host_framed[name]
    got, total = device_rows(infl, [text[a:a + chunk] for a in range(0, len(text), chunk)])
    assert got == want and total == used


def test_framer_every_cut_of_a_short_file(infl):
    recs = [b"@r0 x\nACGTACGTAC\n+\nIIIIIIIIII\n", b"@r1\nA\n+r1\nI\n", b"@r2\n\n+\n\n", b"@r3\r\nACGTTT\r\n+\r\nIIIIII\r\n"]
    for tail in (b"", b"@r4\nACG\n+\nII", b"@r4\nACG\n+\n", b"@r4\nACG", b"@r4\nACG\n+", b"\n", b"\n\n\n\nX"):
        text = b"".join(recs) + tail
        want, used = host_rows(text)
        assert infl.frame(text, final=True)[2] == len(want)
        limit = len(recs[0]) + len(recs[1]) + 2 if tail else len(text)
        for cut in list(range(0, limit)) + [len(text) - 1, len(text)]:
            got, total = device_rows(infl, [text[:cut], text[cut:]])
            assert got == want and total == used == len(text), (tail, cut)
    # not final: only records whose fourth line is terminated count, the rest is left for the next call
    text = b"".join(recs) + b"@r4\nACG\n+\nII"
    rows, stride, n, consumed, longest, rc = infl.frame(text, final=False)
    assert rc == 0 and n == 4 and consumed == len(b"".join(recs))
    assert infl.frame(b"@r\nAC", final=False)[2:4] == (0, 0) and infl.frame(b"", final=True)[2:4] == (0, 0)


def test_framer_long_lines(infl):
    rec = lambda n: b"@long\n" + b"ACGT" * (n // 4) + b"ACGT"[:n % 4] + b"\n+\n" + b"I" * 10 + b"\n"
    short = b"@s\nACGT\n+\nIIII\n"
    text = short * 50 + rec(4094) + short * 50  # the widest row there is
    rows, stride, n, consumed, longest, rc = infl.frame(text, final=True)
    assert rc == 0 and stride == 4096 and n == 101 and longest == 4095
    hrows, hn, hused, hrc = capi.fastq_frame(text, 4096, final=True)
    assert hrc == 0 and hn == n and np.array_equal(hrows, rows)
    for bad in (short * 50 + rec(4095) + short, short + b"@" + b"h" * 4094 + b"\nACGT\n+\nIIII\n", rec(5000) * 3):
        assert capi.fastq_frame(bad, 4096, final=True)[3] == capi.MK_ERR_FORMAT
        assert infl.frame(bad, final=True)[5] == capi.MK_ERR_FORMAT


PORTION = 1 << 20  # MK_FRAME_PORTION (mk_inflate.hip): row bytes the two entries take back at a time
PITCH = 160        # MK_ROW_PITCH(151): the first record below has 150 bases, none has more


def portion_text(nrec):
    """nrec records of 100 to 150 bases, the first of 150; qualities on both sides of -Q 54"""
    rs = np.random.RandomState(nrec)
    lens = rs.randint(100, 151, nrec)
    lens[0] = 150
    bases = np.frombuffer(b"ACGTN", dtype=np.uint8)[rs.randint(0, 5, int(lens.sum()))].tobytes()
    quals = rs.randint(33, 75, int(lens.sum()), dtype=np.uint8).tobytes()
    out, at = [], 0
    for i, n in enumerate(lens):
        out.append(b"@r%d\n%s\n+\n%s\n" % (i, bases[at:at + n], quals[at:at + n]))
        at += n
    return b"".join(out)


@pytest.mark.parametrize("nrec", [20000, PORTION // PITCH, PORTION // PITCH + 1])
def test_framer_rows_in_more_than_one_portion(infl, nrec):
    """the portion loop of mk_fq_framer::rows at sizes where it takes three trips (the last one partial), exactly one (a second
    portion would be empty), and two (one row in the second), for both readers' rules, against the host framers"""
    text = portion_text(nrec)
    if nrec == 20000:
        assert nrec * PITCH > 2 * PORTION  # cannot pass by fitting in one portion
    else:
        assert (nrec * PITCH <= PORTION) == (nrec == PORTION // PITCH) and (nrec + 1) * PITCH > PORTION
    rows, stride, n, consumed, longest, rc = infl.frame(text, final=True)
    assert rc == 0 and (stride, n, consumed) == (PITCH, nrec, len(text))
    hrows, hn, hused, hrc = capi.fastq_frame(text, stride, final=True)
    assert hrc == 0 and (hn, hused) == (n, consumed) and np.array_equal(hrows, rows)
    rows, stride, n, nrecords, consumed, longest, rc = infl.frame_q(text, qmin=54, final=True)
    assert rc == 0 and (stride, n, nrecords, consumed) == (PITCH, nrec, nrec, len(text))
    hrows, hn, hrec, hused, hrc = capi.fastq_frame_q(text, stride, 22, qmin=54, final=True)
    assert hrc == 0 and (hn, hrec, hused) == (n, nrecords, consumed) and np.array_equal(hrows, rows)
    assert (rows == ord("N")).sum() > (np.frombuffer(text, dtype=np.uint8) == ord("N")).sum()  # the mask was at work


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


def run_cli(shuf, flags, out, inp, extra=()):
    r = subprocess.run([CLI, "dist", "-L", shuf] + list(flags) + ["-p", "4", "--quiet", "--timing", "-o", out] + list(extra) + [inp],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
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


FQ_A_CASES = sorted(c for c, e in gc.CASES.items() if e["flags"] == ["-A"] and e["input"].startswith("fq:") and c in MANIFEST["cases"])


@pytest.mark.parametrize("payload", [100, 65280])
@pytest.mark.parametrize("case", FQ_A_CASES)
def test_cli_bgzf_equals_zcat_route_and_reference(case, payload, shuf_files, tmp_path):
    entry = MANIFEST["cases"][case]
    assert not entry["aborted"]
    text = golden_text_of(case)
    inp = str(tmp_path / (case + ".fq.gz"))
    open(inp, "wb").write(bz.write_bgzf(text, payload=payload, level=6)[0])
    shuf = shuf_files(entry["shuf"])
    base = str(tmp_path / "zcat")
    r, routes = run_cli(shuf, entry["flags"], base, inp, ["--no-device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["zcat"]
    exp = os.path.join(gc.GOLDEN, "expected", case)
    for chunk in (["--inflate-chunk-kib", "64"], []):
        out = str(tmp_path / ("dev%d" % len(chunk)))
        r, routes = run_cli(shuf, entry["flags"], out, inp, chunk)
        assert r.returncode == 0, r.stderr.decode()
        assert [x["route"] for x in routes] == ["device-inflate"], "the device route was not taken"  # no silent fall-back
        assert routes[0]["text_bytes"] == len(text) and routes[0]["blocks"] == (len(text) + payload - 1) // payload + 1
        if chunk and len(text) > 65536:
            assert routes[0]["chunks"] > 1
        same_dir(base, out)
        for f in entry["files"]:
            assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), "%s: %s differs from the reference" % (case, f)


def test_cli_other_inputs_keep_the_zcat_route(shuf_files, tmp_path):
    text = bz.golden_text("fq_ragged")
    shuf = shuf_files("L1K7")
    # a .gz that is not BGZF
    plain = str(tmp_path / "ragged500_gz_L1K7.fq.gz")
    with gzip.GzipFile(plain, "wb", mtime=0) as f:
        f.write(text)
    out = str(tmp_path / "plain")
    r, routes = run_cli(shuf, ["-A"], out, plain)
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["zcat"]
    exp = os.path.join(gc.GOLDEN, "expected", "ragged500_gz_L1K7")
    for f in MANIFEST["cases"]["ragged500_gz_L1K7"]["files"]:
        assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), f
    # a BGZF file on the -n / -Q reader
    inp = str(tmp_path / "bg.fq.gz")
    open(inp, "wb").write(bz.write_bgzf(text, payload=5000)[0])
    a, b = str(tmp_path / "n2"), str(tmp_path / "n2_no")
    r, routes = run_cli(shuf, ["-n", "2"], a, inp)
    assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"]
    r, routes = run_cli(shuf, ["-n", "2"], b, inp, ["--no-device-inflate"])
    assert r.returncode == 0 and [x["route"] for x in routes] == ["zcat"]
    same_dir(a, b)


@pytest.mark.parametrize("damage", ["bit", "crc", "isize"])
def test_cli_damaged_bgzf_fails_loudly(damage, shuf_files, tmp_path):
    text = bz.golden_text("fq_ragged")
    f, table = bz.write_bgzf(text, payload=20000, level=6)
    bad = bytearray(f)
    t = table[2]
    if damage == "bit":
        bad[t["in_off"] + 18 + t["pay_len"] // 2] ^= 0x04
    elif damage == "crc":
        struct.pack_into("<I", bad, t["in_off"] + t["in_len"] - 8, t["crc32"] ^ 0x8000)
    else:
        struct.pack_into("<I", bad, t["in_off"] + t["in_len"] - 4, t["isize"] - 1)
    inp = str(tmp_path / "bad.fq.gz")
    open(inp, "wb").write(bytes(bad))
    assert capi.bgzf_scan(path=inp) is not None
    out = str(tmp_path / "out")
    r, routes = run_cli(shuf_files("L1K7"), ["-A"], out, inp)
    err = r.stderr.decode()
    assert r.returncode != 0 and routes == []
    assert "bad.fq.gz" in err and "block 2" in err, err
    if damage == "crc":
        assert "CRC mismatch" in err
    if damage == "isize":
        assert "output length" in err
    assert not os.path.exists(os.path.join(out, "cofiles.stat"))


def test_cli_hand_written_members_equal_zcat_route_and_reference(shuf_files, tmp_path):
    case = "ragged500_L1K7"
    entry = MANIFEST["cases"][case]
    text = golden_text_of(case)
    assert text == bz.golden_text("fq_ragged") and entry["flags"] == ["-A"]
    inp = str(tmp_path / "hand.fq.gz")
    open(inp, "wb").write(bz.hand_bgzf(text, 4096))
    shuf = shuf_files(entry["shuf"])
    base, out = str(tmp_path / "zcat"), str(tmp_path / "dev")
    r, routes = run_cli(shuf, entry["flags"], base, inp, ["--no-device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["zcat"]
    r, routes = run_cli(shuf, entry["flags"], out, inp)
    assert r.returncode == 0, r.stderr.decode()
    assert [x["route"] for x in routes] == ["device-inflate"]
    assert routes[0]["text_bytes"] == len(text) and routes[0]["blocks"] == (len(text) + 4095) // 4096 + 1
    same_dir(base, out)
    exp = os.path.join(gc.GOLDEN, "expected", case)
    for f in entry["files"]:
        assert filecmp.cmp(os.path.join(exp, f), os.path.join(out, f), shallow=False), f
