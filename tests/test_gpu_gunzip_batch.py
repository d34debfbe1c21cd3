"""A batch of single-member gzip files inflated by many wavefronts per file (mk_inflate_members_split,
mk_sketch_batch_begin_gunzip, `metakssd dist --device-gunzip genomes_dir/`): every text against zlib byte for byte,
every file's piece list against tests/gunzip_model.py, damaged files with their exact status between untouched neighbours, guard
bytes around every text's place, the engine's batch against the text batch, and the command line against its own zcat route."""
import functools
import gzip
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_util as bu
import golden_cases as gc
import gunzip_batch_worker as gbw
import gunzip_model as gm
import gz_batch_worker as gw
import util_inputs as ui
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
TEXT = bu.golden_text("fq_ragged")
STREAMS = gm.legal_streams(TEXT)
BY_NAME = {n: (raw, text) for n, raw, text in STREAMS}
RATIO = 1040  # no deflate stream gives more than 1032 bytes a compressed byte: with this R no legal piece can meet its capacity
FILL = 0xC3   # what the text buffer holds where no file has its place
RANDOM = bytes(np.random.RandomState(31).randint(0, 256, 40000, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def model(raw, span, ratio=RATIO):
    return gm.run(raw, span, ratio)


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


def lay(streams, texts, fronts=None):
    """raw deflate streams side by side -> (comp, table).  fronts[i]: bytes in front of stream i (default: one, so that the offsets
    are odd).  Places are 1 KiB apart at least and never touch: the gaps are the guards."""
    comp, table, out = b"", [], 64
    for i, (s, t) in enumerate(zip(streams, texts)):
        comp += b"\xEE" if fronts is None else fronts[i]
        table.append({"pay_off": len(comp), "pay_len": len(s), "out_off": out, "isize": len(t), "crc32": zlib.crc32(t)})
        comp += s + b"\xEE" * 8  # (where a file's trailer would lie)
        out += (len(t) + 1023) // 1024 * 1024 + 64
    return comp, table


def guards_ok(got, table):
    """every byte outside the places is what the caller put there"""
    mask = np.ones(len(got), dtype=bool)
    for e in table:
        mask[e["out_off"]:e["out_off"] + e["isize"]] = False
    return bool((np.frombuffer(got, dtype=np.uint8)[mask] == FILL).all())


def split(infl, comp, table, span, ratio=RATIO):
    got, res, pieces = infl.members(comp, table, split=dict(span_bytes=span, ratio=ratio), fill=FILL)
    assert guards_ok(got, table), "a write outside the files' places"
    return got, res, pieces


def place(got, e):
    return got[e["out_off"]:e["out_off"] + e["isize"]]


def check_good(got, res, pieces, table, streams, texts, span, ratio=RATIO, which=None):
    for i in (range(len(table)) if which is None else which):
        e, s, t = table[i], streams[i], texts[i]
        assert res[i][0] == 0, "file %d: %s" % (i, capi.lib.mk_gunzip_status_text(res[i][0]).decode())
        assert res[i] == (0, e["pay_len"], len(t), zlib.crc32(t)), i
        assert place(got, e) == t, "file %d: text differs" % i
        mst, mtext, want = model(s, span, ratio)
        assert mst == gm.OK and mtext == t
        assert pieces[i] == want, "file %d: pieces differ from the model's" % i
        assert all(0 <= start < max(1, 8 * e["pay_len"]) for start, _ in pieces[i]) and sum(n for _, n in pieces[i]) == len(t)
        assert [p[0] for p in pieces[i]] == sorted(set(p[0] for p in pieces[i])), i


# ---- 1: text and pieces, many files in one launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [256, 1024])
def test_every_legal_stream_side_by_side(infl, span):
    streams, texts = [raw for _, raw, _ in STREAMS], [t for _, _, t in STREAMS]
    for s, t in zip(streams, texts):
        assert zlib.decompress(s, -15) == t  # the fixture itself
    comp, table = lay(streams, texts)
    got, res, pieces = split(infl, comp, table, span)
    check_good(got, res, pieces, table, streams, texts, span)
    _, one_wave = infl.members(comp, table)
    assert res == one_wave  # mk_inflate_members on the same table
    by = {n: len(p) for (n, _, _), p in zip(STREAMS, pieces)}
    if span == 256:
        assert all(by[n] > 20 for n in ("l1_m1", "l6_m1", "l9_m1", "repeat_20k_x10", "sync_flush", "full_flush")), by
    assert all(by[n] == 1 for n in ("fixed_only", "stored_only", "empty", "no_complete_record", "l6_m9")), by


# ---- 2: file edges ----------------------------------------------------------------------------------------------------------------------
def stream_of_len(target):
    """a deflate stream of exactly `target` bytes: a prefix of TEXT at some level, or stored bytes"""
    for lv in (6, 1, 9):
        for n in range(target, 6 * target):
            s = gm.deflate(TEXT[:n], lv, 1)
            if len(s) == target:
                return s, TEXT[:n]
            if len(s) > target + 16:
                break
    s = gm.deflate(RANDOM[:target - 5], 0)
    assert len(s) == target
    return s, RANDOM[:target - 5]


def test_file_edges_in_one_launch(infl):
    S = 256
    cases = [gm.deflate(b"@r1\nACGT"), stream_of_len(2 * S)[0], stream_of_len(3 * S + 1)[0], BY_NAME["stored_only"][0], BY_NAME["repeat_20k_x10"][0],
             stream_of_len(S)[0], stream_of_len(S + 1)[0]]
    texts = [zlib.decompress(s, -15) for s in cases]
    assert len(cases[0]) < S and len(cases[1]) == 2 * S and len(cases[2]) % S == 1
    comp, table = lay(cases, texts)
    got, res, pieces = split(infl, comp, table, S)
    check_good(got, res, pieces, table, cases, texts, S)
    assert len(pieces[0]) == 1 and len(pieces[3]) == 1  # shorter than a span; stored only: no candidate anywhere
    rep = pieces[4]
    assert len(rep) > 20 and max(n for _, n in rep) < 32768  # matches reach across several piece boundaries
    for e, p in zip(table, pieces):  # no piece starts at or ends on a bit of the next file: the last ends with the payload, the lengths say
        assert p[-1][0] < 8 * e["pay_len"] and sum(n for _, n in p) == e["isize"]


# ---- 3: every payload alignment -------------------------------------------------------------------------------------------------------
def test_every_payload_alignment_with_a_different_neighbour_in_front(infl):
    raw, text = BY_NAME["l6_m1"]
    streams, texts, fronts, at = [], [], [], 0
    for k in range(16):
        nb_raw, nb_text = STREAMS[k % 9][1], STREAMS[k % 9][2]
        for s, t, want in ((nb_raw, nb_text, None), (raw, text, k)):
            pad = b"\xEE" if want is None else b"\xEE" * ((want - at) % 16)
            fronts.append(pad)
            at += len(pad) + len(s) + 8
            streams.append(s)
            texts.append(t)
    comp, table = lay(streams, texts, fronts)
    assert [table[2 * k + 1]["pay_off"] % 16 for k in range(16)] == list(range(16))
    got, res, pieces = split(infl, comp, table, 1024)
    check_good(got, res, pieces, table, streams, texts, 1024)
    assert all(pieces[2 * k + 1] == pieces[1] and place(got, table[2 * k + 1]) == text for k in range(16))


# ---- 4: statuses among good neighbours ------------------------------------------------------------------------------------------------
def expected_status(raw, isize, crc, span, ratio):
    """the fold of 4.16 over the model's pieces: the first piece with a status, unless the lengths in front of it pass ISIZE"""
    st, text, pieces = model(raw, span, ratio)
    total = 0
    for k, (_, n) in enumerate(pieces):
        if st and k == len(pieces) - 1:
            return st
        total += n
        if total > isize:
            return gm.OUTPUT_LEN
    return gm.OUTPUT_LEN if total != isize else gm.CRC if zlib.crc32(text) != crc else gm.OK


def missed_stream():
    """tests/test_gpu_gunzip.py's false candidate: a stored block whose bytes hold, just behind the start of span 1 (1024-byte
    spans), the image of a valid non-final dynamic block header; then a final block"""
    w = bu.BitWriter()
    bu.dynamic_block(w, bu.spread(257, {65: 2, 66: 2, 67: 2, 256: 2}), [1, 1], [], 0, stop="ops")
    image = w.done()
    data = bytearray(b"\xff" * 3000)
    at = 1030 - 5  # the stored bytes start at payload byte 5
    data[at:at + len(image)] = image
    w = bu.BitWriter()
    bu.stored_block(w, bytes(data), 0)
    bu.fixed_block(w, list(b"@r\nACGT\n+\nIIII\n"), 1)
    raw = w.done()
    assert gm.header_valid(raw, 8 * 1030) and gm.find_candidates(raw, 1024)[0] == 8 * 1030
    return raw, zlib.decompress(raw, -15)


def damaged_cases():
    raw, text = BY_NAME["l6_m1"]
    crc, n = zlib.crc32(text), len(text)
    flipped = bytearray(raw); flipped[len(raw) // 2] ^= 0x10
    first, second = text[:3000], text[3000:]
    two = gm.deflate(first) + struct.pack("<II", zlib.crc32(first), len(first)) + bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3]) + gm.deflate(second)
    mraw, mtext = missed_stream()
    return [("flipped_bit", bytes(flipped), n, crc, RATIO, None), ("cut_short", raw[:len(raw) // 2], n, crc, RATIO, gm.INPUT),
            ("wrong_crc", raw, n, crc ^ 0x00100000, RATIO, gm.CRC), ("isize_one_small", raw, n - 1, crc, RATIO, gm.OUTPUT_LEN),
            ("isize_one_large", raw, n + 1, crc, RATIO, gm.OUTPUT_LEN), ("two_members", two, len(second), zlib.crc32(second), RATIO, gm.TRAILING),
            ("false_candidate", mraw, len(mtext), zlib.crc32(mtext), RATIO, gm.MISSED), ("ratio_one", raw, n, crc, 1, gm.CAPACITY)]


@pytest.mark.parametrize("case", damaged_cases(), ids=lambda c: c[0])
def test_a_damaged_file_between_two_good_ones(infl, case):
    name, bad, isize, crc, ratio, want = case
    span = 1024
    # neighbours that are fine at this ratio too: stored bytes give fewer symbols than they take
    a = (gm.deflate(RANDOM[:30000], 0), RANDOM[:30000]) if ratio == 1 else BY_NAME["l1_m2"]
    b = (gm.deflate(RANDOM[100:9000], 0), RANDOM[100:9000]) if ratio == 1 else BY_NAME["sync_flush"]
    streams, texts = [a[0], bad, b[0]], [a[1], b"\0" * isize, b[1]]
    comp, table = lay(streams, texts)
    table[1]["crc32"] = crc
    expect = expected_status(bad, isize, crc, span, ratio)
    assert expect != gm.OK and (want is None or expect == want), (expect, want)
    got, res, pieces = split(infl, comp, table, span, ratio)
    assert res[1][0] == expect, "%s, not %s" % (capi.lib.mk_gunzip_status_text(res[1][0]).decode(), capi.lib.mk_gunzip_status_text(expect).decode())
    check_good(got, res, pieces, table, streams, texts, span, ratio, which=(0, 2))
    # the same launch without the damaged file: no byte outside its place differs
    alone, res2, _ = split(infl, comp, [table[0], table[2]], span, ratio)
    assert [r[0] for r in res2] == [0, 0]
    e = table[1]
    alone = alone + bytes([FILL]) * (len(got) - len(alone))
    assert got[:e["out_off"]] == alone[:e["out_off"]] and got[e["out_off"] + isize:] == alone[e["out_off"] + isize:]


# ---- 5, 6: the engine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tab_bits", [0, 9])
def test_gunzip_batch_equals_text_batch(shufs, tab_bits):
    gbw.check_parity(capi, shufs("L1K7"), tab_bits)


@pytest.mark.parametrize("poison", ["0xA5", "0x43"])
def test_gunzip_batch_equals_text_batch_under_poison(poison):
    """MK_POISON fills every allocation before use (read once per process: a process of its own)"""
    env = dict(os.environ, MK_POISON=poison)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gunzip_batch_worker.py"), "7", "4", "1", "7", "9"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"gunzip batch parity ok" in r.stdout, r.stderr.decode()[-3000:]


def test_gunzip_batch_bad_files_leave_their_neighbours_alone(shufs):
    texts, gzs, counts = gbw.genomes()
    two = gw.gz(texts[1][:3000]) + gw.gz(texts[1])
    crc = bytearray(gzs[2]); crc[-8] ^= 0x04
    short = bytearray(gzs[0]); struct.pack_into("<I", short, len(short) - 4, len(texts[0]) - 1)
    bit = bytearray(gzs[4]); bit[len(bit) // 2] ^= 0x20
    opts = dict(span_bytes=gbw.SPAN, ratio=gbw.RATIO)
    eng = capi.Engine(shufs("L1K7"), 0)
    try:
        eng.batch_begin(texts, capi.MK_MODE_SET)
        want = eng.batch_end()
        batch = [gzs[0], two, gzs[1], bytes(crc), gzs[3], bytes(short), bytes(bit), gzs[4]]
        eng.batch_begin_gz(batch, capi.MK_MODE_SET, gunzip=opts)
        got = eng.batch_end()
        st = eng.batch_gz_status(len(batch))
        assert st[0] == st[2] == st[4] == st[7] == 0
        assert (st[1], st[3], st[5]) == (capi.MK_INFL_TRAILING, capi.MK_INFL_CRC, capi.MK_INFL_OUTPUT_LEN) and st[6] != 0
        np_ = eng.batch_gz_pieces(len(batch))
        assert [np_[i] for i in (0, 2, 4, 7)] == [counts[i] for i in (0, 1, 3, 4)]
        for i in (1, 3, 5, 6):
            assert got[i][0] == capi.MK_ERR_FORMAT and got[i][2] == []
        gw.same([got[0], got[2], got[4], got[7]], [want[0], want[1], want[3], want[4]], "good files beside bad ones")
        for refused in (dict(span_bytes=gbw.SPAN, flags=capi.MK_GUNZIP_MEMBERS), dict(span_bytes=64, ratio=65536)):
            with pytest.raises(capi.MkError) as err:  # members are out of scope in batches; the symbol buffer's bound
                eng.batch_begin_gz(gzs, capi.MK_MODE_SET, gunzip=refused)
            assert err.value.code == capi.MK_ERR_ARG
        eng.batch_begin(texts[:1], capi.MK_MODE_SET)  # the engine is still usable
        gw.same(eng.batch_end(), want[:1], "text batch after a refused gunzip batch")
    finally:
        eng.close()


# ---- 7: the command line ---------------------------------------------------------------------------------------------------------------
GUNZIP = ["--device-gunzip", "--gunzip-span-bytes", "1024"]
TWO = "g6_two.fa.gz"


@pytest.fixture(scope="module")
def shuf_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("shuf") / "L1K7.shuf")
    gc.make_shuf("L1K7", p)
    return p


@functools.lru_cache(maxsize=None)
def genome_files():
    """six .fa.gz genomes of a few hundred KB of text, and one of two members"""
    rs = np.random.RandomState(417)
    files = {}
    for i, (n, lvl) in enumerate(((250000, 6), (400000, 1), (300000, 9), (350000, 6), (260000, 1), (320000, 6))):
        text = ui.fasta_bytes([ui.rand_seq(rs, n // 2), ui.rand_seq(rs, n - n // 2)], width=60 if i % 2 else 70)
        files["g%d.fa.gz" % i] = gw.gz(text, lvl, "g%d.fa" % i if i == 3 else "")
    text = ui.fasta_bytes([ui.rand_seq(rs, 200000)])
    files[TWO] = gw.gz(text[:5000]) + gw.gz(text[5000:])
    return files


def genome_dir(d, damaged=None):
    os.makedirs(d)
    for n, b in genome_files().items():
        if n == damaged:
            b = bytearray(b)
            b[len(b) // 2] ^= 0x08
        open(os.path.join(d, n), "wb").write(bytes(b))


def run_cli(shuf, out, inputs, extra=()):
    r = subprocess.run([CLI, "dist", "-L", shuf, "-p", "4", "--quiet", "--timing", "-o", out] + list(extra) + list(inputs),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    routes = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return r, routes


def same_dir(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and "cofiles.stat" in fa
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("flags", [[], ["-u"]])
def test_cli_directory_of_gz_genomes(flags, shuf_file, tmp_path):
    d = str(tmp_path / "genomes")
    genome_dir(d)
    names = sorted(genome_files())
    base, out = str(tmp_path / "zcat"), str(tmp_path / "dev")
    r, routes = run_cli(shuf_file, base, [d], flags + ["--no-device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert sorted((os.path.basename(x["input"]), x["route"]) for x in routes) == [(n, "zcat") for n in names]
    for extra in (GUNZIP, ["--device-inflate"] + GUNZIP) if not flags else (GUNZIP,):  # --device-gunzip decides the genome route
        r, routes = run_cli(shuf_file, out, [d], flags + extra)
        assert r.returncode == 0, r.stderr.decode()
        by = {os.path.basename(x["input"]): x for x in routes}
        assert sorted(by) == names and len(routes) == len(names)
        for n in names:
            if n == TWO:  # more members than one: never silently
                assert by[n]["route"] == "zcat" and by[n]["fallback"] == capi.lib.mk_gunzip_status_text(capi.MK_INFL_TRAILING).decode(), by[n]
            else:
                assert by[n]["route"] == "device-gunzip" and by[n]["pieces"] > 1 and "fallback" not in by[n], by[n]
        same_dir(base, out)
    if not flags:
        for extra in (GUNZIP + ["--no-batch"], GUNZIP + ["--no-device-inflate"], ["--no-device-inflate"] + GUNZIP):
            r, routes = run_cli(shuf_file, out, [d], extra)
            assert r.returncode == 0, r.stderr.decode()
            assert len(routes) == len(names) and all(x["route"] == "zcat" and "fallback" not in x for x in routes), extra
            same_dir(base, out)


def test_cli_damaged_gz_genome_ends_like_the_zcat_route(shuf_file, tmp_path):
    d = str(tmp_path / "genomes")
    genome_dir(d, damaged="g1.fa.gz")
    with pytest.raises(Exception):
        gzip.decompress(open(os.path.join(d, "g1.fa.gz"), "rb").read())
    ends = []
    for name, extra in (("zcat", ["--no-device-inflate"]), ("dev", GUNZIP)):
        out = str(tmp_path / name)
        r, routes = run_cli(shuf_file, out, [d], extra)
        err = r.stderr.decode()
        assert r.returncode != 0 and "g1.fa.gz" in err and "zcat -fc" in err, err
        assert not os.path.exists(os.path.join(out, "cofiles.stat"))
        ends.append((r.returncode, [ln for ln in err.splitlines() if "g1.fa.gz" in ln and "metakssd" in ln]))
    assert ends[0] == ends[1]
