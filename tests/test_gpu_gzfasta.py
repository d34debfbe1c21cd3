"""plain gzip FASTA on the device: the inflate kernel on members of any size against zlib byte for byte, the CRC kernels against
zlib.crc32, statuses instead of faults, mk_sketch_batch_begin_gz against the text batch, and `metakssd dist --device-inflate` on a
directory of .fa.gz genomes against its own `--no-device-inflate` run (the route is off by default: DESIGN.md 4.11)"""
import gzip
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_util as bz
import golden_cases as gc
import gz_batch_worker as gw
import util_inputs as ui
from metakssd_amd import capi

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
SLICE = capi.MK_CRC_SLICE
RS = np.random.RandomState(78)
RANDOM = bytes(RS.randint(0, 256, 300000, dtype=np.uint8))
FA = ui.fasta_bytes([ui.rand_seq(np.random.RandomState(5), 198000)])[:200000]
assert len(FA) == 200000


@pytest.fixture(scope="module")
def infl():
    h = capi.Inflate(0)
    yield h
    h.close()


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return bz.deflate_raw(data, level, strategy)


def lay(streams, texts, gap=0):
    """raw deflate streams side by side (each at an odd offset) -> (comp, table); places rounded up to 1 KiB like a batch's"""
    comp, table, out = b"", [], 0
    for s, t in zip(streams, texts):
        comp += b"\xEE" * (1 + gap)
        table.append({"pay_off": len(comp), "pay_len": len(s), "out_off": out, "isize": len(t), "crc32": zlib.crc32(t)})
        comp += s
        out += (len(t) + 1023) // 1024 * 1024
    return comp, table


def check(infl, streams, texts):
    for s, t in zip(streams, texts):
        assert zlib.decompress(s, -15) == t  # the fixture itself
    comp, table = lay(streams, texts)
    got, res = infl.members(comp, table)
    for i, (t, e, (st, consumed, pos, crc)) in enumerate(zip(texts, table, res)):
        assert st == 0, "member %d: %s" % (i, capi.lib.mk_inflate_status_text(st).decode())
        assert (consumed, pos, crc) == (e["pay_len"], len(t), zlib.crc32(t)), i
        assert got[e["out_off"]:e["out_off"] + len(t)] == t, "member %d: text differs" % i


# ---- members of any size against zlib ---------------------------------------------------------------------------------------------
def test_inflate_just_above_the_bgzf_bound(infl):
    check(infl, [raw(FA[:65537]), raw(RANDOM[:65537], 0)], [FA[:65537], RANDOM[:65537]])


@pytest.mark.parametrize("level,strategy", [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY),
                                            (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED)])
def test_inflate_200000_bytes_of_fasta(infl, level, strategy):
    check(infl, [raw(FA, level, strategy)], [FA])


def test_inflate_homopolymer_and_one_byte(infl):
    homo = b"A" * 300000  # distance 1, length 258 throughout
    check(infl, [raw(homo, 9), raw(b"G"), raw(b"\n", 0)], [homo, b"G", b"\n"])


def test_inflate_70_members_of_mixed_sizes_in_one_launch(infl):
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 4097, 65535, 65536, 65537, 100003] * 5
    sizes = sizes[:70]
    texts, at = [], 0
    for i, n in enumerate(sizes):
        src = FA if i % 2 else RANDOM
        texts.append(src[at % 1000:at % 1000 + n])
        at += 37
    check(infl, [raw(t, (6, 1, 0, 9)[i % 4]) for i, t in enumerate(texts)], texts)


def test_inflate_maximal_tokens_at_window_boundaries_beyond_64k(infl):
    """bgzf_util's sweep -- every member's first maximal token (length 258, distance 24 577+, 15-bit codes, all extra bits) starts at
    every bit offset -40..40 around the input window's refills -- as plain members with 71 670 stored bytes in front: the stream is
    70 KiB longer (the window phases stay), the tokens land at output positions beyond 64 KiB and their distances reach back into
    the stored bytes"""
    f, text, phases = bz.sweep_file(RANDOM, offsets=range(-40, 41, 3), boundaries=(1024, 2048), passes=1)
    table = capi.bgzf_scan(f)
    filler = RANDOM[100000:100000 + 71670]
    w = bz.BitWriter()
    bz.stored_block(w, filler[:65535], 0)
    bz.stored_block(w, filler[65535:], 0)
    front = w.done()
    assert len(front) == 70 * 1024
    comp, members, texts, out = b"", [], [], 0
    for t, (bnd, off, pay_off, in_off) in zip(table[1:-1], phases):
        s = f[t["in_off"] + t["pay_off"]:t["in_off"] + t["pay_off"] + t["pay_len"]]
        txt = filler + text[t["out_off"]:t["out_off"] + t["isize"]]
        comp += b"\0" * ((in_off + pay_off - len(comp)) % 16)  # the payload's address keeps its residue mod 16
        assert zlib.decompress(front + s, -15) == txt
        members.append({"pay_off": len(comp), "pay_len": len(front) + len(s), "out_off": out, "isize": len(txt), "crc32": zlib.crc32(txt)})
        comp += front + s
        texts.append(txt)
        out += (len(txt) + 1023) // 1024 * 1024
    assert len(members) == 2 * 27 and all(len(t) > 65536 + 2000 for t in texts)
    got, res = infl.members(comp, members)
    for i, (m, t, r) in enumerate(zip(members, texts, res)):
        assert r == (0, m["pay_len"], len(t), zlib.crc32(t)), (i, r)
        assert got[m["out_off"]:m["out_off"] + len(t)] == t, i


# ---- the CRC kernels ------------------------------------------------------------------------------------------------------------------
def test_crc_of_every_size_class(infl):
    sizes = [1, 255, 256, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5, 2, 3, 4, 5, 63, 64, 65, 2 * SLICE]
    texts = [RANDOM[i * 13:i * 13 + n] for i, n in enumerate(sizes)]
    comp, table = lay([raw(t, 0) for t in texts], texts)
    got, res = infl.members(comp, table)
    assert [r[3] for r in res] == [zlib.crc32(t) for t in texts]
    assert [r[0] for r in res] == [0] * len(texts)


def test_crc_slices_of_neighbouring_files_interleave(infl):
    """the launch's slices: 3 of file 0, 1 of file 1, 2 of file 2 -- a workgroup's four waves work on two files at once"""
    texts = [RANDOM[:2 * SLICE + 100], RANDOM[7:7 + 50], RANDOM[500:500 + SLICE + 1], RANDOM[9:9 + 4 * SLICE]]
    comp, table = lay([raw(t, 1) for t in texts], texts)
    got, res = infl.members(comp, table)
    assert [r[3] for r in res] == [zlib.crc32(t) for t in texts] and [r[0] for r in res] == [0, 0, 0, 0]
    # one flipped bit of the trailer's CRC: that file only
    for victim in range(4):
        bad = [dict(t) for t in table]
        bad[victim]["crc32"] ^= 1 << (7 * victim)
        got2, res2 = infl.members(comp, bad)
        assert [r[0] for r in res2] == [capi.MK_INFL_CRC if i == victim else 0 for i in range(4)]
        assert got2 == got


# ---- statuses, not faults -------------------------------------------------------------------------------------------------------------
def with_neighbours(infl, stream, entry_patch, isize, crc):
    """the member under test between two good ones -> its result; both neighbours must be byte-exact"""
    a, b = FA[:70001], RANDOM[:66000]
    comp, table = lay([raw(a), stream, raw(b, 1)], [a, b"\0" * isize, b])
    table[1]["crc32"] = crc
    table[1].update(entry_patch)
    got, res = infl.members(comp, table)
    for e, t, r in ((table[0], a, res[0]), (table[2], b, res[2])):
        assert r == (0, e["pay_len"], len(t), zlib.crc32(t))
        assert got[e["out_off"]:e["out_off"] + len(t)] == t
    return res[1]


def test_two_concatenated_members_are_trailing(infl):
    first, second = FA[:30000], FA[30000:100000]
    f = gw.gz(first) + gw.gz(second)
    info = capi.gzip_scan(f)
    assert info["isize"] == len(second)
    s = f[info["pay_off"]:info["pay_off"] + info["pay_len"]]
    st, consumed, pos, _ = with_neighbours(infl, s, {}, info["isize"], info["crc32"])
    assert st == capi.MK_INFL_TRAILING
    assert pos == len(first) and consumed == len(raw(first))
    # the larger member first: its text does not fit the last trailer's ISIZE -- a status either way
    f = gw.gz(second) + gw.gz(first)
    info = capi.gzip_scan(f)
    st, _, pos, _ = with_neighbours(infl, f[info["pay_off"]:info["pay_off"] + info["pay_len"]], {}, info["isize"], info["crc32"])
    assert st == capi.MK_INFL_OUTPUT_LEN and pos <= len(first)


def test_truncated_short_and_damaged_payloads(infl):
    t = FA[:150000]
    s = raw(t)
    st, consumed, pos, _ = with_neighbours(infl, s[:len(s) // 2], {}, len(t), zlib.crc32(t))
    assert st == capi.MK_INFL_INPUT and pos < len(t) and consumed <= len(s) // 2
    st, _, pos, _ = with_neighbours(infl, s, {}, len(t) - 1, zlib.crc32(t))  # ISIZE one short
    assert st == capi.MK_INFL_OUTPUT_LEN and pos <= len(t) - 1
    st, _, pos, _ = with_neighbours(infl, s, {}, len(t) + 1, zlib.crc32(t))  # ISIZE one long
    assert st == capi.MK_INFL_OUTPUT_LEN and pos == len(t)
    for at, bit in ((len(s) // 3, 0x10), (len(s) - 40, 0x01), (20, 0x80)):
        bad = bytearray(s)
        bad[at] ^= bit
        st, _, pos, _ = with_neighbours(infl, bytes(bad), {}, len(t), zlib.crc32(t))
        assert st != 0 and pos <= len(t)


# ---- batches through the ABI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tab_bits", [0, 9])
def test_gz_batch_equals_text_batch(shufs, tab_bits):
    gw.check_parity(capi, shufs("L1K7"), tab_bits)


@pytest.mark.parametrize("poison", ["0xA5", "0x43"])
def test_gz_batch_equals_text_batch_under_poison(poison):
    """MK_POISON fills every allocation before use (read once per process: a process of its own)"""
    env = dict(os.environ, MK_POISON=poison)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gz_batch_worker.py"), "7", "4", "1", "7", "9"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"gz batch parity ok" in r.stdout, r.stderr.decode()[-3000:]


def test_gz_batch_bad_files_leave_their_neighbours_alone(shufs):
    texts = gw.fasta_texts()
    gzs = [gw.gz(t) for t in texts]
    two = gw.gz(texts[1][:3000]) + gw.gz(texts[1])
    crc = bytearray(gzs[2]); crc[-8] ^= 0x04
    short = bytearray(gzs[0]); struct.pack_into("<I", short, len(short) - 4, len(texts[0]) - 1)
    bit = bytearray(gzs[4]); bit[len(bit) // 2] ^= 0x20
    eng = capi.Engine(shufs("L1K7"), 0)
    try:
        eng.batch_begin(texts, capi.MK_MODE_SET)
        want = eng.batch_end()
        batch = [gzs[0], two, gzs[1], bytes(crc), gzs[3], bytes(short), bytes(bit), gzs[4]]
        eng.batch_begin_gz(batch, capi.MK_MODE_SET)
        got = eng.batch_end()
        st = eng.batch_gz_status(len(batch))
        assert st[0] == st[2] == st[4] == st[7] == 0
        assert (st[1], st[3], st[5]) == (capi.MK_INFL_TRAILING, capi.MK_INFL_CRC, capi.MK_INFL_OUTPUT_LEN) and st[6] != 0
        for i in (1, 3, 5, 6):
            assert got[i][0] == capi.MK_ERR_FORMAT and got[i][2] == []
        gw.same([got[0], got[2], got[4], got[7]], [want[0], want[1], want[3], want[4]], "good files beside bad ones")
        with pytest.raises(capi.MkError):
            eng.batch_begin_gz([b"not gzip at all, but long enough to be asked"], capi.MK_MODE_SET)
        eng.batch_begin(texts[:1], capi.MK_MODE_SET)  # the engine is still usable
        gw.same(eng.batch_end(), want[:1], "text batch after a refused gz batch")
    finally:
        eng.close()


# ---- the command line --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shuf_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("shuf") / "L1K7.shuf")
    gc.make_shuf("L1K7", p)
    return p


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


def genome_dir(d):
    texts = gw.fasta_texts()
    os.makedirs(d)
    files = {"g0.fa.gz": gw.gz(texts[0]), "g1.fa.gz": gw.gz(texts[1], 1), "g2.fa": texts[2], "g3.fa.gz": gw.gz(texts[2], 9),
             "g4_two.fa.gz": gw.gz(texts[1][:5000]) + gw.gz(texts[1][5000:]), "g5_named.fa.gz": gw.gz(texts[4], 6, "g5_named.fa")}
    for n, b in files.items():
        open(os.path.join(d, n), "wb").write(b)
    assert capi.gzip_scan(files["g5_named.fa.gz"])["pay_off"] > 10
    return files


@pytest.mark.parametrize("flags", [[], ["-u"]])
def test_cli_directory_of_gz_genomes(flags, shuf_file, tmp_path):
    d = str(tmp_path / "genomes")
    genome_dir(d)
    base, out = str(tmp_path / "zcat"), str(tmp_path / "dev")
    r, routes = run_cli(shuf_file, base, [d], flags + ["--no-device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    assert sorted((os.path.basename(x["input"]), x["route"]) for x in routes) == [(n, "zcat") for n in ("g0.fa.gz", "g1.fa.gz", "g3.fa.gz", "g4_two.fa.gz", "g5_named.fa.gz")]
    assert not any("fallback" in x for x in routes)
    for extra in ([], ["--device-inflate", "--no-batch"]):  # off by default; and never without the batch driver
        r, routes = run_cli(shuf_file, out, [d], flags + extra)
        assert r.returncode == 0, r.stderr.decode()
        assert len(routes) == 5 and all(x["route"] == "zcat" and "fallback" not in x for x in routes)
        same_dir(base, out)
    r, routes = run_cli(shuf_file, out, [d], flags + ["--device-inflate"])
    assert r.returncode == 0, r.stderr.decode()
    by = {os.path.basename(x["input"]): x for x in routes}
    assert sorted(by) == ["g0.fa.gz", "g1.fa.gz", "g3.fa.gz", "g4_two.fa.gz", "g5_named.fa.gz"] and len(routes) == 5  # none for the plain file
    for n in ("g0.fa.gz", "g1.fa.gz", "g3.fa.gz", "g5_named.fa.gz"):
        assert by[n]["route"] == "device-inflate" and "fallback" not in by[n], by[n]  # no silent fall-back
    assert by["g4_two.fa.gz"]["route"] == "zcat" and by["g4_two.fa.gz"]["fallback"] == capi.lib.mk_inflate_status_text(capi.MK_INFL_TRAILING).decode()
    same_dir(base, out)


def test_cli_damaged_gz_genome_ends_like_the_zcat_route(shuf_file, tmp_path):
    d = str(tmp_path / "genomes")
    files = genome_dir(d)
    bad = bytearray(files["g1.fa.gz"])
    bad[len(bad) // 2] ^= 0x08
    open(os.path.join(d, "g1.fa.gz"), "wb").write(bytes(bad))
    with pytest.raises(Exception):
        gzip.decompress(bytes(bad))
    ends = []
    for name, extra in (("zcat", ["--no-device-inflate"]), ("dev", ["--device-inflate"])):
        out = str(tmp_path / name)
        r, routes = run_cli(shuf_file, out, [d], extra)
        err = r.stderr.decode()
        assert r.returncode != 0 and "g1.fa.gz" in err and "zcat -fc" in err, err
        assert not os.path.exists(os.path.join(out, "cofiles.stat"))
        ends.append((r.returncode, [ln for ln in err.splitlines() if "g1.fa.gz" in ln and "metakssd" in ln]))
    assert ends[0] == ends[1]
