"""The engine against the COMPILED REFERENCE's bytes at the sizes and table loads it is measured at.

tests/golden/fullsize_digests.json holds the digests of what `oracle/_ref/metakssd dist -A -p 1` wrote for prefixes of the bench read
stream (seed 20261002, 150 bp; made by tests/golden/make_golden_fullsize.py).  Every test here sketches the same reads on the GPU
and compares all four digests, exactly: the two files, their concatenation, and the sorted (id, count) multiset -- the last one
makes a failure say whether the CONTENT differs (scan / resolve / insert) or only the ORDER (ordinals / layout / dump).

  * ladder       L3K11 at 1 M / 4 M / 16 M reads, one push and seven (a count that does not divide N)
  * dense table  L3K10 at 30 M reads: load 0.456 of 2 097 143 slots, config 4's collision regime in 5 GB of HBM; one push, several,
                 and halves on two engines merged through partial_export / partial_import
  * row geometry the sketch does not depend on how the rows lie in memory, so every pitch, alignment and host route gives the
                 reference's digests.  mk_launch_scan_ex (mk_engine.hip) picks mk_scan_kernel<K,SUBK,VEC16,THREADS,NPIECES,ONEPASS> from
                 pitch, pointer alignment and LDS budget; GEOMETRY below lists what each case reaches.
  * command line `metakssd dist -L L3K11.shuf -A` on the 1 M reads as a FASTQ file: the two files' sha256 and cofiles.stat.

Families the shipped library can select for K = 11 (and 10), SUBK = 6, and the pitch that reaches each (column block CB, staging
pieces a lane ppr; THREADS falls from 1024 by 256 while filter + tiles exceed 160 KiB of LDS):
  <true, 1024, 5, true >  pitch 160 (CB 80, two blocks, one pass): the hot kernel
  <true,  768, 8, false>  pitch 176 (CB 96), 320 (CB 112)
  <true,  512, 8, false>  pitch 512, 4096 (CB 128; 4 and 32 column blocks)
  <false,1024,20, false>  pitch 152 (CB 80 on the 8-byte grid), pitch 160 with the pointer off by 4
  <false,1024,32, false>  pitch 168 (CB 88)
  <false, 768,32, false>  pitch 200 (CB 104)
  <false, 512,32, false>  pitch 248 (CB 128)
  generic <0,0,false,1024|768,32,false>  pitch 164 (CB 84), 308 (CB 104): not a multiple of 8
  mk_scan_packed_kernel<K,6>  64-byte packed rows
Not reachable from the shipped library with 150-base rows: <true,*,5,false> (a 16-byte-path block of at most 80 bytes that is not
half of the row needs a pitch of at most 144); <true,1024,8,false> (a block of 96 bytes or more never fits 16 waves);
<true,768|512,5,true> and <false,768|512,20,false> (blocks of 80 bytes always fit 16 waves; the MK_SCAN_THREADS knob exists in tuning
builds only); the generic kernel on the 16-byte path (a 16-byte grid is an 8-byte grid, so the tuned kernel is taken).

No test reads the reference or needs oracle/_ref; device memory is freed in `finally`."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import fullsize_ref as fr
from dev_rows import DevRows, dev_alloc, hip_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")


@pytest.fixture(scope="module")
def capi():
    from metakssd_amd import capi as c
    if c.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run on the MI355X box")
    return c


@pytest.fixture(scope="module")
def hip():
    return hip_lib()


@pytest.fixture(scope="module")
def ref():
    return fr.entries()


_engines = {}


@pytest.fixture(scope="module")
def engine_for(capi, shufs):
    def get(name):
        if name not in _engines:
            _engines[name] = capi.Engine(shufs(name), 0)
        return _engines[name]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


def sketch_dev(capi, eng, rows, pushes=1, first=0, n=None):
    """begin, push rows [first, first + n) in `pushes` pieces, finish -> (ids, counts)"""
    n = rows.n - first if n is None else n
    eng.begin(capi.MK_MODE_KOC)
    per = (n + pushes - 1) // pushes
    done = 0
    while done < n:
        m = min(per, n - done)
        eng.push_reads_device(rows.ptr + (first + done) * rows.pitch, rows.pitch, m, first + done)
        done += m
    got = eng.finish()
    assert len(got) == 1
    return got[0]


# ---- b. the ladder ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pushes", [1, 7])
@pytest.mark.parametrize("name", ["L3K11_1M", "L3K11_4M", "L3K11_16M"])
def test_ladder_equals_reference(capi, hip, ref, engine_for, name, pushes):
    x = ref[name]
    assert x["reads"] % pushes != 0 or pushes == 1
    rows = DevRows(capi, hip, x, 160)
    try:
        ids, cnt = sketch_dev(capi, engine_for(x["shuf"]), rows, pushes)
    finally:
        rows.free()
    fr.assert_equals_reference(x, ids, cnt, "device rows, pitch 160, %d push(es)" % pushes)


# ---- c. the dense table -----------------------------------------------------------------------------------------------------------
def test_dense_table_equals_reference(capi, hip, ref, shufs, engine_for):
    """L3K10, 30 M reads: 955 995 keys in 2 097 143 slots (load 0.456): nearly every insert probes past occupied slots, so the slot
    order -- the file's byte order -- depends on the first-occurrence ordinals being the reference's.  One engine with one push and
    with eleven; then the halves on two engines, merged through the partial lists (what two GPUs do)."""
    x = ref["L3K10_dense"]
    assert 0.40 <= x["keys"] / x["slots"] <= 0.50
    e0 = engine_for(x["shuf"])
    e1 = capi.Engine(shufs(x["shuf"]), 0)
    rows = None
    bufs = []
    try:
        rows = DevRows(capi, hip, x, 160)
        for pushes in (1, 11):
            ids, cnt = sketch_dev(capi, e0, rows, pushes)
            fr.assert_equals_reference(x, ids, cnt, "dense table, one engine, %d push(es)" % pushes)
        assert int(cnt.max()) == x["max_count"]
        n, half = rows.n, rows.n // 2 + 1
        for e in (e0, e1):
            e.begin(capi.MK_MODE_KOC)
        e0.push_reads_device(rows.ptr, 160, half, 0)
        e1.push_reads_device(rows.ptr + half * 160, 160, n - half, half)
        d1 = e1.partial_count()
        for nbytes in (8 * d1, 4 * d1, 8 * d1):
            bufs.append(dev_alloc(hip, nbytes))
        assert e1.partial_export(bufs[0].value, bufs[1].value, bufs[2].value, d1) == d1
        e0.partial_import(bufs[0].value, bufs[1].value, bufs[2].value, d1)
        ids, cnt = e0.finish()[0]
        fr.assert_equals_reference(x, ids, cnt, "dense table, halves on two engines merged (%d keys imported)" % d1)
    finally:
        for p in bufs:
            hip.hipFree(p)
        if rows is not None:
            rows.free()
        e1.close()


# ---- d. row geometry --------------------------------------------------------------------------------------------------------------
# (entry, pitch, pointer offset)            what mk_launch_scan_ex selects: <VEC16, THREADS, NPIECES, ONEPASS>, tuned / generic
GEOMETRY = [
    ("L3K11_4M", 160, 0),     # <true, 1024, 5, true>   tuned  CB 80 x 2, one pass: the hot kernel
    ("L3K11_4M", 176, 0),     # <true,  768, 8, false>  tuned  CB 96 x 2 (6 pieces a lane)
    ("L3K11_4M", 320, 0),     # <true,  768, 8, false>  tuned  CB 112 x 3 (7 pieces a lane)
    ("L3K11_4M", 512, 0),     # <true,  512, 8, false>  tuned  CB 128 x 4
    ("L3K11_1M", 4096, 0),    # <true,  512, 8, false>  tuned  CB 128 x 32: many column blocks
    ("L3K11_4M", 152, 0),     # <false,1024,20, false>  tuned  CB 80 + 72 (8-byte grid)
    ("L3K11_4M", 168, 0),     # <false,1024,32, false>  tuned  CB 88 x 2 (22 pieces a lane)
    ("L3K11_4M", 200, 0),     # <false, 768,32, false>  tuned  CB 104 x 2
    ("L3K11_4M", 248, 0),     # <false, 512,32, false>  tuned  CB 128 x 2
    ("L3K11_4M", 160, 4),     # <false,1024,20, false>  tuned  VEC16 lost through alignment, not pitch
    ("L3K11_4M", 164, 0),     # <0,0,false,1024,32,false> generic  CB 84 x 2: a multiple of 4 only
    ("L3K11_4M", 308, 0),     # <0,0,false, 768,32,false> generic  CB 104 x 3
    # the <10,6,...> family on the loaded table
    ("L3K10_dense", 152, 0),  # <false,1024,20, false>  tuned
    ("L3K10_dense", 176, 0),  # <true,  768, 8, false>  tuned
    ("L3K10_dense", 308, 0),  # generic
    ("L3K10_dense", 160, 4),  # <false,1024,20, false>  tuned
]


@pytest.mark.parametrize("name,pitch,offset", GEOMETRY, ids=["%s-p%d+%d" % g for g in GEOMETRY])
def test_row_geometry_equals_reference(capi, hip, ref, engine_for, name, pitch, offset):
    x = ref[name]
    rows = DevRows(capi, hip, x, pitch, offset)
    try:
        assert (rows.ptr & 15) == (offset & 15)
        ids, cnt = sketch_dev(capi, engine_for(x["shuf"]), rows, 3)
    finally:
        rows.free()
    fr.assert_equals_reference(x, ids, cnt, "device rows, pitch %d, pointer + %d, 3 pushes" % (pitch, offset))


@pytest.fixture(scope="module")
def host_rows_4m(capi, ref):
    x = ref["L3K11_4M"]
    return capi.synth_rows_host(x["seed"], 0, x["reads"], x["read_len"], 160)


def test_host_rows_staged_equal_reference(capi, ref, engine_for, host_rows_4m):
    """push_reads of pageable rows: copied through the staging regions (256 MiB each), one scan a region"""
    x = ref["L3K11_4M"]
    eng = engine_for("L3K11")
    eng.begin(capi.MK_MODE_KOC)
    cut = 1_234_567
    eng.push_reads(host_rows_4m[:cut * 160], 160, 0)
    eng.push_reads(host_rows_4m[cut * 160:], 160, cut)
    ids, cnt = eng.finish()[0]
    fr.assert_equals_reference(x, ids, cnt, "host rows, push_reads (staged), pitch 160")


def test_host_rows_async_tickets_equal_reference(capi, ref, engine_for, host_rows_4m):
    """push_reads_async: 42 pushes in flight behind one another (more than the ticket ring), waited for in reverse order"""
    x = ref["L3K11_4M"]
    eng = engine_for("L3K11")
    n, per = x["reads"], 97_001
    eng.begin(capi.MK_MODE_KOC)
    tickets = [eng.push_reads_async(host_rows_4m[lo * 160:min(n, lo + per) * 160], 160, lo) for lo in range(0, n, per)]
    assert len(tickets) > 32
    for t in reversed(tickets):
        eng.push_wait(t)
    ids, cnt = eng.finish()[0]
    fr.assert_equals_reference(x, ids, cnt, "host rows, push_reads_async with tickets, pitch 160")


def test_pinned_rows_scanned_in_place_equal_reference(capi, ref, shufs, host_rows_4m):
    """MK_OPT_DIRECT_HOST: the scan kernel reads pinned host rows over the bus, no staging copy"""
    x = ref["L3K11_4M"]
    eng = capi.Engine(shufs("L3K11"), 0)
    p = C.c_void_p()
    try:
        eng.set_option(capi.MK_OPT_DIRECT_HOST, 1)
        assert capi.lib.mk_host_alloc(C.byref(p), host_rows_4m.size) == 0
        C.memmove(p, host_rows_4m.ctypes.data, host_rows_4m.size)
        eng.begin(capi.MK_MODE_KOC)
        n, cut = x["reads"], 1_500_001
        t1, t2 = C.c_uint64(0), C.c_uint64(0)
        capi._check(capi.lib.mk_sketch_push_reads_async(eng.h, p, 160, cut, 0, C.byref(t1)), eng.h)
        capi._check(capi.lib.mk_sketch_push_reads_async(eng.h, C.c_void_p(p.value + cut * 160), 160, n - cut, cut, C.byref(t2)), eng.h)
        eng.push_wait(t1.value)
        eng.push_wait(t2.value)
        ids, cnt = eng.finish()[0]
    finally:
        eng.close()
        if p:
            capi.lib.mk_host_free(p)
    fr.assert_equals_reference(x, ids, cnt, "pinned host rows scanned in place (MK_OPT_DIRECT_HOST), pitch 160")


def test_packed_rows_equal_reference(capi, ref, engine_for, host_rows_4m):
    """64-byte packed rows (mk_pack_rows_host -> MK_ROWS_PACKED): mk_scan_packed_kernel<11,6>"""
    x = ref["L3K11_4M"]
    packed = capi.pack_rows_host(host_rows_4m, 160)
    assert packed.size == x["reads"] * capi.MK_PACKED_PITCH
    eng = engine_for("L3K11")
    eng.begin(capi.MK_MODE_KOC)
    cut = 2_000_003
    P = capi.MK_PACKED_PITCH | capi.MK_ROWS_PACKED
    eng.push_reads(packed[:cut * 64], P, 0)
    eng.push_reads(packed[cut * 64:], P, cut)
    ids, cnt = eng.finish()[0]
    fr.assert_equals_reference(x, ids, cnt, "host rows packed to 64 bytes (MK_ROWS_PACKED)")


# ---- e. the command line ----------------------------------------------------------------------------------------------------------
def test_command_line_files_equal_reference(capi, ref, shufs, tmp_path):
    """`metakssd dist -L L3K11.shuf -A` on the 1 M reads as a FASTQ file (318 MB): the FILES are the reference's"""
    x = ref["L3K11_1M"]
    sp, fq, out = str(tmp_path / "L3K11.shuf"), str(tmp_path / "reads.fq"), str(tmp_path / "out")
    shufs("L3K11").write(sp)
    assert hashlib.sha256(open(sp, "rb").read()).hexdigest() == x["shuf_sha256"]
    assert capi.lib.mk_synth_fastq_write_mt(fq.encode(), x["seed"], 0, x["reads"], x["read_len"], 8) == 0
    try:
        r = subprocess.run([PRODUCT_CLI, "dist", "-L", sp, "-A", "-o", out, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
    finally:
        os.unlink(fq)
    ids = np.fromfile(os.path.join(out, "combco.0"), dtype=np.uint32)
    cnt = np.fromfile(os.path.join(out, "combco.0.a"), dtype=np.uint16)
    assert not os.path.exists(os.path.join(out, "combco.1"))
    fr.assert_equals_reference(x, ids, cnt, "command line, FASTQ file")
    assert hashlib.sha256(open(os.path.join(out, "combco.0"), "rb").read()).hexdigest() == x["combco_sha256"]
    assert hashlib.sha256(open(os.path.join(out, "combco.0.a"), "rb").read()).hexdigest() == x["combco_a_sha256"]
    b = open(os.path.join(out, "cofiles.stat"), "rb").read()
    koc = struct.unpack_from("<B", b, 4)[0]
    comp_num, infile_num, all_ctx = struct.unpack_from("<iiQ", b, 16)
    assert (koc, comp_num, infile_num, all_ctx) == (1, 1, 1, x["keys"])
    assert struct.unpack_from("<I", b, 32)[0] == x["keys"]
