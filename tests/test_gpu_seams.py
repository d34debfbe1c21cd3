"""The tuned scan kernels at every row pitch the front ends and other ABI callers can choose, on ragged rows with PLANTED accepted
k-mers at every column a column-block seam can touch (tests/seam_cases.py): the engine against the CPU oracle, bit for bit -- ids,
order and counts -- as one push and as three uneven pushes that do not fall on tile bounds.

MK_ROW_PITCH turns 100-base reads into pitch 112, 125-base reads into 144, 250-base reads into 272, 300-base reads into 304, and so on
up to 4096; tests/test_gpu_refdigest.py reaches the same launch families with the benchmark's rows only (150 clean bases, every row
ending at the same column), where pair body B runs on the last pair of a row and nothing is carried across a seam but a full window.

PITCHES below says what mk_launch_scan_ex (mk_engine.hip) selects for each pitch: mk_scan_kernel<K, SUBK, VEC16, THREADS, NPIECES,
ONEPASS>, the column block CB, the number of blocks and the width of the last one; tests/test_seam_cases.py checks the table against
seam_cases.launch_plan without a GPU.  K, SUBK are the geometry's (<11,6>, <10,6>, <9,6>, <11,5>) where the row says tuned and <0,0>
where it says generic.

Two cases go through the front ends that pick the pitch themselves (the engine's FASTQ stream, `metakssd dist -A`), and five inputs
are pinned to what the compiled reference wrote for them (tests/golden/seams, made by tests/golden/make_golden_seams.py).

No test reads the reference or needs oracle/_ref; device memory is freed in `finally`."""
import filecmp
import os
import subprocess

import pytest

import seam_cases as sc
from dev_rows import DevRows, hip_lib
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_CLI = os.path.join(ROOT, "oracle", "kssd_oracle_cli")
PRODUCT_CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")

# (pitch, pointer offset, VEC16, THREADS at subk 6, at subk 5, NPIECES, ONEPASS, CB, blocks, last block, tuned)
PITCHES = [
    # the 16-byte path: what MK_ROW_PITCH gives the front ends
    (48, 0, True, 1024, 1024, 5, False, 48, 1, 48, True),       # one block; <true,1024,5,false> is reached by no 150-base row
    (80, 0, True, 1024, 1024, 5, False, 80, 1, 80, True),       # one block of the widest 5-piece width
    (112, 0, True, 768, 768, 8, False, 112, 1, 112, True),      # 100-base reads: one block of 112 (7 pieces a lane)
    (144, 0, True, 1024, 1024, 5, False, 80, 2, 64, True),      # 125-base reads: 80 + 64, a short last block, no one-pass staging
    (160, 0, True, 1024, 1024, 5, True, 80, 2, 80, True),       # 150-base reads: 80 x 2, one pass -- the hot kernel
    (176, 0, True, 768, 768, 8, False, 96, 2, 80, True),        # 96 + 80
    (272, 0, True, 768, 768, 8, False, 96, 3, 80, True),        # 250-base reads: 96, 96, 80
    (304, 0, True, 768, 768, 8, False, 112, 3, 80, True),       # 300-base reads: 112, 112, 80
    (528, 0, True, 768, 768, 8, False, 112, 5, 80, True),       # the base streams' pitch: 4 x 112 + 80
    (1040, 0, True, 512, 512, 8, False, 128, 9, 16, True),      # 8 x 128 + 16: a last block of one piece
    (4096, 0, True, 512, 512, 8, False, 128, 32, 128, True),    # 32 x 128: ordinals and `meta` columns above 560
    # the 8-byte path: what other ABI callers may choose
    (152, 0, False, 1024, 1024, 20, False, 80, 2, 72, True),    # 80 + 72
    (168, 0, False, 1024, 1024, 32, False, 88, 2, 80, True),    # 88 + 80 (22 pieces a lane)
    (200, 0, False, 768, 768, 32, False, 104, 2, 96, True),     # 104 + 96
    (248, 0, False, 512, 512, 32, False, 128, 2, 120, True),    # 128 + 120
    (160, 4, False, 1024, 1024, 20, False, 80, 2, 80, True),    # VEC16 lost through the pointer, not the pitch: device rows
    # a multiple of 4 only: a tuned geometry on the generic kernel <0,0,false,T,32,false> (its filter is 2^10 words at subk 5)
    (164, 0, False, 1024, 1024, 32, False, 84, 2, 80, False),   # 84 + 80
    (308, 0, False, 768, 1024, 32, False, 104, 3, 100, False),  # 104, 104, 100
]
CASES = [(g, row[0], row[1]) for g in sc.GEOMS for row in PITCHES]


@pytest.fixture(scope="module")
def capi():
    from metakssd_amd import capi as c
    if c.device_count() < 1:
        pytest.fail("no HIP device: the -m gpu tests must run on the MI355X box")
    return c


@pytest.fixture(scope="module")
def hip():
    return hip_lib()


_engines = {}


@pytest.fixture(scope="module")
def engine_for(capi, shufs):
    """one engine a geometry (L2K11: the 21 GB engine tests/test_gpu_parity.py allocates too)"""
    def get(name):
        if name not in _engines:
            _engines[name] = capi.Engine(shufs(name), 0)
        return _engines[name]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


@pytest.fixture(scope="module")
def oracles(shufs, oracle_for):
    made = {}

    def get(name):
        if name not in made:
            made[name] = oracle_for(shufs(name))
        return made[name]
    return get


def uneven_cuts(n):
    """three pushes of different sizes, neither cut on a multiple of 64"""
    c1, c2 = n // 5, n * 3 // 5 + 7
    c1 += c1 % 64 == 0
    c2 += c2 % 64 == 0
    assert 0 < c1 < c2 < n and c1 % 64 and c2 % 64
    return [0, c1, c2, n]


def sketch_rows(capi, eng, rows, pitch, cuts, dev=None):
    """begin, push rows [cuts[i], cuts[i + 1]) from the host array (or from device rows), finish"""
    eng.begin(capi.MK_MODE_KOC)
    for lo, hi in zip(cuts, cuts[1:]):
        if dev is None:
            eng.push_reads(rows[lo * pitch:hi * pitch], pitch, lo)
        else:
            eng.push_reads_device(dev.ptr + lo * pitch, pitch, hi - lo, lo)
    return eng.finish()


@pytest.mark.parametrize("geom,pitch,offset", CASES, ids=["%s-p%d+%d" % c for c in CASES])
def test_planted_seams_equal_oracle(capi, hip, engine_for, oracles, geom, pitch, offset):
    case = sc.get_case(geom, pitch)
    rc, want = oracles(geom).koc_from_rows(case.rows, pitch)
    assert rc == 0
    sc.check_conditions(case, want)  # the comparison below is about planted k-mers at every anchor, not about an empty sketch
    eng = engine_for(geom)
    dev = DevRows.from_host(hip, case.rows, pitch, offset) if offset else None
    try:
        assert dev is None or (dev.ptr & 15) == offset
        for cuts in ([0, case.nrows], uneven_cuts(case.nrows)):
            got = sketch_rows(capi, eng, case.rows, pitch, cuts, dev)
            label = "%s pitch %d pointer + %d, %d push(es)" % (geom, pitch, offset, len(cuts) - 1)
            have = case.counts_of_planted(got)
            miss = [(j, h, case.expected[int(k)]) for j, h, k in zip(case.anchors, have, case.keys) if h != case.expected[int(k)]]
            assert not miss, "%s: planted k-mers with another count (end column, got, want): %s" % (label, miss[:12])
            assert_same(got, want, label)
    finally:
        if dev is not None:
            dev.free()


@pytest.mark.parametrize("name", sorted(sc.GOLDEN))
def test_engine_reproduces_reference_fixture(capi, engine_for, name):
    """what the compiled reference wrote for the FASTQ form of these rows (dist -A -p 1)"""
    geom, pitch, lmax = sc.GOLDEN[name]
    case = sc.get_case(geom, pitch, lmax)
    got = sketch_rows(capi, engine_for(geom), case.rows, pitch, uneven_cuts(case.nrows))
    assert_same(got, sc.fixture(name), name)
    assert case.counts_of_planted(got) == sc.manifest()["cases"][name]["planted_counts"]


def oracle_cli_sketch(shufs, geom, fq, tmp_path):
    """the oracle command line's directory for the FASTQ file: (path, [(ids, counts)] per component)"""
    sp, out = str(tmp_path / (geom + ".shuf")), str(tmp_path / "out_oracle")
    shufs(geom).write(sp)
    r = subprocess.run([ORACLE_CLI, "-L", sp, "-A", "-o", out, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
    return sp, out, sc.load_dir(out, sc.params(geom).component_num)


def front_end_input(capi, geom):
    """the pitch-272 input with rows of at most 255 bases as a FASTQ text; the stream frames it at MK_ROW_PITCH(256) = 272"""
    case = sc.get_case(geom, 272, 255)
    data = case.fastq()
    pushes, st, rc = capi.fastq_stream(data, nthreads=4)
    assert rc == 0 and sum(p[2] for p in pushes) == case.nrows
    assert [p[1] for p in pushes] == [272] * len(pushes), "the stream's stride"
    return case, data


def test_fastq_stream_picks_pitch_272(capi, engine_for, oracles, shufs, tmp_path):
    geom = "L3K11"
    case, data = front_end_input(capi, geom)
    rc, want = oracles(geom).koc_from_fastq(data)
    assert rc == 0
    sc.check_conditions(case, want)
    eng = engine_for(geom)
    eng.begin(capi.MK_MODE_KOC)
    st = eng.push_fastq(data, nthreads=4)
    assert st.rows == case.nrows
    got = eng.finish()
    assert_same(got, want, "FASTQ stream against koc_from_fastq")
    fq = str(tmp_path / "reads.fq")
    open(fq, "wb").write(data)
    _, _, cli = oracle_cli_sketch(shufs, geom, fq, tmp_path)
    assert_same(got, cli, "FASTQ stream against the oracle command line")


def test_command_line_picks_pitch_272(capi, oracles, shufs, tmp_path):
    geom = "L3K9"
    case, data = front_end_input(capi, geom)
    fq = str(tmp_path / "reads.fq")
    open(fq, "wb").write(data)
    sp, out_o, cli = oracle_cli_sketch(shufs, geom, fq, tmp_path)
    out_p = str(tmp_path / "out_product")
    r = subprocess.run([PRODUCT_CLI, "dist", "-L", sp, "-A", "-o", out_p, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-400:]
    names = sorted(f for f in os.listdir(out_o) if f.startswith("combco"))
    assert names and names == sorted(f for f in os.listdir(out_p) if f.startswith("combco"))
    for f in names:
        assert filecmp.cmp(os.path.join(out_o, f), os.path.join(out_p, f), shallow=False), f
    got = sc.load_dir(out_p, sc.params(geom).component_num)
    rc, want = oracles(geom).koc_from_fastq(data)
    assert rc == 0
    sc.check_conditions(case, want)
    assert_same(got, want, "metakssd dist -A against koc_from_fastq")
