"""`dist --byread`, `reverse -b` and `reverse` on the GPU: the command line and the C ABI reproduce the reference-made fixtures of
tests/golden/byread byte for byte, equal tests/byread_model.py (pinned to the reference by tests/test_byread_model.py) on seeded
random FASTA, do not depend on how the text is cut into pushes, and satisfy two properties that need no model."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import byread_model as bm
from golden_cases import make_shuf
from test_byread_model import GOLD, MANIFEST, build_sketch_dir, fixture_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
SHUFS = ["L3K10", "L1K7", "L0K6", "L2K11"]


@pytest.fixture(scope="module")
def shuf_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("shufs")
    made = {}

    def get(name):
        if name not in made:
            p = str(d / (name + ".shuf"))
            make_shuf(name, p)
            made[name] = p
        return made[name]
    return get


@pytest.fixture(scope="module")
def handles(shufs):
    from metakssd_amd import capi
    made = {}

    def get(name):
        if name not in made:
            made[name] = capi.ByRead(shufs(name), 0)
        return made[name]
    yield get
    for h in made.values():
        h.close()


def run_cli(args, cwd, env=None, check=True):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([BIN] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    if check:
        assert r.returncode == 0, (args, r.stderr.decode(errors="replace")[-500:])
    return r


def check_fixture_pipeline(case, shuf_files, tmp_path, env=None):
    e = MANIFEST["cases"][case]
    shuf = shuf_files(e["shuf"])
    inp = str(tmp_path / e["name"])
    open(inp, "wb").write(fixture_text(e))
    out = str(tmp_path / "out")
    r = run_cli(["dist", "-L", shuf, "--byread", "-o", out, inp], tmp_path, env)
    lines = r.stdout.decode().splitlines()
    assert "decomposing %s by reads" % inp in lines and "decomposing %s by reads is complete!" % inp in lines
    C = e["header"]["comp_num"]
    for c in range(C):
        for f in ("combco.%d" % c, "combco.index.%d" % c):
            assert open(os.path.join(out, f), "rb").read() == open(os.path.join(GOLD, case, f), "rb").read(), (case, f)
    assert sorted(os.listdir(out)) == sorted(["cofiles.stat"] + [f for f in e["files"] if f.startswith("combco")])
    raw = open(os.path.join(out, "cofiles.stat"), "rb").read()
    assert len(raw) == 32 + 4 + 256
    st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
    assert {k: st[k] for k in e["header"]} == e["header"]
    assert st["ctx_ct"] == [0]  # the reference leaves this word uninitialised; the product writes 0
    assert st["names"] == [inp] and raw[36 + len(inp):] == b"\0" * (256 - len(inp))
    r = run_cli(["reverse", "-L", shuf, "-b", out], tmp_path, env)
    assert r.stdout == gzip.open(os.path.join(GOLD, case, "reverse_b.txt.gz")).read(), case


@pytest.mark.parametrize("case", sorted(MANIFEST["cases"]))
def test_cli_reproduces_byread_fixture(case, shuf_files, tmp_path):
    check_fixture_pipeline(case, shuf_files, tmp_path)


def test_cli_fixture_pipeline_under_poison(shuf_files, tmp_path):
    """MK_POISON fills every allocation of the library before use: a kernel that read what nobody wrote would not match"""
    check_fixture_pipeline("synthetic_L0K6", shuf_files, tmp_path, env={"MK_POISON": "0xA5"})
    (tmp_path / "b").mkdir()
    check_fixture_pipeline("fa_sA_L2K11", shuf_files, tmp_path / "b", env={"MK_POISON": "0xA5"})


@pytest.mark.parametrize("case", sorted(MANIFEST["cases"]))
def test_abi_reproduces_byread_fixture(case, handles):
    e = MANIFEST["cases"][case]
    h = handles(e["shuf"])
    ids, index, records, _ = h.run(fixture_text(e))
    assert records == e["records"] and len(ids) == e["header"]["comp_num"]
    for c in range(len(ids)):
        assert ids[c].tobytes() == open(os.path.join(GOLD, case, "combco.%d" % c), "rb").read(), (case, c)
        assert index[c].tobytes() == open(os.path.join(GOLD, case, "combco.index.%d" % c), "rb").read(), (case, c)
    # reverse -b through the ABI: the cursor rule on the host, the lines from the device
    want = gzip.open(os.path.join(GOLD, case, "reverse_b.txt.gz")).read()
    lines = [h.reverse_ids(ids[c], c) for c in range(len(ids))]
    W = h.params.TL + 1
    out, cur = [], [0] * len(ids)
    for n in range(records):
        out.append(b">read %d\n" % (n + 1))
        for c in range(len(ids)):
            k = int(index[c][n + 1]) - int(index[c][n])
            out.append(lines[c][cur[c] * W:(cur[c] + k) * W])
            cur[c] += k
    assert b"".join(out) == want


@pytest.mark.parametrize("case", sorted(MANIFEST["reverse_cases"]))
def test_cli_reproduces_reverse_fixture(case, shuf_files, tmp_path):
    e = build_sketch_dir(case, str(tmp_path / "sk"))
    shuf = shuf_files(e["shuf"])
    (tmp_path / "kmers").mkdir()
    # options in any order, -p accepted
    run_cli(["reverse", str(tmp_path / "sk"), "-p", "3", "-o", str(tmp_path / "kmers"), "-L", shuf], tmp_path)
    assert sorted(os.listdir(str(tmp_path / "kmers"))) == sorted(e["outputs"])  # nothing for the sketch without ids
    for name in e["outputs"]:
        assert open(str(tmp_path / "kmers" / name), "rb").read() == gzip.open(os.path.join(GOLD, case, "kmers", name + ".gz")).read(), (case, name)


def same(got, want_ids, want_index, tag):
    ids, index = got[0], got[1]
    assert len(ids) == len(want_ids)
    for c in range(len(ids)):
        assert np.array_equal(ids[c], want_ids[c]), (tag, "ids", c, len(ids[c]), len(want_ids[c]))
        assert np.array_equal(index[c], want_index[c]), (tag, "index", c)


@pytest.mark.parametrize("shuf_name", SHUFS)
def test_abi_equals_model_on_random_fasta(shuf_name, shufs, handles):
    P = bm.Params.from_shuf(shufs(shuf_name))
    h = handles(shuf_name)
    rs = np.random.RandomState(SHUFS.index(shuf_name) + 100)
    texts = {
        # thousands of short records, some of them empty or shorter than 2k, CRLF, lower case, N
        "short": bm.random_fasta(rs, nrec=6000, min_len=0, max_len=90, width=60, lower=0.2, n_rate=0.001, crlf=True, lead=37),
        # records of more than 4 095 bases (the FASTQ ordinal's in-row position has 12 bits) and empty ones
        "mid": bm.random_fasta(rs, nrec=40, min_len=0, max_len=30000, width=70, n_rate=0.0002),
        # one record of more than 2^20 bases between two small ones, several pushes of MK_BYREAD_MAX_PUSH... and no final newline
        "long": (bm.random_fasta(rs, nrec=1, min_len=500, max_len=500) + bm.random_fasta(rs, nrec=1, min_len=(1 << 20) + 12345, max_len=(1 << 20) + 12345, width=80)
                 + bm.random_fasta(rs, nrec=2, min_len=0, max_len=300)).rstrip(b"\n"),
    }
    for tag, text in texts.items():
        want_ids, want_index = bm.byread(text, P)
        same(h.run(text), want_ids, want_index, (shuf_name, tag))
        same(h.run(text, pieces=1 << 18), want_ids, want_index, (shuf_name, tag, "256 KiB pushes"))


def test_large_text_spans_several_full_pushes(shufs, handles):
    """more than two pushes of MK_BYREAD_MAX_PUSH bytes: a record of 17 Mi bases (positions and counts beyond one push)"""
    from metakssd_amd import capi
    P = bm.Params.from_shuf(shufs("L3K10"))
    rs = np.random.RandomState(5)
    text = b">big\n" + np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, size=17 << 20)].tobytes() + b"\n>tail\nACGTTGCAACGTTGCAACGTAGCATCGA\n"
    assert len(text) > 2 * capi.MK_BYREAD_MAX_PUSH
    want_ids, want_index = bm.byread(text, P)
    same(handles("L3K10").run(text), want_ids, want_index, "17 Mi bases")


@pytest.mark.parametrize("shuf_name", ["L1K7", "L2K11"])
def test_chunk_invariance(shuf_name, shufs, handles):
    """the same text whole, byte by byte over its first 300 bytes, and in pieces of 63, 1 023, 1 024 and 1 025 bytes"""
    h = handles(shuf_name)
    rs = np.random.RandomState(9)
    text = bm.synthetic_text() + b"\n" + bm.random_fasta(rs, nrec=30, min_len=0, max_len=2500, width=61, lower=0.1, n_rate=0.001, crlf=True)
    whole = h.run(text)
    P = bm.Params.from_shuf(shufs(shuf_name))
    same(whole, *bm.byread(text, P), tag="whole")
    for tag, cuts in [("bytewise", list(range(1, 301)))] + [(str(s), list(range(s, len(text), s))) for s in (63, 1023, 1024, 1025)]:
        got = h.run(text, pieces=cuts)
        same(got, whole[0], whole[1], (shuf_name, tag))
        assert got[2] == whole[2]


def revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@pytest.mark.parametrize("shuf_name", ["L1K7", "L3K10"])
def test_recovered_kmers_occur_in_their_record(shuf_name, handles):
    """needs no model: every k-mer `reverse` gives back for a record's ids occurs in that record, on one strand"""
    h = handles(shuf_name)
    rs = np.random.RandomState(21)
    recs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, size=int(rs.randint(200, 60000)))].tobytes() for _ in range(12)]
    text = b"".join(b">r%d\n" % i + b"\n".join(r[j:j + 60] for j in range(0, len(r), 60)) + b"\n" for i, r in enumerate(recs))
    ids, index, records, _ = h.run(text)
    assert records == len(recs)
    W = h.params.TL + 1
    total = 0
    for c in range(len(ids)):
        assert index[c][0] == 0 and index[c][-1] == len(ids[c])
        lines = h.reverse_ids(ids[c], c)
        for n, r in enumerate(recs):
            both = r + b"|" + revcomp(r)
            for i in range(int(index[c][n]), int(index[c][n + 1])):
                kmer = lines[i * W:(i + 1) * W - 1]
                assert lines[(i + 1) * W - 1:(i + 1) * W] == b"\n" and kmer in both, (shuf_name, c, n, kmer)
                total += 1
    assert total > 20


@pytest.mark.parametrize("shuf_name", ["L1K7", "L2K11"])
def test_distinct_byread_ids_are_the_plain_sketch(shuf_name, shuf_files, tmp_path):
    """needs no model: the distinct ids of a by-read run are the ids of the plain `dist` sketch of the same file.  The one
    exception is key 0: only the by-read path stores it (fasta2co() treats a zero slot as empty), so id 0 of component 0 is
    left out of the comparison on both sides."""
    inp = str(tmp_path / "g.fa")
    open(inp, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "inputs", "fa_genome.fa.gz")).read())
    shuf = shuf_files(shuf_name)
    run_cli(["dist", "-L", shuf, "--byread", "-o", str(tmp_path / "br"), inp], tmp_path)
    run_cli(["dist", "-L", shuf, "-o", str(tmp_path / "sk"), inp], tmp_path)
    C = bm.parse_stat(str(tmp_path / "sk" / "cofiles.stat"))["comp_num"]
    n = 0
    for c in range(C):
        a = np.unique(np.fromfile(str(tmp_path / "br" / ("combco.%d" % c)), dtype="<u4"))
        b = np.sort(np.fromfile(str(tmp_path / "sk" / ("combco.%d" % c)), dtype="<u4"))
        if c == 0:
            a, b = a[a != 0], b[b != 0]
        assert np.array_equal(a, b), (shuf_name, c)
        n += a.size
    assert n > 100


@pytest.mark.parametrize("shuf_name", SHUFS)
def test_reverse_ids_equals_model_on_a_million_ids(shuf_name, shufs, handles):
    P = bm.Params.from_shuf(shufs(shuf_name))
    h = handles(shuf_name)
    rs = np.random.RandomState(33)
    id_bits = 4 * (P.k - P.drlevel) - P.comp_code_bits
    for c in sorted({0, P.component_num - 1, P.component_num // 2}):
        ids = rs.randint(0, 1 << id_bits, size=1000003, dtype=np.int64).astype(np.uint32)
        assert h.reverse_ids(ids, c) == bm.kmer_lines(ids, c, P), (shuf_name, c)
    assert h.reverse_ids(np.zeros(0, np.uint32), 0) == b""


def test_rejected_command_lines(shuf_files, tmp_path):
    shuf = shuf_files("L1K7")
    fa = str(tmp_path / "a.fa")
    open(fa, "wb").write(b">a\nACGTACGTACGTACGTACGT\n")
    gz = str(tmp_path / "b.fa.gz")
    open(gz, "wb").write(gzip.compress(b">a\nACGT\n"))
    out = str(tmp_path / "o")
    bad = [["dist", "-L", shuf, "--byread", "-o", out, fa, fa],
           ["dist", "-L", shuf, "--byread", "-o", out],
           ["dist", "-L", shuf, "--byread", "-A", "-o", out, fa],
           ["dist", "-L", shuf, "--byread", "-u", "-o", out, fa],
           ["dist", "-L", shuf, "--byread", "-n", "2", "-o", out, fa],
           ["dist", "-L", shuf, "--byread", "-Q", "20", "-o", out, fa],
           ["dist", "-L", shuf, "--byread", "--devices", "0,0", "-o", out, fa],
           ["dist", "-L", shuf, "--byread", "-o", out, gz],
           ["dist", "--byread", "-o", out, fa]]
    run_cli(["dist", "-L", shuf, "--byread", "-o", out, fa], tmp_path)
    # reverse: a missing output directory, no sketch directory, two directories, a table that cannot be inverted
    small = str(tmp_path / "small.shuf")
    b = bytearray(open(shuf, "rb").read())
    tab = np.frombuffer(bytes(b[16:]), dtype="<i4").copy()
    i, j = int(np.nonzero(tab == 5)[0][0]), int(np.nonzero(tab == 5000)[0][0])
    tab[i] = 5000  # 4 095 entries below 4 096
    open(small, "wb").write(bytes(b[:16]) + tab.tobytes())
    assert j != i
    bad += [["reverse", "-L", shuf, "-o", str(tmp_path / "missing"), out],
            ["reverse", "-L", shuf, "-b", str(tmp_path)],
            ["reverse", "-L", shuf, "-b", out, out],
            ["reverse", "-L", small, "-b", out],
            ["reverse", "-b", out]]
    for args in bad:
        r = run_cli(args, tmp_path, check=False)
        assert r.returncode != 0 and r.stderr.strip(), args
    # a file that ends inside a header line: the reference gives up, so does the product
    open(fa, "wb").write(b">a\nACGTACGTACGTACGTACGT\n>cut")
    r = run_cli(["dist", "-L", shuf, "--byread", "-o", out, fa], tmp_path, check=False)
    assert r.returncode != 0 and b"header" in r.stderr
