"""tests/byread_model.py is what the GPU tests of `dist --byread` / `reverse` lean on, so it is pinned here, without a GPU:
it equals every fixture of tests/golden/byread (made by the reference, tests/golden/make_golden_byread.py) byte for byte, and,
where the compiled reference is at hand, the reference itself on seeded random FASTA texts."""
import gzip
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import byread_model as bm
from golden_cases import make_shuf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "byread")
REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))


def fixture_text(entry):
    if entry["input"] == "synthetic":
        return open(os.path.join(GOLD, "synthetic.fa"), "rb").read()
    return gzip.open(os.path.join(ROOT, "tests", "golden", "inputs", entry["input"])).read()


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


def test_fixture_tree_is_complete():
    """every file the manifest lists is there with the hash the generator recorded; the committed synthetic text is the model's"""
    for sec in ("cases", "reverse_cases"):
        for case, e in MANIFEST[sec].items():
            for f, h in e["files"].items():
                assert hashlib.sha256(open(os.path.join(GOLD, case, f), "rb").read()).hexdigest() == h, (case, f)
    assert open(os.path.join(GOLD, "synthetic.fa"), "rb").read() == bm.synthetic_text()
    sizes = [os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(GOLD) for f in fs]
    assert max(sizes) <= 256 << 10 and sum(sizes) < 1 << 20


@pytest.mark.parametrize("case", sorted(MANIFEST["cases"]))
def test_model_equals_byread_fixture(case, shuf_files, tmp_path):
    e = MANIFEST["cases"][case]
    shuf = shuf_files(e["shuf"])
    assert hashlib.sha256(open(shuf, "rb").read()).hexdigest() == e["shuf_sha256"]
    P = bm.Params.from_file(shuf)
    out = str(tmp_path / "out")
    bm.write_byread_dir(out, fixture_text(e), P, "/somewhere/" + e["name"])
    assert P.component_num == e["header"]["comp_num"]
    for c in range(P.component_num):
        for f in ("combco.%d" % c, "combco.index.%d" % c):
            assert open(os.path.join(out, f), "rb").read() == open(os.path.join(GOLD, case, f), "rb").read(), (case, f)
    st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
    assert {k: st[k] for k in e["header"]} == e["header"]
    assert st["names"] == ["/somewhere/" + e["recorded_name"]]
    assert bm.reverse_byread(out, P) == gzip.open(os.path.join(GOLD, case, "reverse_b.txt.gz")).read()


def test_synthetic_case_has_what_it_was_built_for():
    """a non-zero entry 0 (so that `reverse -b` prints shifted ids and drops the tail), an empty record, nine records"""
    idx = np.fromfile(os.path.join(GOLD, "synthetic_L0K6", "combco.index.0"), dtype="<u8")
    assert idx.size == 10 and idx[0] > 0
    assert np.any(np.diff(idx) == 0)
    text = gzip.open(os.path.join(GOLD, "synthetic_L0K6", "reverse_b.txt.gz")).read()
    assert text.count(b"\n") - text.count(b">read") == int(idx[-1] - idx[0])  # the last idx[0] ids are never printed


def build_sketch_dir(case, dst):
    """the sketch directory of a plain-reverse fixture: its combco files and a cofiles.stat rebuilt from the manifest"""
    e = MANIFEST["reverse_cases"][case]
    os.makedirs(dst)
    for f in e["files"]:
        if f.startswith("sketch/"):
            open(os.path.join(dst, f[7:]), "wb").write(open(os.path.join(GOLD, case, f), "rb").read())
    h = e["header"]
    with open(os.path.join(dst, "cofiles.stat"), "wb") as f:
        f.write(struct.pack("<IB3xiiiiQ", h["shuf_id"], h["koc"], h["kmerlen"], h["dim_rd_len"], h["comp_num"], h["infile_num"], h["all_ctx_ct"]))
        f.write(struct.pack("<%dI" % len(e["ctx_ct"]), *e["ctx_ct"]))
        for n in e["names"]:
            name = os.fsencode("/data/in put/" + n)
            f.write(name + b"\0" * (bm.PATHLEN - len(name)))
    return e


@pytest.mark.parametrize("case", sorted(MANIFEST["reverse_cases"]))
def test_model_equals_reverse_fixture(case, shuf_files, tmp_path):
    e = build_sketch_dir(case, str(tmp_path / "sk"))
    P = bm.Params.from_file(shuf_files(e["shuf"]))
    got = bm.reverse_dir(str(tmp_path / "sk"), P)
    assert sorted(got) == sorted(e["outputs"])
    assert 0 in e["ctx_ct"] and len(got) == len(e["ctx_ct"]) - 1  # the sketch without ids leaves no file
    for name, data in got.items():
        assert data == gzip.open(os.path.join(GOLD, case, "kmers", name + ".gz")).read(), (case, name)
        assert hashlib.sha256(data).hexdigest() == e["outputs"][name]


@pytest.mark.parametrize("shuf_name", ["L3K10", "L1K7", "L0K6", "L2K11"])
def test_model_equals_reference_on_random_fasta(shuf_name, shuf_files, tmp_path):
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/metakssd is not built here (the fixtures carry the comparison)")
    shuf = shuf_files(shuf_name)
    P = bm.Params.from_file(shuf)
    rs = np.random.RandomState({"L3K10": 310, "L1K7": 17, "L0K6": 6, "L2K11": 211}[shuf_name])
    for i in range(10):
        # texts below 65 536 bytes, so that no header lies across one of the reference's buffer refills
        text = bm.random_fasta(rs, nrec=int(rs.randint(1, 40)), min_len=0, max_len=int(rs.choice([30, 200, 1500])), width=int(rs.choice([7, 60, 80])),
                               lower=float(rs.choice([0.0, 0.3])), n_rate=float(rs.choice([0.0, 0.002])), crlf=bool(rs.randint(2)),
                               lead=int(rs.choice([0, 0, 90])))[:65000]
        if rs.randint(2):
            text = text.rstrip(b"\r\n")
        try:
            bm.base_stream(text)
        except ValueError:  # cut inside a header line: the reference gives up there
            text += b"\n"
        inp, out, mine = str(tmp_path / ("t%d.fa" % i)), str(tmp_path / ("ref%d" % i)), str(tmp_path / ("model%d" % i))
        open(inp, "wb").write(text)
        r = subprocess.run([REF, "dist", "-L", shuf, "--byread", "-p", "1", "-o", out, inp], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr[-300:]
        bm.write_byread_dir(mine, text, P, inp)
        for c in range(P.component_num):
            for f in ("combco.%d" % c, "combco.index.%d" % c):
                assert open(os.path.join(mine, f), "rb").read() == open(os.path.join(out, f), "rb").read(), (shuf_name, i, f)
        r = subprocess.run([REF, "reverse", "-L", shuf, "-b", out], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == bm.reverse_byread(mine, P), (shuf_name, i)
