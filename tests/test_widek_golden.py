"""Wide k-mers (k 12-16, tests/widek_cases.py) without a GPU: the fixtures of tests/golden/widek were made by the REAL reference
(tests/golden/make_golden_widek.py, -p 1); here the oracle CLI reproduces every `dist` directory byte for byte (cofiles.stat
field-wise: the reference leaves padding bytes uninitialised), tests/byread_model.py reproduces the by-read ids and both reverse
texts, the .shuf generator and the seeded inputs reproduce the pinned sha256s, and the conditions the inputs were planted for hold
on the ORACLE's output as they held on the reference's when the fixtures were made -- an input that shrank to nothing fails here.
The three heavy geometries (536 870 909 slots, a 4.3 GB oracle table per run) run like test_golden.py's heavy cases: as they are."""
import gzip
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import byread_model as bm
import widek_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "widek")
ORACLE_CLI = os.path.join(ROOT, "oracle", "kssd_oracle_cli")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
CASES, BYREAD_CASES, REVERSE_CASES = MANIFEST["cases"], MANIFEST["byread_cases"], MANIFEST["reverse_cases"]


def sha_file(p):
    h = hashlib.sha256()
    with open(p, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


@pytest.fixture(scope="module")
def shuf_files(tmp_path_factory):
    """geometry -> path of its .shuf (the (16,7,7) table is 1 GiB: written once per module)"""
    d = tmp_path_factory.mktemp("widek_shufs")
    made = {}

    def get(name):
        if name not in made:
            p = str(d / (name + ".shuf"))
            wc.get_shuf(name).write(p)
            made[name] = p
        return made[name]
    yield get
    for p in made.values():
        os.remove(p)


def write_input(geom, kind, d):
    inp = wc.get_input(geom)
    p = os.path.join(str(d), "%s.%s" % (geom, kind))
    if not os.path.exists(p):
        open(p, "wb").write(inp.fasta() if kind == "fa" else inp.fastq())
    return p


def check_dist_dir(case, out, input_path):
    """a `dist` output directory against the reference-made fixture of `case`"""
    e = CASES[case]
    got = sorted(f for f in os.listdir(out) if f.startswith("combco"))
    assert got and sorted(wc.fixture_name(f) for f in got) == sorted(e["files"])
    for f in got:
        assert open(os.path.join(out, f), "rb").read() == open(os.path.join(GOLD, case, wc.fixture_name(f)), "rb").read(), "%s: %s differs" % (case, f)
    st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
    assert {k: st[k] for k in e["stat"]} == e["stat"]
    assert st["names"] == [input_path]


def build_sketch_dir(case, dst):
    """the sketch directory of a plain-reverse fixture: its combco files and a cofiles.stat rebuilt from the manifest"""
    e = REVERSE_CASES[case]
    os.makedirs(dst)
    for f in e["files"]:
        if f.startswith("sketch/"):
            open(os.path.join(dst, f[7:]), "wb").write(open(os.path.join(GOLD, case, f), "rb").read())
    h = e["header"]
    with open(os.path.join(dst, "cofiles.stat"), "wb") as f:
        f.write(struct.pack("<IB3xiiiiQ", h["shuf_id"], h["koc"], h["kmerlen"], h["dim_rd_len"], h["comp_num"], h["infile_num"], h["all_ctx_ct"]))
        f.write(struct.pack("<%dI" % len(e["ctx_ct"]), *e["ctx_ct"]))
        for n in e["names"]:
            name = os.fsencode("/data/wide/" + n)
            f.write(name + b"\0" * (bm.PATHLEN - len(name)))
    return e


def load_components(d, C, counts=False):
    ids = [np.fromfile(os.path.join(d, "combco.%d" % c), dtype="<u4") for c in range(C)]
    if not counts:
        return ids
    return ids, [np.fromfile(os.path.join(d, "combco.%d.a" % c), dtype="<u2") for c in range(C)]


def test_manifest_covers_every_geometry_and_flavour():
    assert sorted(MANIFEST["geometries"]) == sorted(wc.GEOMS)
    assert sorted(CASES) == sorted(g + "_" + f for g in wc.GEOMS for f in wc.FLAVOURS)
    assert sorted(BYREAD_CASES) == sorted(g + "_byread" for g in wc.BYREAD)
    assert sorted(REVERSE_CASES) == sorted(g + "_reverse" for g in wc.BYREAD)
    for g, e in MANIFEST["geometries"].items():
        assert (e["k"], e["subk"], e["drlevel"], e["seed"]) == wc.GEOMS[g] and e["clamped"] == wc.clamped(g)
        assert e["clamped"] == (g != "W12S6D3")
        c = e["conditions"]  # recorded from the reference's output when the fixtures were made
        assert c["distinct_keys_A"] >= wc.MIN_KEYS[g] and c["fwd_canonical_windows"] > 0 and c["rc_canonical_windows"] > 0 and c["max_count"] > 1
        assert (c["colliding_unituples"] > 0) == e["clamped"]
        if e["k"] >= 13:
            assert c["top_bit_unituples"] > 0 and c["keys_beyond_44_bit_unituple"] > 0
    c = MANIFEST["geometries"][wc.SATURATE]
    assert 26000 <= c["conditions"]["distinct_keys_A"] <= 60000 and c["conditions"]["max_count"] == 65535 and c["hashsize"] == 131071


def test_fixture_tree_equals_manifest():
    """every file the manifest lists is there with the recorded hash, nothing unlisted beside them, nothing above 256 KiB"""
    want = {}
    for sec in ("cases", "byread_cases", "reverse_cases"):
        for case, e in MANIFEST[sec].items():
            assert e["files"], case
            for f, h in e["files"].items():
                want[os.path.join(case, f)] = h
    have = {os.path.relpath(os.path.join(dp, f), GOLD) for dp, _, fs in os.walk(GOLD) for f in fs} - {"manifest.json"}
    assert have == set(want), (sorted(have - set(want))[:5], sorted(set(want) - have)[:5])
    assert not [f for f in have if f.endswith(".a")] and sum(f.endswith(".a.u16") for f in have) == sum(
        CASES[g + "_fq_A"]["stat"]["comp_num"] for g in wc.GEOMS)  # every -A case carries its 16-bit counts, as combco.N.a.u16
    for rel, h in want.items():
        assert sha_file(os.path.join(GOLD, rel)) == h, "fixture changed: " + rel
        assert os.path.getsize(os.path.join(GOLD, rel)) <= 256 << 10, rel


@pytest.mark.parametrize("geom", list(wc.GEOMS))
def test_shuf_generator_and_inputs_are_stable(geom, shuf_files):
    """the seeded .shuf generator and the seeded planted inputs keep producing the bytes the reference was run on"""
    e = MANIFEST["geometries"][geom]
    assert sha_file(shuf_files(geom)) == e["shuf_sha256"]
    inp = wc.get_input(geom)
    assert hashlib.sha256(inp.fasta()).hexdigest() == e["fasta_sha256"]
    assert hashlib.sha256(inp.fastq()).hexdigest() == e["fastq_sha256"]
    TL = 2 * e["k"]
    assert sorted({len(r) for r in inp.rows[:3]}) == [TL - 1, TL, TL + 1] and max(len(r) for r in inp.rows) == 150
    assert sum(r.count(b"N") == 1 and len(r) == TL + 20 for r in inp.rows) == TL  # an N at each of the 2k positions
    assert (len(inp.rows) - len(inp.body) == 69999) == (geom == wc.SATURATE)


@pytest.fixture(scope="module")
def oracle_dirs(shuf_files, tmp_path_factory):
    """case -> (output directory of the oracle CLI, input path); every case runs once per module"""
    d = tmp_path_factory.mktemp("widek_oracle")
    made = {}

    def get(case):
        if case not in made:
            e = CASES[case]
            inp = write_input(e["geometry"], e["input"], d)
            out = str(d / (case + ".out"))
            r = subprocess.run([ORACLE_CLI, "-L", shuf_files(e["geometry"])] + e["flags"] + ["-o", out, inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 0, r.stderr.decode()
            made[case] = (out, inp)
        return made[case]
    return get


@pytest.mark.parametrize("case", sorted(CASES))
def test_oracle_reproduces_reference_dist(case, oracle_dirs):
    out, inp = oracle_dirs(case)
    check_dist_dir(case, out, inp)


@pytest.mark.parametrize("geom", list(wc.GEOMS))
def test_planted_conditions_hold_on_the_oracle_output(geom, oracle_dirs):
    """distinct keys, top bits, both strands, counts, colliding unituples, sixteen non-empty components: asserted on what the oracle
    computes now, and equal to the counts recorded from the reference's output"""
    C = CASES[geom + "_fq_A"]["stat"]["comp_num"]
    ids, counts = load_components(oracle_dirs(geom + "_fq_A")[0], C, counts=True)
    got = wc.check_conditions(geom, ids, counts, load_components(oracle_dirs(geom + "_fa")[0], C))
    assert got == MANIFEST["geometries"][geom]["conditions"]
    n2 = load_components(oracle_dirs(geom + "_fq_n2Q53")[0], C)
    assert 100 <= sum(len(x) for x in n2) < got["distinct_keys_A"]  # -n 2 drops the keys seen once, -Q 53 some windows


@pytest.mark.parametrize("case", sorted(BYREAD_CASES))
def test_model_reproduces_reference_byread(case, tmp_path):
    e = BYREAD_CASES[case]
    P = wc.params(e["geometry"])
    text = wc.get_input(e["geometry"]).fasta()
    out = str(tmp_path / "out")
    bm.write_byread_dir(out, text, P, "/somewhere/x.fa")
    assert P.component_num == e["header"]["comp_num"]
    for c in range(P.component_num):
        for f in ("combco.%d" % c, "combco.index.%d" % c):
            assert open(os.path.join(out, f), "rb").read() == open(os.path.join(GOLD, case, f), "rb").read(), (case, f)
    st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
    assert {k: st[k] for k in e["header"]} == e["header"]
    want = gzip.open(os.path.join(GOLD, case, "reverse_b.txt.gz")).read()
    assert hashlib.sha256(want).hexdigest() == e["reverse_b_sha256"] and want.count(b"\n") - want.count(b">read") == e["ids"] >= wc.MIN_KEYS[e["geometry"]]
    assert bm.reverse_byread(out, P) == want


@pytest.mark.parametrize("case", sorted(REVERSE_CASES))
def test_model_reproduces_reference_reverse(case, tmp_path):
    e = build_sketch_dir(case, str(tmp_path / "sk"))
    P = wc.params(e["geometry"])
    got = bm.reverse_dir(str(tmp_path / "sk"), P)
    assert sorted(got) == sorted(e["outputs"]) and len(got) == 2 and e["ctx_ct"][1] == 0  # the sketch without ids leaves no file
    for name, data in got.items():
        assert data == gzip.open(os.path.join(GOLD, case, "kmers", name + ".gz")).read(), (case, name)
        assert hashlib.sha256(data).hexdigest() == e["outputs"][name]


def test_recovered_kmers_occur_in_the_text_only_where_the_subspace_is_not_clamped():
    """`reverse` is meaningful at (12,6,3); at a clamped geometry pf overlaps the outer context and the recovered k-mers are
    (almost) never substrings of the input -- pinned as the reference prints them all the same"""
    def share(geom):
        text = b"".join(ln for ln in wc.get_input(geom).fasta().upper().split(b"\n") if not ln.startswith(b">"))
        both = text + b"|" + text.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]
        e = REVERSE_CASES[geom + "_reverse"]
        lines = gzip.open(os.path.join(GOLD, geom + "_reverse", "kmers", e["inputs"][0] + ".gz")).read().split(b"\n")[:200]
        return sum(ln in both for ln in lines) / 200.0
    assert share("W12S6D3") == 1.0
    assert share("W13S6D5") < 0.1 and share("W16S7D7") < 0.1
