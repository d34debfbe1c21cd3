"""`composite -r <ref> -i` and `composite -r <ref> -s <0|1|2> <x.abv>...` (index_abv() / abv_search(), command_composite.c:212-440):
the index files and the stdout of the three metrics, byte for byte, against the numpy restatement in abv_model.py, against the
compiled reference (oracle/_ref/metakssd) where it exists, and against the reference's committed output in tests/golden/abv."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import abv_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "abv")
SUFFIXES = ("name", "yl2n", "abm", "abmi")


def run(cmd, ok=True):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if ok:
        assert r.returncode == 0, (cmd, r.stderr.decode(errors="replace")[-2000:])
    return r


def index_files(root):
    return {k: open(os.path.join(root, "abundance_Vec." + k), "rb").read() for k in SUFFIXES}


def make_db(root, rs, nsamples, nref, lo, hi, extras=True):
    """nsamples random vectors of lo..hi species; with extras the edge cases: two copies of one file (exact ties), a species
    listed twice in one file, an empty file, an all-zero vector (NaN cosines) and a file that is not a .abv"""
    files = [("s%06d.abv" % i, am.random_vec(rs, nref, int(rs.randint(lo, hi + 1)))) for i in range(nsamples)]
    if extras:
        files.append(("copyA.abv", files[0][1]))
        files.append(("copyB.abv", files[0][1]))
        rep = am.random_vec(rs, nref, 12)
        files.append(("repeat.abv", np.concatenate([rep, rep[2:5]])))
        files.append(("empty.abv", np.zeros(0, am.BINVEC)))
        files.append(("zeros.abv", am.random_vec(rs, nref, 9, zero=True)))
        files.append(("readme.txt", am.random_vec(rs, nref, 4)))
    am.write_db(root, nref, files)


def queries_for(root, qdir, rs, nref, nq, k):
    """query arguments: relative names (resolved under <ref>/abundance_Vec), then paths with '/': random vectors, one with a
    species repeated, one of a species no sample holds, an all-zero one, an empty one.  (Relative after absolute would send the
    reference's sprintf into argv, :245-247.)"""
    os.makedirs(qdir, exist_ok=True)
    names = am.dir_order(root)
    rel = [(n, am.read_vec(os.path.join(root, "abundance_Vec", n))) for n in names[:min(3, len(names))]]
    rel.append(("not_a_vector.txt", None))
    ab = []
    held = set()
    for n in names:
        held.update(am.read_vec(os.path.join(root, "abundance_Vec", n))["r"].tolist())
    unheld = [r for r in range(nref) if r not in held]
    for i in range(nq):
        q = am.random_vec(rs, nref, k)
        if i == 1:
            q = np.concatenate([q, q[:3]])
        if i == 2 and unheld:
            q = np.concatenate([q, np.array([(unheld[0], 7.5)], am.BINVEC)])
        ab.append(q)
    ab.append(am.random_vec(rs, nref, 5, zero=True))
    ab.append(np.zeros(0, am.BINVEC))
    out = []
    for i, q in enumerate(ab):
        p = os.path.join(qdir, "q%03d.abv" % i)
        q.tofile(p)
        out.append((p, q))
    return rel + out


def check_db(tmp_path, rs, nsamples, nref, lo, hi, nq, k, extras=True):
    root = str(tmp_path / "db")
    make_db(root, rs, nsamples, nref, lo, hi, extras)
    run([CLI, "composite", "-r", root, "-i"])
    got = index_files(root)
    want = am.index_model(root, nref)
    for s in SUFFIXES:
        assert got[s] == want[s], "abundance_Vec.%s differs from the restatement" % s
    qs = queries_for(root, str(tmp_path / "q"), rs, nref, nq, k)
    idx = am.read_index(root)
    outs = {}
    for metric in (0, 1, 2):
        r = run([CLI, "composite", "-r", root, "-s", str(metric)] + [a for a, _ in qs])
        outs[metric] = r.stdout
        assert r.stdout.decode() == am.search_stdout(idx, qs, metric), "metric %d" % metric
    return root, qs, got, outs


@pytest.mark.gpu
@pytest.mark.parametrize("nsamples,nref,lo,hi,nq,k", [
    (300, 500, 0, 40, 1, 20),
    (2000, 3000, 1, 120, 8, 60),
    (20000, 85205, 20, 300, 16, 300),
])
def test_index_and_search_match_restatement(tmp_path, nsamples, nref, lo, hi, nq, k):
    check_db(tmp_path, np.random.RandomState(nsamples), nsamples, nref, lo, hi, nq, k)


@pytest.mark.gpu
def test_large_database_64_queries(tmp_path):
    """about 200 k samples over the 85 205 species of the GTDB r214 marker database, 64 queries in one batch"""
    check_db(tmp_path, np.random.RandomState(214), 200000, 85205, 5, 40, 64, 300, extras=False)


@pytest.mark.gpu
def test_against_compiled_reference(tmp_path):
    """the same directory indexed and searched by both programs: index files and stdout byte for byte, ties and NaN included"""
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/metakssd not built (needs the reference sources)")
    root, qs, got, outs = check_db(tmp_path, np.random.RandomState(77), 1500, 2000, 0, 80, 6, 50)
    run([REF, "composite", "-r", root, "-i"])
    assert index_files(root) == got
    for metric in (0, 1, 2):
        r = run([REF, "composite", "-r", root, "-s", str(metric)] + [a for a, _ in qs])
        assert r.stdout == outs[metric], "metric %d" % metric
    assert b"-nan" in outs[0]


@pytest.mark.gpu
def test_reproduces_committed_reference_output(tmp_path):
    """tests/golden/abv: the reference's four index files, the query vectors and its stdout (make_golden_abv.py)"""
    root = str(tmp_path / "db")
    os.makedirs(os.path.join(root, "abundance_Vec"))
    for s in SUFFIXES:
        shutil.copy(os.path.join(GOLDEN, "abundance_Vec." + s), root)
    qs = sorted(n for n in os.listdir(GOLDEN) if n.endswith(".abv"))
    args = [os.path.join(GOLDEN, n) for n in qs]
    for metric in (0, 1, 2):
        r = run([CLI, "composite", "-r", root, "-s%d" % metric] + args)
        assert r.stdout == open(os.path.join(GOLDEN, "search_s%d.txt" % metric), "rb").read(), "metric %d" % metric


@pytest.mark.gpu
def test_reference_made_vectors_end_to_end(tmp_path):
    """the .abv files the reference's `composite -b` wrote for the golden composite cases, indexed and searched"""
    exp = os.path.join(ROOT, "tests", "golden", "expected")
    root = str(tmp_path / "db")
    files = []
    for case in sorted(os.listdir(exp)):
        for n in sorted(os.listdir(os.path.join(exp, case))):
            if n.endswith(".abv"):
                files.append((case + "_" + n, am.read_vec(os.path.join(exp, case, n))))
    assert len(files) >= 2
    nref = int(max(int(v["r"].max()) for _, v in files if len(v)) + 1)
    am.write_db(root, nref, files + [(n.replace(".abv", "_again.abv"), v) for n, v in files])
    run([CLI, "composite", "-r", root, "-i"])
    assert index_files(root) == am.index_model(root, nref)
    idx = am.read_index(root)
    qs = [(n, v) for n, v in files]
    for metric in (0, 1, 2):
        r = run([CLI, "composite", "-r", root, "-s", str(metric)] + [n for n, _ in qs])
        assert r.stdout.decode() == am.search_stdout(idx, qs, metric)


@pytest.mark.gpu
def test_measures_are_not_contracted():
    """the float measures through the C ABI, bit for bit: 4 000 products summed into one sample.  A build that fuses
    acc += a * b into one fma rounds differently (checked once with a build that contracts)"""
    from metakssd_amd import capi
    rs = np.random.RandomState(3)
    nref = 4000
    v = np.zeros(nref, am.BINVEC)
    v["r"] = np.arange(nref)
    v["p"] = (rs.rand(nref) * 3.0 + 0.01).astype(np.float32)
    q = v.copy()
    q["p"] = (rs.rand(nref) * 3.0 + 0.01).astype(np.float32)
    other = am.random_vec(rs, nref, 50)
    a = capi.Abv(0)
    try:
        abm, abmi, yl2n = a.index([v, other], nref)
        a.load(abm, abmi, yl2n)
        idx = (["v", "o"], yl2n, abm.view(am.BINVEC), abmi)
        for metric in (0, 1, 2):
            (ids, ms), = a.search(metric, [q])
            wids, wms = am.search_model(idx, q, metric)
            assert np.array_equal(ids, wids)
            assert ms.view(np.uint32).tolist() == wms.view(np.uint32).tolist(), "metric %d" % metric
        assert a.last_kernel_ms()[1] > 0
    finally:
        a.close()


@pytest.mark.gpu
def test_species_outside_the_database_is_rejected(tmp_path):
    """ref_idx == nref: the reference writes past its arrays (:390-397); here -i fails and names the file, writing nothing.
    A query species outside the index is refused the same way."""
    root = str(tmp_path / "db")
    rs = np.random.RandomState(1)
    bad = am.random_vec(rs, 50, 5)
    bad["r"][2] = 50
    am.write_db(root, 50, [("fine.abv", am.random_vec(rs, 50, 5)), ("broken.abv", bad)])
    r = run([CLI, "composite", "-r", root, "-i"], ok=False)
    assert r.returncode != 0 and b"broken.abv" in r.stderr
    assert not os.path.exists(os.path.join(root, "abundance_Vec.abm"))
    os.remove(os.path.join(root, "abundance_Vec", "broken.abv"))
    run([CLI, "composite", "-r", root, "-i"])
    qp = str(tmp_path / "q.abv")
    bad.tofile(qp)
    r = run([CLI, "composite", "-r", root, "-s", "1", qp], ok=False)
    assert r.returncode != 0 and b"q.abv" in r.stderr


# ---- host-only paths: no device needed ---------------------------------------------------------------------------------
def empty_index(tmp_path):
    root = str(tmp_path / "db")
    os.makedirs(os.path.join(root, "abundance_Vec"))
    for s in SUFFIXES:
        open(os.path.join(root, "abundance_Vec." + s), "wb").close()
    return root


@pytest.mark.parametrize("arg", [["-s", "3"], ["-s7"], ["-s", "-2"]])
def test_search_metric_out_of_range_prints_usage(tmp_path, arg):
    root = empty_index(tmp_path)
    r = run([CLI, "composite", "-r", root] + arg + ["x.abv"])
    assert r.stdout == b"\vUsage: metakssd composite -r <ref> -s <0|1|2> <query.abv>\n\v"


def test_search_without_vectors_and_without_mode_print_usage(tmp_path):
    root = empty_index(tmp_path)
    assert run([CLI, "composite", "-r", root, "-s", "0"]).stdout == b"\vUsage: metakssd composite -r <ref> -s <0|1|2> <query.abv>\n\v"
    assert run([CLI, "composite", "-r", root]).stdout == b"\vUsage: metakssd composite -r <ref> < mode: -q | -i | -s >\n\v"
    # -s -1 is the reference's "unset" (:55): no mode
    assert run([CLI, "composite", "-r", root, "-s", "-1", "x.abv"]).stdout == b"\vUsage: metakssd composite -r <ref> < mode: -q | -i | -s >\n\v"


def test_search_skips_arguments_that_are_not_abv(tmp_path):
    root = empty_index(tmp_path)
    r = run([CLI, "composite", "-r", root, "-s1", "notes.txt", "table.tsv"])
    assert r.stdout == (b"0th argument notes.txt is not a .abv file, skipped\n"
                        b"1th argument table.tsv is not a .abv file, skipped\n")


def test_model_reproduces_committed_reference_output():
    """the restatement the GPU tests compare with gives the reference's committed stdout (a check of the yardstick itself)"""
    idx = am.read_index(GOLDEN)
    qs = sorted(n for n in os.listdir(GOLDEN) if n.endswith(".abv"))
    args = [(os.path.join(GOLDEN, n), am.read_vec(os.path.join(GOLDEN, n))) for n in qs]
    for metric in (0, 1, 2):
        assert am.search_stdout(idx, args, metric).encode() == open(os.path.join(GOLDEN, "search_s%d.txt" % metric), "rb").read()
