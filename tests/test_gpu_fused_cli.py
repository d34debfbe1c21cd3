"""`metakssd dist -L <x.shuf> -A --composite <markerdb> <fastq>...`: reads to species report in one process, the sketch
staying on the device.  Its stdout is what `composite -r <markerdb> -q <dir>` prints for the directory `dist -A -o <dir>` writes from the
same inputs: pinned to the reference's own golden reports, and byte for byte to the product's two-step route on every reader route."""
import filecmp
import gzip
import json
import os
import subprocess

import pytest

import bgzf_util as bz
import composite_model as cm
import golden_cases as gc
import test_cli_surface as cs
import test_golden as tg

pytestmark = pytest.mark.gpu
shuf_files = tg.shuf_files
DIST = [tg.PRODUCT_CLI, "dist", "-p", "4"]


def run_cli(args, env=None):
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, (args, r.stderr.decode())
    return r.stdout


def fused(shuf, db, files, extra=(), env=None):
    return run_cli(DIST + ["-L", shuf, "-A", "--composite", db] + list(extra) + list(files), env)


# ---- the reference's golden reports -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(tg.MANIFEST["composite_cases"]))
def test_fused_reproduces_reference_golden(case, shuf_files, tmp_path):
    entry = tg.MANIFEST["composite_cases"][case]
    db, qsk = cm.build_marker_db(case, shuf_files, tmp_path, DIST, [tg.PRODUCT_CLI, "set"])
    _, qry = gc.build_composite_inputs(case, str(tmp_path))
    shuf = shuf_files(entry["shuf"])
    out = fused(shuf, db, qry)
    got = []
    for ln in out.decode().splitlines():
        f = ln.split("\t")
        f[0] = os.path.basename(f[0])
        got.append("\t".join(f))
    exp = os.path.join(gc.GOLDEN, "expected", case)
    assert got == open(os.path.join(exp, "composite.tsv")).read().splitlines()
    assert len(got) == entry["lines"] and len(got) > 0
    assert out == run_cli([tg.PRODUCT_CLI, "composite", "-r", db, "-q", qsk])      # the unedited bytes, against the two-step route
    abv = str(tmp_path / "abv")
    assert fused(shuf, db, qry, ["--abv", "--abv-dir", abv]) == b""
    want_abv = sorted(f for f in tg.golden_listing("expected/" + case) if f.endswith(".abv"))
    assert sorted(os.listdir(abv)) == want_abv and want_abv
    for f in want_abv:
        assert filecmp.cmp(os.path.join(exp, f), os.path.join(abv, f), shallow=False), f
    assert not any(n.startswith("combco") or n == "cofiles.stat" for n in os.listdir(os.getcwd()))     # no sketch directory, not even "."


# ---- routes and options -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(shuf_files, tmp_path_factory):
    """the marker database of composite_mix_L1K7, five samples of strain mixes (one of them without rows), and their two-step report"""
    tmp = tmp_path_factory.mktemp("fused_cli")
    mixes = [(0.7, 0.0, 0.3), (0.0, 1.0, 0.0), (0.2, 0.5, 0.3), (0.0, 0.1, 0.9), (1.0, 0.0, 0.0)]
    files = [cm.strain_mix_fastq(str(tmp / ("sample%d.fq" % i)), 300 + i, w) for i, w in enumerate(mixes)]
    db, q5 = cm.build_marker_db("composite_mix_L1K7", shuf_files, tmp, DIST, [tg.PRODUCT_CLI, "set"], query_files=files)
    want = run_cli([tg.PRODUCT_CLI, "composite", "-r", db, "-q", q5])
    assert len({ln.split(b"\t")[0] for ln in want.splitlines()}) >= 3
    return dict(db=db, files=files, want=want, shuf=shuf_files("L1K7"), tmp=tmp)


@pytest.mark.parametrize("poison", [None, "0xA5"])
def test_fused_equals_two_steps(world, poison):
    env = dict(os.environ, MK_POISON=poison) if poison else None
    assert fused(world["shuf"], world["db"], world["files"], env=env) == world["want"]
    # one sample: the two-step route takes its per-query join there
    one = world["files"][:1]
    q1 = str(world["tmp"] / ("q1_%s" % poison))
    run_cli(DIST + ["-L", world["shuf"], "-A", "-o", q1] + one)
    want1 = run_cli([tg.PRODUCT_CLI, "composite", "-r", world["db"], "-q", q1])
    assert want1.count(b"\n") > 0 and fused(world["shuf"], world["db"], one, env=env) == want1


def test_a_directory_of_samples_in_discover_order(world):
    """more than eight files (several engines would take turns in a plain dist): one engine, names and order as mk_sketchdir_add stores them"""
    d = world["tmp"] / "many"
    d.mkdir()
    for i in range(9):
        os.symlink(world["files"][i % 5], str(d / ("s%02d.fq" % (8 - i))))
    qd = str(world["tmp"] / "q_many")
    run_cli(DIST + ["-L", world["shuf"], "-A", "-o", qd, str(d)])
    want = run_cli([tg.PRODUCT_CLI, "composite", "-r", world["db"], "-q", qd])
    assert fused(world["shuf"], world["db"], [str(d)]) == want
    assert want.splitlines()[0].startswith(str(d).encode() + b"/s00.fq\t")


def test_batch_mib_0_is_a_sample_a_batch(world):
    out = fused(world["shuf"], world["db"], world["files"], ["--batch-mib", "0", "--timing"])
    lines = out.split(b"\n")
    t = [json.loads(ln)["composite_timing"] for ln in lines if ln.startswith(b'{"composite_timing"')]
    assert len(t) == 1 and t[0]["batches"] == 5 and t[0]["samples"] == 5
    assert b"\n".join(ln for ln in lines if not ln.startswith(b"{")) == world["want"]


def test_timing_lines(world):
    out = fused(world["shuf"], world["db"], world["files"], ["--timing"]).decode()
    tl = cs.timing_lines(out)
    assert len(tl) == 1 and list(tl[0]) == ["timing"] and list(tl[0]["timing"]) == cs.TIMING_KEYS
    assert tl[0]["timing"]["rows"] == 5 * 1500
    ct = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{"composite_timing"')]
    assert len(ct) == 1
    c = ct[0]["composite_timing"]
    assert list(c) == ["route", "samples", "batches", "hits", "load_kernel_ms", "query_kernel_ms"]       # composite's keys
    assert c["route"] == "device" and c["samples"] == 5 and c["batches"] == 1 and c["hits"] > 0
    assert c["load_kernel_ms"] > 0 and c["query_kernel_ms"] > 0
    assert "".join(ln + "\n" for ln in out.splitlines() if not ln.startswith("{")).encode() == world["want"]


def test_shuf_id_warning_comes_first(world):
    """a sample sketched with another table: composite's warning line, then whatever rows there are -- as the two steps print them"""
    from metakssd_amd import capi
    p = str(world["tmp"] / "L1K7_other.shuf")
    capi.Shuf.generate(7, 4, 1, 99).write(p)
    qd = str(world["tmp"] / "q_other")
    run_cli(DIST + ["-L", p, "-A", "-o", qd] + world["files"][:2])
    want = run_cli([tg.PRODUCT_CLI, "composite", "-r", world["db"], "-q", qd])
    assert want.startswith(b"get_species_abundance(): qry shuf_id ")
    assert fused(p, world["db"], world["files"][:2]) == want


def compressed_copies(world):
    """every sample gzip-compressed (one member, as gzip writes it) and BGZF-compressed, under the names the plain files have + .gz; the
    report's first field is the name, so the expected bytes are the plain report with the names changed"""
    out = {}
    for kind in ("gz", "bgzf"):
        d = world["tmp"] / kind
        if not d.exists():
            d.mkdir()
            for f in world["files"]:
                data = open(f, "rb").read()
                blob = gzip.compress(data, 6) if kind == "gz" else bz.write_bgzf(data, payload=20000)[0]
                (d / (os.path.basename(f) + ".gz")).write_bytes(blob)
        names = [str(d / (os.path.basename(f) + ".gz")) for f in world["files"]]
        want = world["want"]
        for f, n in zip(world["files"], names):
            want = want.replace(f.encode() + b"\t", n.encode() + b"\t")
        out[kind] = (names, want)
    return out


def test_gzip_samples_zcat_and_device_gunzip(world):
    names, want = compressed_copies(world)["gz"]
    assert want != world["want"]
    assert fused(world["shuf"], world["db"], names) == want                            # zcat
    assert fused(world["shuf"], world["db"], names, ["--device-gunzip"]) == want
    # the routes were the ones meant
    out = fused(world["shuf"], world["db"], names[:1], ["--device-gunzip", "--timing"]).decode()
    routes = [json.loads(ln)["route"] for ln in out.splitlines() if ln.startswith('{"input"')]
    assert routes == ["device-gunzip"], out[-600:]
    out = fused(world["shuf"], world["db"], names[:1], ["--timing"]).decode()
    assert [json.loads(ln)["route"] for ln in out.splitlines() if ln.startswith('{"input"')] == ["zcat"]


def test_bgzf_samples(world):
    names, want = compressed_copies(world)["bgzf"]
    assert fused(world["shuf"], world["db"], names) == want
    out = fused(world["shuf"], world["db"], names[:1], ["--timing"]).decode()
    routes = [json.loads(ln)["route"] for ln in out.splitlines() if ln.startswith('{"input"')]
    assert routes == ["device-inflate"], out[-600:]
    assert fused(world["shuf"], world["db"], names, ["--no-device-inflate"]) == want     # and its fall-back, zcat
