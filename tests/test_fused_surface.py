"""`metakssd dist -A --composite <markerdb>`: what the fused form refuses, with the exact text and exit status, each
decided before the device is touched -- these run on a machine without a GPU."""
import os
import subprocess

import pytest

import test_cli_surface as cs

run = cs.run


@pytest.fixture()
def world(tmp_path):
    """a marker directory with a (whole) cofiles.stat of no sketches, a directory without one, a FASTQ and a FASTA input, and a name for the
    .shuf file that is never read: every refusal comes first"""
    db = tmp_path / "db"
    db.mkdir()
    (db / "cofiles.stat").write_bytes(cs.co_header(0))
    (tmp_path / "nodb").mkdir()
    fq = tmp_path / "a.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">g\nACGT\n")
    gz = tmp_path / "b.fastq.gz"
    gz.write_bytes(b"")
    return dict(db=str(db), nodb=str(tmp_path / "nodb"), fq=str(fq), fa=str(fa), gz=str(gz), shuf=str(tmp_path / "none.shuf"), tmp=tmp_path)


def refused(text, *args):
    assert run("dist", *args) == (1, "", "metakssd: " + text + "\n")


def test_without_A(world):
    refused("--composite needs -A: the report reads the k-mer counts", "-L", world["shuf"], "--composite", world["db"], world["fq"])


@pytest.mark.parametrize("opt", [("-n", "2"), ("-Q", "20"), ("-n", "1")])
def test_with_n_or_Q(world, opt):
    refused("--composite does not take -n or -Q: the report reads every k-mer of the reads", "-L", world["shuf"], "-A", "--composite", world["db"],
            *opt, world["fq"])


def test_with_devices(world):
    refused("--composite works on one GPU: --device D, not --devices", "-L", world["shuf"], "-A", "--composite", world["db"], "--devices", "0,1",
            world["fq"])
    refused("--composite works on one GPU: --device D, not --devices", "-L", world["shuf"], "-A", "--devices", "0", "--composite", world["db"],
            world["fq"])


@pytest.mark.parametrize("n", [2, 4])
def test_with_several_engines(world, n):
    refused("--composite works with one engine: not --engines %d" % n, "-L", world["shuf"], "-A", "--composite", world["db"], "--engines", n,
            world["fq"])


def test_with_an_output_directory(world):
    out = world["tmp"] / "out"
    refused("--composite keeps the sketch on the device; for a directory run dist -o and composite -q", "-L", world["shuf"], "-A", "-o", out,
            "--composite", world["db"], world["fq"])
    assert not out.exists()


def test_marker_directory_without_cofiles_stat(world):
    """composite's own text (cmd_composite(): `cannot find cofiles.stat under <dir> `, with its trailing blank)"""
    refused("cannot find cofiles.stat under %s " % world["nodb"], "-L", world["shuf"], "-A", "--composite", world["nodb"], world["fq"])
    missing = str(world["tmp"] / "not_there")
    refused("cannot find cofiles.stat under %s " % missing, "-L", world["shuf"], "-A", "--composite", missing, world["fq"])
    rc, out, err = run("composite", "-r", world["nodb"], "-q", world["db"])
    assert (rc, out, err) == (1, "", "metakssd: cannot find cofiles.stat under %s \n" % world["nodb"])


def test_input_that_is_no_fastq(world):
    refused("--composite takes FASTQ inputs: %s is none" % world["fa"], "-L", world["shuf"], "-A", "--composite", world["db"], world["fa"])
    refused("--composite takes FASTQ inputs: %s is none" % world["fa"], "-L", world["shuf"], "-A", "--composite", world["db"], world["fq"],
            world["gz"], world["fa"])
    # a directory is looked into, as discover() does for every dist
    d = world["tmp"] / "reads"
    d.mkdir()
    (d / "x.fq").write_bytes(b"")
    (d / "y.fna").write_bytes(b"")
    refused("--composite takes FASTQ inputs: %s/y.fna is none" % d, "-L", world["shuf"], "-A", "--composite", world["db"], d)


def test_order_of_the_switches_does_not_matter(world):
    refused("--composite keeps the sketch on the device; for a directory run dist -o and composite -q", "--composite", world["db"], world["fq"],
            "-A", "-L", world["shuf"], "-o", world["tmp"] / "o2")


def test_usage_does_not_change():
    """tests/test_cli_surface.py pins the text; the fused form is documented in README and in the option loop"""
    assert run() == (2, "", cs.USAGE)


def test_no_inputs(world):
    refused("please specify the input/query files", "-L", world["shuf"], "-A", "--composite", world["db"])


def test_refusals_need_no_device(world):
    """the same with the device hidden from the process"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([cs.CLI, "dist", "-L", world["shuf"], "-A", "--composite", world["db"], "-n", "3", world["fq"]], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"metakssd: --composite does not take -n or -Q: the report reads every k-mer of the reads\n")
