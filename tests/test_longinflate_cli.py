"""`dist -A --long-inflate` without a GPU: what the switch refuses, with exact text and status, before the device is
touched, and the surface of the three entry points behind it (header, built library, binding).  What the route computes is
tests/test_gpu_longinflate.py's business."""
import ctypes
import os
import re
import subprocess

import pytest

import test_cli_surface as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
run = cs.run


@pytest.fixture()
def world(tmp_path):
    fq = tmp_path / "a.fq.gz"
    fq.write_bytes(b"\x1f\x8b")  # never read: every refusal comes first, like the .shuf
    return dict(fq=str(fq), shuf=str(tmp_path / "none.shuf"), out=tmp_path / "o")


def refused(world, text, *args):
    assert run("dist", "-L", world["shuf"], "-o", world["out"], *args, world["fq"]) == (1, "", "metakssd: " + text + "\n")
    assert not world["out"].exists()


def test_without_A(world):
    refused(world, "--long-inflate needs -A: it is the route of the counted sketch", "--long-inflate")
    refused(world, "--long-inflate needs -A: it is the route of the counted sketch", "--long-reads", "--long-inflate")


@pytest.mark.parametrize("opt", [("-n", "2"), ("-Q", "20")])
def test_with_n_or_Q(world, opt):
    refused(world, "--long-inflate does not take -n or -Q: their reader frames lines of up to 19998 characters itself", "-A", "--long-inflate", *opt)
    refused(world, "--long-inflate does not take -n or -Q: their reader frames lines of up to 19998 characters itself", "-A", *opt, "--long-inflate")


def test_with_byread(world):
    for args in (["--byread", "--long-inflate"], ["--long-inflate", "-A", "--byread"]):
        refused(world, "--long-inflate does not go with --byread: per-read sketches keep the framing contract", *args)


def test_with_devices(world):
    refused(world, "--long-inflate works on one GPU: --device D, not --devices", "-A", "--long-inflate", "--devices", "0,1")
    refused(world, "--long-inflate works on one GPU: --device D, not --devices", "--devices", "0", "-A", "--long-inflate")


@pytest.mark.parametrize("opt", ["--device-inflate", "--device-gunzip"])
def test_with_a_short_read_inflate_switch(world, opt):
    line = "--long-inflate chooses the device route itself: not --device-inflate or --device-gunzip"
    refused(world, line, "-A", opt, "--long-inflate")
    refused(world, line, "-A", "--long-inflate", opt)
    refused(world, line, "-A", "--long-reads", "--long-inflate", opt)


def test_long_reads_keeps_its_own_line(world):
    """the switch this one implies refuses the same two with the line tests/test_longreads_model.py pins"""
    refused(world, "--long-reads reads .gz files through zcat: not --device-inflate or --device-gunzip", "-A", "--long-reads", "--device-gunzip")


def test_refusals_need_no_device(world):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args, line in ((["--long-inflate"], b"--long-inflate needs -A: it is the route of the counted sketch"),
                       (["-A", "--long-inflate", "--device-gunzip"], b"--long-inflate chooses the device route itself: not --device-inflate or --device-gunzip"),
                       (["-A", "--long-inflate", "--devices", "0,1"], b"--long-inflate works on one GPU: --device D, not --devices"),
                       (["-A", "--long-inflate", "-n", "2"], b"--long-inflate does not take -n or -Q: their reader frames lines of up to 19998 characters itself"),
                       (["--long-inflate", "--byread"], b"--long-inflate does not go with --byread: per-read sketches keep the framing contract")):
        r = subprocess.run([cs.CLI, "dist", "-L", world["shuf"], "-o", str(world["out"])] + args + [world["fq"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"metakssd: " + line + b"\n")
    assert not world["out"].exists()


def test_usage_does_not_change():
    """tests/test_cli_surface.py pins the usage text; the switch is documented in the README and in the option loop"""
    assert run() == (2, "", cs.USAGE)
    assert "--long-inflate" in open(os.path.join(ROOT, "README.md")).read()


PROTOS = {
    "mk_sketch_push_fastq_long_device": r"int mk_sketch_push_fastq_long_device\(mk_engine \*e, const uint8_t \*d_text, uint64_t n, int final\);",
    "mk_sketch_push_gzip_long": r"int mk_sketch_push_gzip_long\(mk_engine \*e, int fd, size_t size, const mk_gunzip_opts \*opts, int final, mk_gunzip_stats \*st\);",
    "mk_sketch_push_bgzf_long": r"int mk_sketch_push_bgzf_long\(mk_engine \*e, int fd, size_t size, const mk_bgzf_opts \*o, int final, mk_bgzf_stats \*st\);",
}


@pytest.mark.parametrize("name", sorted(PROTOS))
def test_symbol_in_header_library_and_binding(name):
    h = open(os.path.join(ROOT, "include", "metakssd_hip.h")).read()
    assert re.search(PROTOS[name], h)
    comment = h[:h.index("int %s(" % name)].rsplit("/*", 1)[1]  # every entry cites the rule it frames by
    assert "DESIGN.md 4.19's rule" in comment
    from metakssd_amd import capi
    assert getattr(capi.lib, name).argtypes is not None
    assert callable(getattr(capi.Engine, {"mk_sketch_push_fastq_long_device": "push_fastq_long_device", "mk_sketch_push_gzip_long": "push_gzip_long",
                                          "mk_sketch_push_bgzf_long": "push_bgzf_long"}[name]))
    built = ctypes.CDLL(capi.lib._name)  # the library as it was built, not the binding's table
    assert getattr(built, name) is not None
