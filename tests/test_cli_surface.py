"""The command line's surface: exit statuses and the exact texts of `metakssd` where it decides without the device -- usage, the
option errors of `set` and `dist`, dist_dispatch()'s choices, what the readers of cofiles.stat say about a missing or truncated file --
and, on the GPU, the keys of the --timing line (the contract with bench.py) and the batch path of stage I against the serial one."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import util_inputs as ui

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
PATHLEN = 256

USAGE = (
    "usage: metakssd dist -L <file.shuf> [-A] [-u] [-n minocc] [-Q minqual] [-o outdir] [-p N] [--device D | --devices 0-7] [--engines 1..4] [--no-batch | --batch-text] <fastq|fasta|dir>...\n"
    "       metakssd dist -o <mco dir> <sketch dir>                      (stage II: inverted index)\n"
    "       metakssd dist -L <file.shuf> -r <genomes> -o <db dir>         (stage I + II)\n"
    "       metakssd dist -r <mco dir> -o <outdir> [-M 0|1] [-O 0|1|2] [-N n] [-D d] [--correction 0|1] [--keepskf] [-f skf] <sketch dir>\n"
    "       metakssd dist -L <file.shuf> --byread -o <outdir> [--device D] <one plain fasta|fastq file>   (ids per record, repeats kept)\n"
    "       metakssd reverse -L <file.shuf> [-o outdir] [-p N] [--device D] <sketch dir>   (k-mers of every sketch into <outdir>/<name>)\n"
    "       metakssd reverse -L <file.shuf> -b [--device D] <byread dir>                   (k-mers per read to stdout)\n"
    "       metakssd set -u|-q|-i <pan dir>|-s <pan dir>|-g <tax.tsv>|-c|-P [-o outdir] [--device D] <sketch dir>\n"
    "       metakssd composite -r <marker db dir> -q <-A sketch dir> [-b] [-o outdir] [--device D]\n"
    "       metakssd composite -d <x.abv>...\n"
    "       metakssd composite -r <marker db dir> -i [--device D]                 (index <dir>/abundance_Vec/*.abv)\n"
    "       metakssd composite -r <marker db dir> -s <0|1|2> [--device D] <x.abv>...  (0 cosine, 1 L1, 2 L2)\n"
    "       metakssd shuffle -k <halfK> -s <halfSubK> -l <level> [--seed N] -o <prefix>\n")


def run(*args, cwd=None, env=None):
    r = subprocess.run([CLI] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=cwd, env=env)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def co_header(infile_num, shuf_id=77, koc=0, kmerlen=14, dim_rd_len=2, comp_num=1, all_ctx_ct=0):
    """co_dstat_t (global_basic.h:116-126): shuf_id, koc, kmerlen, dim_rd_len, comp_num, infile_num, all_ctx_ct"""
    return struct.pack("<IB3xiiiiQ", shuf_id, koc, kmerlen, dim_rd_len, comp_num, infile_num, all_ctx_ct)


@pytest.fixture()
def truncated(tmp_path):
    """a directory whose cofiles.stat is a 32-byte header that claims three sketches, with no record behind it"""
    d = tmp_path / "trunc"
    d.mkdir()
    (d / "cofiles.stat").write_bytes(co_header(3))
    return str(d)


def test_no_arguments_prints_the_usage():
    assert run() == (2, "", USAGE)


def test_unknown_command():
    assert run("frobnicate") == (1, "", "metakssd: only `dist`, `set`, `composite`, `reverse` and `shuffle` are part of this build (got `frobnicate`)\n")


def test_set_unknown_option():
    assert run("set", "--bogus", "x") == (1, "", "metakssd: set option --bogus is not part of this build (-u -q -i -s -g -c -P are)\n")


def test_set_without_an_operation():
    assert run("set", "x") == (255, "set operation use : -u, -q, -i or -s\n", "")


def test_set_P_without_cofiles_stat(tmp_path):
    assert run("set", "-P", tmp_path) == (1, "", "metakssd: cannot find cofiles.stat under %s \n" % tmp_path)


def test_set_P_on_a_truncated_cofiles_stat(truncated):
    assert run("set", "-P", truncated) == (1, "", "metakssd: sketch_union():%s/cofiles.stat\n" % truncated)


def test_set_P_prints_counts_and_names(tmp_path):
    """two sketches; the second name fills its 256 bytes without a terminating NUL: "%.*s" stops at the record's end"""
    full = b"n" * PATHLEN
    (tmp_path / "cofiles.stat").write_bytes(co_header(2, all_ctx_ct=12) + struct.pack("<2I", 5, 7) + b"first.fa".ljust(PATHLEN, b"\0") + full)
    assert run("set", "-P", tmp_path) == (0, "5\tfirst.fa\n7\t%s\n" % full.decode(), "")


def test_dist_unknown_option():
    assert run("dist", "--bogus") == (1, "", "metakssd: option --bogus is not part of the sketching path built here\n")


def test_dist_without_L():
    assert run("dist", "x.fa") == (1, "", "metakssd: -L <file.shuf> is required (numeric levels generate a time-seeded table in the reference; use `metakssd shuffle`)\n")


def test_dist_without_input():
    assert run("dist", "-L", "x.shuf") == (1, "", "metakssd: please specify the input/query files\n")


def test_dist_wrong_input_format(tmp_path):
    (tmp_path / "notes.txt").write_text("no sequences\n")
    assert run("dist", "-L", "x.shuf", "notes.txt", cwd=str(tmp_path)) == (
        1, "", "metakssd: wrong format 1th argument: notes.txt (supported: .fna .fas .fasta .fq .fastq .fa, optionally .gz/.bz2)\n")


def test_dist_r_on_a_missing_path():
    assert run("dist", "-r", "/no/such/path", "q") == (1, "", "metakssd: test_get_fullpath()::/no/such/path: No such file or directory\n")


def test_dist_stage2_on_a_truncated_cofiles_stat(truncated, tmp_path):
    out = tmp_path / "out"
    assert run("dist", truncated, "-o", out) == (1, "", "metakssd: run_stageII(():%s/cofiles.stat\n" % truncated)
    assert not out.exists()


# the keys of the --timing line, in the order of its format string: bench.py and the tools read them by name
TIMING_KEYS = [
    "t0_abs", "exit_abs", "shuf_read", "hip_ready", "engine_ready", "first_push", "last_push", "unmapped", "written", "finish_s", "begin_s",
    "rows", "threads", "chunks", "chunks_discarded", "serial_rows", "stream_setup_s", "stream_wait_frame_s", "stream_push_s", "stream_total_s",
    "push_call_s", "wait_call_s", "push_call_max_s", "first_push_call_s", "gpus", "gather_ms", "tail_ms", "transport",
    "batches", "batch_wait_readers_s", "batch_pin_s", "batch_begin_s", "readers_read_cpu_s", "readers_pack_cpu_s", "readers_blocked_s",
    "pin_calls", "pin_s", "pinned_mib", "pool_mib"]


def timing_lines(stdout):
    out = []
    for line in stdout.splitlines():
        if line.startswith("{"):
            d = json.loads(line)
            if "timing" in d:
                out.append(d)
    return out


def read_dir(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_timing_keys_and_the_batch_path_against_the_serial_path(tmp_path, shufs):
    sp = str(tmp_path / "L0K6.shuf")
    shufs("L0K6").write(sp)
    rs = np.random.RandomState(48)
    fq = str(tmp_path / "four.fq")
    open(fq, "wb").write(ui.fastq_bytes([ui.rand_seq(rs, 150) for _ in range(4)]))
    rc, out, err = run("dist", "-L", sp, "-A", "--quiet", "--timing", "-o", tmp_path / "fq_out", fq)
    assert rc == 0, err
    tl = timing_lines(out)
    assert len(tl) == 1 and list(tl[0]) == ["timing"] and list(tl[0]["timing"]) == TIMING_KEYS
    assert tl[0]["timing"]["rows"] == 4 and tl[0]["timing"]["batches"] == 0

    # three tiny genomes: two contigs of 40 bases each, one file with a run of N -- a batch of three
    gd = tmp_path / "genomes"
    gd.mkdir()
    names = ["a.fa", "b.fna", "c.fasta"]
    for i, n in enumerate(names):
        contigs = [ui.rand_seq(rs, 40), ui.rand_seq(rs, 40)]
        if i == 1:
            contigs[0] = contigs[0][:14] + b"N" * 9 + contigs[0][23:]
        (gd / n).write_bytes(ui.fasta_bytes(contigs))
    dirs = {}
    for tag, extra, env in (("batch", [], {}), ("serial", ["--no-batch"], {}), ("tiny", [], {"MK_BATCH_TAB_BITS": "9"})):
        d = str(tmp_path / tag)
        rc, out, err = run("dist", "-L", sp, "--quiet", "--timing", "-o", d, gd, *extra, env=dict(os.environ, **env))
        assert rc == 0, err
        tl = timing_lines(out)
        assert len(tl) == 1 and list(tl[0]["timing"]) == TIMING_KEYS
        assert tl[0]["timing"]["batches"] == (0 if tag == "serial" else 1)
        dirs[tag] = read_dir(d)
    got = dirs["batch"]
    assert dirs["serial"] == got and dirs["tiny"] == got
    st = got["cofiles.stat"]
    comp_num, infile_num = struct.unpack_from("<ii", st, 16)
    assert infile_num == 3 and len(st) == 32 + 3 * (4 + PATHLEN)
    listed = [st[32 + 4 * 3 + PATHLEN * i:][:PATHLEN].split(b"\0")[0].decode() for i in range(3)]
    assert listed == [os.path.join(str(gd), n) for n in sorted(names)]
    cts = struct.unpack_from("<3I", st, 32)
    idx = struct.unpack("<4Q", got["combco.index.0"])
    assert idx[0] == 0 and all(a < b for a, b in zip(idx, idx[1:])) and idx[3] * 4 == len(got["combco.0"])
    if comp_num == 1:
        assert tuple(b - a for a, b in zip(idx, idx[1:])) == cts
