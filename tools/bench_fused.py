#!/usr/bin/env python3
"""tools/bench_fused.py -- reads to species report: `dist -A -o <dir>` + `composite -r <markerdb> -q <dir>` (two processes, the sketch
through the file system) against `dist -A --composite <markerdb>` (one process, the sketch stays on the device).

The marker database is tools/bench_composite.py's (every id private to one sketch), carrying the .shuf file's id; the samples are
stretches of bench.py's read stream (mk_synth_fastq_write_mt, same seed and read length), sketched at L3K11.  For every cell of
--reads x --samples three legs take turns, --runs times, the files in the page cache (every leg reads them once before the first turn):
  two_step   this build: both commands, wall = the two processes from start to exit, added
  parent     --parent-cli <metakssd of the parent commit>: the same two commands
  fused      this build's one command
The report of every leg of every run is compared byte for byte (the --timing lines apart) BEFORE any time is reported: a difference
ends the run with an error.  Beside the walls: the kernel times of the two --timing lines (the sketch's finish, the database load and
the query kernels).  Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_composite as bc  # noqa: E402

CLI = bc.CLI
SEED, READ_LEN = 20261002, 150  # bench.py's SEED and READ_LEN


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1700)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (cmd[:8], r.stderr.decode(errors="replace")[-500:]))
    lines = r.stdout.split(b"\n")
    info = {}
    for ln in lines:
        if ln.startswith(b"{"):
            info.update(json.loads(ln))
    return dt, b"\n".join(ln for ln in lines if not ln.startswith(b"{")), info


def two_step(cli, shuf, db, files, tmp):
    d = os.path.join(tmp, "sk")
    shutil.rmtree(d, ignore_errors=True)
    t1, _, i1 = run([cli, "dist", "-L", shuf, "-A", "-o", d, "--quiet", "--timing"] + files)
    t2, out, i2 = run([cli, "composite", "-r", db, "-q", d, "--timing"])
    shutil.rmtree(d, ignore_errors=True)
    return t1 + t2, out, {"dist_s": t1, "composite_s": t2, "finish_s": i1["timing"]["finish_s"], **{k: i2["composite_timing"][k] for k in
                          ("route", "batches", "hits", "load_kernel_ms", "query_kernel_ms")}}


def fused(shuf, db, files):
    t, out, i = run([CLI, "dist", "-L", shuf, "-A", "--composite", db, "--timing"] + files)
    return t, out, {"finish_s": i["timing"]["finish_s"], **{k: i["composite_timing"][k] for k in
                    ("route", "batches", "hits", "load_kernel_ms", "query_kernel_ms")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=50, help="sketches of the marker database (few: a sample of random reads then shares 6+ ids with each)")
    ap.add_argument("--ids-per-sketch", type=int, default=2000000)
    ap.add_argument("--reads", default="1000000,4000000", help="reads per sample")
    ap.add_argument("--samples", default="1,4,16")
    ap.add_argument("--max-total-reads", type=int, default=0, help="skip the cells with more reads than this in all (0: none)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-cli", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from golden_cases import make_shuf
    from metakssd_amd import capi
    tmp = tempfile.mkdtemp(prefix="bench_fused_", dir=a.tmp)
    res = {"bench": "fused", "what": "wall seconds from process start to exit, `dist -A -o` + `composite -q` against `dist -A --composite`, L3K11, "
           "median of %d runs, the legs taking turns, files in the page cache" % a.runs, "ref_ids": a.sketches * a.ids_per_sketch,
           "sketches": a.sketches, "runs": a.runs, "cells": {}, "outputs_equal": True}
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        shuf_id = capi.Shuf.read(shuf).c.id
        db = os.path.join(tmp, "db")
        bc.write_db(db, a.sketches, a.ids_per_sketch)
        with open(os.path.join(db, "cofiles.stat"), "r+b") as f:  # the samples' table: no shuf-id warning in the report
            f.write(struct.pack("<i", shuf_id))
        for reads in [int(x) for x in a.reads.split(",")]:
            nmax = max(int(x) for x in a.samples.split(","))
            if a.max_total_reads:
                nmax = max([int(x) for x in a.samples.split(",") if int(x) * reads <= a.max_total_reads] or [0])
            files = []
            for i in range(nmax):
                p = os.path.join(tmp, "r%d_s%02d.fq" % (reads, i))
                assert capi.lib.mk_synth_fastq_write_mt(p.encode(), SEED, i * reads, reads, READ_LEN, 16) == 0
                files.append(p)
            for n in [int(x) for x in a.samples.split(",")]:
                if n > nmax:
                    continue
                fl = files[:n]
                for p in fl:  # into the page cache
                    with open(p, "rb") as f:
                        while f.read(64 << 20):
                            pass
                legs = {"two_step": lambda: two_step(CLI, shuf, db, fl, tmp), "fused": lambda: fused(shuf, db, fl)}
                if a.parent_cli:
                    legs["parent"] = lambda: two_step(a.parent_cli, shuf, db, fl, tmp)
                walls, infos, want, failed = {k: [] for k in legs}, {}, None, {}
                for _ in range(a.runs):
                    for k, leg in legs.items():  # taking turns: a drift of the machine hits every leg alike
                        if k in failed:
                            continue
                        try:
                            dt, out, info = leg()
                        except RuntimeError as e:
                            if k != "parent":  # the parent build may not get through a cell; this build must
                                raise
                            failed[k] = str(e).strip().splitlines()[-1][-300:]  # the command's last line on stderr
                            continue
                        if want is None:
                            want = out
                        if out != want:
                            raise RuntimeError("reads %d samples %d: the report of leg %s differs" % (reads, n, k))
                        walls[k].append(dt)
                        infos[k] = info
                    print("reads %d samples %d: %s" % (reads, n, {k: round(v[-1], 3) for k, v in walls.items() if v}), file=sys.stderr, flush=True)
                cell = {"lines": want.count(b"\n"), "outputs_equal": True}
                for k in legs:
                    if k in failed:
                        cell[k] = {"error": failed[k]}
                        continue
                    cell[k] = {"wall_s": statistics.median(walls[k]), "wall_min_s": min(walls[k]), "wall_max_s": max(walls[k]),
                               "wall_runs": [round(x, 4) for x in walls[k]], **infos[k]}
                base = "parent" if a.parent_cli and "parent" not in failed else "two_step"
                cell["saved_s_vs_" + base] = cell[base]["wall_s"] - cell["fused"]["wall_s"]
                cell["outside_the_spread"] = cell["fused"]["wall_max_s"] < cell[base]["wall_min_s"]
                res["cells"]["%dx%d" % (reads, n)] = cell
                if a.out:  # kept after every cell
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        f.write(json.dumps(res) + "\n")
            for p in files:
                os.remove(p)
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
