#!/usr/bin/env python3
"""tools/bench_longreads.py -- `dist -A --long-reads` on reads of 10 000 bases against the only way the parent commit
can sketch the same bases: the file chopped into pieces of at most 4 094 characters (every TL-window in exactly one piece,
tests/longreads_cases.py) through its default -A route.

The input is seeded: --gbases Gbases (2 by default) of reads of --read-len bases cut from both strands of a random sequence of a
tenth of that size (ten-fold coverage: counts above 1), L3K11.  Both files are read once into the page cache; then the legs take
turns, --runs times:
  long_reads   this build: dist -A --long-reads on the file as it is
  chopped      --parent-cli <metakssd of the parent commit> (this build's when not given): dist -A on the chopped file
Wall time is from process start to its exit, the directory on disk.  The two directories are compared byte for byte (combco.*) BEFORE
a time is kept; a difference ends the run with an error.  Reported: the median, the least and the largest of the runs of each leg,
their ratio, and whether it lies outside the spread of both.  With --rocprof DIR one more run of the long route and one of
`dist` on a FASTA file of the same bases (mk_sketch_push_stream) under `rocprofv3 --kernel-trace --stats`: the time of the
three mk_fql_* kernels per text byte beside that of mk_fa_*.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
SEED, FQ_MAX = 20261020, 4094
_COMP = np.zeros(256, np.uint8)
_COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


def write_inputs(tmp, gbases, read_len, TL, with_fasta):
    """-> (long FASTQ, chopped FASTQ, FASTA of the same bases (with_fasta), reads, bases)"""
    rs = np.random.RandomState(SEED)
    nreads = int(gbases * 1e9) // read_len
    genome = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=max(nreads * read_len // 10, 4 * read_len))]
    starts = rs.randint(0, len(genome) - read_len, size=nreads)
    flip = rs.rand(nreads) < 0.5
    step = FQ_MAX - (TL - 1)
    cuts, at = [], 0  # tests/longreads_cases.py's chop()
    while True:
        cuts.append((at, min(at + FQ_MAX, read_len)))
        if at + FQ_MAX >= read_len:
            break
        at += step
    qual = b"I" * read_len
    paths = [os.path.join(tmp, n) for n in ("long.fq", "chopped.fq", "same.fa")]
    with open(paths[0], "wb") as fl, open(paths[1], "wb") as fc, open(paths[2], "wb") as fa:
        for i in range(nreads):
            s = genome[starts[i]:starts[i] + read_len]
            s = (_COMP[s][::-1] if flip[i] else s).tobytes()
            fl.write(b"@read%d length=%d\n%s\n+\n%s\n" % (i, read_len, s, qual))
            for j, (a, b) in enumerate(cuts):
                fc.write(b"@read%d/%d\n%s\n+\n%s\n" % (i, j, s[a:b], qual[:b - a]))
            if with_fasta:
                fa.write(b">read%d\n%s\n" % (i, s))
    return paths[0], paths[1], paths[2], nreads, nreads * read_len


def run(cmd):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1700)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (cmd[:8], r.stderr.decode(errors="replace")[-500:]))
    info = {}
    for ln in r.stdout.split(b"\n"):
        if ln.startswith(b'{"timing"') or ln.startswith(b'{"input"'):
            info.update(json.loads(ln))
    return dt, info


def combco(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d)) if n.startswith("combco")}


def kernel_totals(directory, name):
    """{kernel: (total ms, calls)} from the kernel_stats CSV rocprofv3 wrote for -o `name`"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", name + "_kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            m = re.search(r"\bmk_[a-z0-9_]+", row.get("Name", ""))
            if m:
                t, c = out.get(m.group(0), (0.0, 0))
                out[m.group(0)] = (round(t + float(row["TotalDurationNs"]) / 1e6, 3), c + int(row["Calls"]))
    return out


def write_compressed(tmp, fq):
    """the long FASTQ three ways, written side by side: one gzip member at level 1, one at level 6, BGZF (`bgzip` where the machine
    has it, else members of 65 280 text bytes by tests/bgzf_util.py's writer) -> {name: path}, {name: how it was written}"""
    import bgzf_util as bu
    paths = {"gzip1": os.path.join(tmp, "long_l1.fq.gz"), "gzip6": os.path.join(tmp, "long_l6.fq.gz"), "bgzf": os.path.join(tmp, "long_bgzf.fq.gz")}
    how = {"gzip1": "gzip -1", "gzip6": "gzip -6"}
    procs = [subprocess.Popen(["gzip", "-%d" % lv, "-n", "-c", fq], stdout=open(paths[k], "wb")) for k, lv in (("gzip1", 1), ("gzip6", 6))]
    if shutil.which("bgzip"):
        how["bgzf"] = "bgzip"
        procs.append(subprocess.Popen(["bgzip", "-c", fq], stdout=open(paths["bgzf"], "wb")))
    else:
        how["bgzf"] = "tests/bgzf_util.py member(), 65 280 text bytes a member, level 6"
        with open(fq, "rb") as src, open(paths["bgzf"], "wb") as dst:
            while True:
                piece = src.read(65280)
                if not piece:
                    break
                dst.write(bu.member(piece, 6))
            dst.write(bu.EOF_MARKER)
    for p in procs:
        if p.wait() != 0:
            raise RuntimeError("writing a compressed input failed")
    return paths, how


def spread(walls):
    return {"wall_s": round(statistics.median(walls), 4), "wall_min_s": round(min(walls), 4), "wall_max_s": round(max(walls), 4), "wall_runs": [round(v, 4) for v in walls]}


def main_gz(a):
    """--gz: the long FASTQ compressed three ways; per file the parent's `dist -A --long-reads` (its zcat child) against
    this build's `dist -A --long-inflate`, and the plain file through `--long-reads` of both builds (the carry moved to the device)."""
    from golden_cases import make_shuf
    if not a.parent_cli:
        raise SystemExit("--gz needs --parent-cli: the legs it is measured against are the parent commit's")
    tmp = tempfile.mkdtemp(prefix="bench_longreads_gz_", dir=a.tmp)
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        t0 = time.perf_counter()
        fq, chopped, fa, nreads, bases = write_inputs(tmp, a.gbases, a.read_len, 22, False)
        os.remove(chopped)
        os.remove(fa)
        files, how = write_compressed(tmp, fq)
        files["plain"] = fq
        write_s = time.perf_counter() - t0
        for p in files.values():  # into the page cache
            with open(p, "rb") as f:
                while f.read(64 << 20):
                    pass
        want_source = {"gzip1": "device-gunzip", "gzip6": "device-gunzip", "bgzf": "device-inflate", "plain": "file"}
        legs = {}
        for k, p in files.items():
            legs[k + "/parent"] = [a.parent_cli, "dist", "-L", shuf, "-A", "--long-reads", "--quiet", "--timing", "-o", os.path.join(tmp, "out_parent_" + k), p]
            legs[k + "/this"] = [CLI, "dist", "-L", shuf, "-A", "--long-reads" if k == "plain" else "--long-inflate", "--quiet", "--timing", "-o",
                                 os.path.join(tmp, "out_this_" + k), p]
        walls, infos, want = {k: [] for k in legs}, {}, None
        for r in range(a.runs):
            for k, cmd in legs.items():  # taking turns: a drift of the machine hits all legs alike
                shutil.rmtree(cmd[-2], ignore_errors=True)
                dt, infos[k] = run(cmd)
                got = combco(cmd[-2])
                want = want or got
                if not got or got != want:  # before a time is kept
                    raise RuntimeError("run %d, leg %s: its directory differs from the first leg's" % (r, k))
                if k.endswith("/this") and (infos[k].get("source") != want_source[k.split("/")[0]] or "fallback" in infos[k]):
                    raise RuntimeError("run %d, leg %s: the route was not taken (%s)" % (r, k, infos[k]))
                walls[k].append(dt)
            print("run %d: %s" % (r, {k: round(v[-1], 3) for k, v in walls.items()}), file=sys.stderr, flush=True)
        keys = sum(len(v) for n, v in want.items() if not n.endswith(".a") and ".index." not in n) // 4
        res = {"bench": "longreads_gz", "what": "wall seconds from process start to exit (directory on disk): dist -A --long-reads of the parent commit (zcat child for a "
               ".gz) against dist -A --long-inflate of this build on the same file, reads of %d bases, L3K11, median of %d runs, the legs taking turns, files in the "
               "page cache; plain: dist -A --long-reads of both builds on the uncompressed file" % (a.read_len, a.runs),
               "reads": nreads, "bases": bases, "read_len": a.read_len, "runs": a.runs, "keys": keys, "directories_equal": True, "writing_the_files_s": round(write_s, 1),
               "written_by": how, "file_bytes": {k: os.path.getsize(p) for k, p in files.items()}, "inputs": {}}
        for k in files:
            p, t = spread(walls[k + "/parent"]), spread(walls[k + "/this"])
            route = {f: v for f, v in infos[k + "/this"].items() if f not in ("input", "timing")}
            res["inputs"][k] = {"parent": p, "this": t, "gbases_s": {"parent": round(bases / p["wall_s"] / 1e9, 3), "this": round(bases / t["wall_s"] / 1e9, 3)},
                                "ratio_parent_over_this": round(p["wall_s"] / t["wall_s"], 3),
                                "outside_the_spread": t["wall_min_s"] > p["wall_max_s"] or t["wall_max_s"] < p["wall_min_s"], "route_line_of_the_last_run": route}
        if a.rocprof:
            os.makedirs(a.rocprof, exist_ok=True)
            res["rocprof"] = {}
            for k in ("gzip6", "bgzf"):
                cmd = legs[k + "/this"]
                shutil.rmtree(cmd[-2], ignore_errors=True)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", "longinflate_" + k, "--"] + cmd + ["--slow-exit"],
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1700, check=True)
                tot = kernel_totals(a.rocprof, "longinflate_" + k)
                res["rocprof"][k] = {"kernels_ms": {n: v[0] for n, v in sorted(tot.items())}, "calls": {n: v[1] for n, v in sorted(tot.items())}}
        line = json.dumps(res)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbases", type=float, default=2.0)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-cli", default=None, help="metakssd of the parent commit for the chopped leg (this build's when not given)")
    ap.add_argument("--rocprof", default=None, help="directory: one more run of the long route and one of the FASTA stream under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gz", action="store_true", help="the compressed inputs of dist -A --long-inflate (DESIGN.md 4.20) against --parent-cli's --long-reads")
    a = ap.parse_args()
    if a.gz:
        return main_gz(a)
    from golden_cases import make_shuf
    tmp = tempfile.mkdtemp(prefix="bench_longreads_", dir=a.tmp)
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        fq, chopped, fa, nreads, bases = write_inputs(tmp, a.gbases, a.read_len, 22, bool(a.rocprof))
        for p in (fq, chopped):  # into the page cache
            with open(p, "rb") as f:
                while f.read(64 << 20):
                    pass
        chop_cli = a.parent_cli or CLI
        legs = {"long_reads": [CLI, "dist", "-L", shuf, "-A", "--long-reads", "--quiet", "--timing", "-o", os.path.join(tmp, "out_long"), fq],
                "chopped": [chop_cli, "dist", "-L", shuf, "-A", "--quiet", "--timing", "-o", os.path.join(tmp, "out_chopped"), chopped]}
        walls, infos = {k: [] for k in legs}, {}
        for r in range(a.runs):
            for k, cmd in legs.items():  # taking turns: a drift of the machine hits both legs alike
                shutil.rmtree(cmd[-2], ignore_errors=True)
                dt, infos[k] = run(cmd)
                walls[k].append(dt)
            x, y = combco(legs["long_reads"][-2]), combco(legs["chopped"][-2])
            if not x or x != y:  # before a time is kept
                raise RuntimeError("run %d: the directories of the two legs differ (%s)" % (r, [n for n in x if x[n] != y.get(n)][:4]))
            print("run %d: %s" % (r, {k: round(v[-1], 3) for k, v in walls.items()}), file=sys.stderr, flush=True)
        keys = sum(len(v) for n, v in x.items() if not n.endswith(".a") and ".index." not in n) // 4
        res = {"bench": "longreads", "what": "wall seconds from process start to exit (directory on disk), dist -A --long-reads on reads of %d bases against "
               "dist -A of %s on the same reads chopped into pieces of at most 4 094 characters, L3K11, median of %d runs, the legs taking turns, files in "
               "the page cache" % (a.read_len, "the parent commit" if a.parent_cli else "this build", a.runs),
               "reads": nreads, "bases": bases, "read_len": a.read_len, "runs": a.runs, "keys": keys, "directories_equal": True,
               "text_bytes": {"long_reads": os.path.getsize(fq), "chopped": os.path.getsize(chopped)}, "chopped_leg_cli": "parent" if a.parent_cli else "this build"}
        for k in legs:
            t = infos[k].get("timing", {})
            res[k] = {"wall_s": round(statistics.median(walls[k]), 4), "wall_min_s": round(min(walls[k]), 4), "wall_max_s": round(max(walls[k]), 4),
                      "wall_runs": [round(v, 4) for v in walls[k]], "gbases_s": round(bases / statistics.median(walls[k]) / 1e9, 3),
                      "first_push": t.get("first_push"), "last_push": t.get("last_push"), "route": infos[k].get("route")}
        res["ratio_long_over_chopped"] = round(res["long_reads"]["wall_s"] / res["chopped"]["wall_s"], 3)
        res["outside_the_spread"] = res["long_reads"]["wall_min_s"] > res["chopped"]["wall_max_s"] or res["long_reads"]["wall_max_s"] < res["chopped"]["wall_min_s"]
        if a.rocprof:
            os.makedirs(a.rocprof, exist_ok=True)
            prof = {}
            for name, cmd, nbytes in (("longreads_fq", legs["long_reads"], os.path.getsize(fq)),
                                      ("longreads_fa", [CLI, "dist", "-L", shuf, "--quiet", "--timing", "-o", os.path.join(tmp, "out_fa"), fa], os.path.getsize(fa))):
                shutil.rmtree(cmd[-2], ignore_errors=True)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", name, "--"] + cmd + ["--slow-exit"],
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1700, check=True)
                tot = kernel_totals(a.rocprof, name)
                pre = "mk_fql_" if name.endswith("fq") else "mk_fa_"
                three = {k: v for k, v in tot.items() if k in (pre + "summary_kernel", pre + "scan_kernel", pre + "emit_kernel")}
                prof[name] = {"text_bytes": nbytes, "kernels_ms": {k: v[0] for k, v in sorted(tot.items())}, "calls": {k: v[1] for k, v in sorted(three.items())},
                              "three_kernels_ms": round(sum(v[0] for v in three.values()), 3),
                              "three_kernels_ps_per_text_byte": round(sum(v[0] for v in three.values()) * 1e9 / nbytes, 3)}
            res["rocprof"] = prof
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
