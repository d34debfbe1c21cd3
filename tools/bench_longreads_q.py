#!/usr/bin/env python3
"""tools/bench_longreads_q.py -- `dist -n 2 -Q 53 --long-reads-q / --long-inflate-q` on reads of 10 000 bases against
the only way the parent commit sketches these reads: its default route (host framer; `zcat` child for a .gz).

The input is seeded: --reads reads (50 000 by default) of --read-len bases cut from both strands of a random sequence of a tenth of
that size, L3K11; quality lines of 'I' with about one byte in a hundred below Q = 53, from a seeded generator.  Both files (plain,
gzip level 6) are read once into the page cache; then the legs take turns, --runs times:
  plain/parent   --parent-cli: dist -n 2 -Q 53 on the plain file
  plain/this     this build: the same with --long-reads-q
  gzip6/parent   --parent-cli on the .gz (zcat)
  gzip6/this     this build with --long-inflate-q (a gzip status sends the file to zcat, as the switch promises: the source and the
                 "fallback" of every run are recorded)
  bgzf/...       with --bgzf: the same pair on the text as a BGZF chain
The plain and the BGZF leg must report their source in every run.  When the gzip leg left the device route, one control run each:
the parent's `dist -A --long-inflate` on the same file (the same decode without this route) and this route at three other span sizes.
Wall time is from process start to its exit, the directory on disk.  The directories are compared byte for byte (combco.*) in every
run BEFORE a time is kept; a difference ends the run with an error.  Reported: the median, the least and the largest of the runs
of each leg, their ratio, and whether it lies outside the spread of both.  With --rocprof DIR one more run of `--long-reads-q` and
one of `dist -A --long-reads` on the same text under `rocprofv3 --kernel-trace --stats`, each in a run of its own: the time of the
mk_fqq_* kernels per text byte beside that of mk_fql_summary / _scan / _emit.  Prints one JSON line; --out writes it to a file as
well."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_longreads as bl  # noqa: E402

CLI = bl.CLI
SEED, Q, M = 20261021, 53, 2


def write_inputs(tmp, nreads, read_len):
    """-> (FASTQ, its gzip -6, bases, share of quality bytes below Q)"""
    rs = np.random.RandomState(SEED)
    genome = np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, size=max(nreads * read_len // 10, 4 * read_len))]
    starts = rs.randint(0, len(genome) - read_len, size=nreads)
    flip = rs.rand(nreads) < 0.5
    quals, low = [], 0
    for _ in range(256):  # 256 quality lines, taken in turn
        q = np.full(read_len, ord("I"), np.uint8)
        at = rs.rand(read_len) < 0.01
        q[at] = rs.choice(np.array([Q - 1, 33, 40], np.uint8), size=int(at.sum()))
        quals.append(q.tobytes())
        low += int(at.sum())
    fq = os.path.join(tmp, "long_q.fq")
    with open(fq, "wb") as f:
        for i in range(nreads):
            s = genome[starts[i]:starts[i] + read_len]
            s = (bl._COMP[s][::-1] if flip[i] else s).tobytes()
            f.write(b"@read%d length=%d\n%s\n+\n%s\n" % (i, read_len, s, quals[i % 256]))
    gz = fq + ".gz"
    with open(gz, "wb") as out:
        subprocess.run(["gzip", "-6", "-n", "-c", fq], stdout=out, check=True)
    return fq, gz, nreads * read_len, low / (256.0 * read_len)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-cli", required=True, help="metakssd of the parent commit: the legs this route is measured against")
    ap.add_argument("--rocprof", default=None, help="directory: one more run of --long-reads-q and one of dist -A --long-reads under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--bgzf", action="store_true", help="one more pair of legs: the same text as a BGZF chain")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from golden_cases import make_shuf
    tmp = tempfile.mkdtemp(prefix="bench_longreads_q_", dir=a.tmp)
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        t0 = time.perf_counter()
        fq, gz, bases, low_share = write_inputs(tmp, a.reads, a.read_len)
        write_s = time.perf_counter() - t0
        files = {"plain": fq, "gzip6": gz}
        if a.bgzf:  # the same text as a BGZF chain (members of 65 280 text bytes, level 6, tests/bgzf_util.py's writer)
            import bgzf_util as bu
            files["bgzf"] = os.path.join(tmp, "long_q_bgzf.fq.gz")
            with open(fq, "rb") as src, open(files["bgzf"], "wb") as dst:
                while True:
                    piece = src.read(65280)
                    if not piece:
                        break
                    dst.write(bu.member(piece, 6))
                dst.write(bu.EOF_MARKER)
        for p in files.values():  # into the page cache
            with open(p, "rb") as f:
                while f.read(64 << 20):
                    pass
        occ = ["-n", str(M), "-Q", str(Q)]
        switch = {"plain": "--long-reads-q", "gzip6": "--long-inflate-q", "bgzf": "--long-inflate-q"}
        want_source = {"plain": "file", "gzip6": "device-gunzip", "bgzf": "device-inflate"}
        legs = {}
        for k, p in files.items():
            legs[k + "/parent"] = [a.parent_cli, "dist", "-L", shuf] + occ + ["--quiet", "--timing", "-o", os.path.join(tmp, "out_parent_" + k), p]
            legs[k + "/this"] = [CLI, "dist", "-L", shuf] + occ + [switch[k], "--quiet", "--timing", "-o", os.path.join(tmp, "out_this_" + k), p]
        walls, infos, want = {k: [] for k in legs}, {}, None
        sources = {k: [] for k in legs}
        for r in range(a.runs):
            for k, cmd in legs.items():  # taking turns: a drift of the machine hits all legs alike
                shutil.rmtree(cmd[-2], ignore_errors=True)
                dt, infos[k] = bl.run(cmd)
                got = bl.combco(cmd[-2])
                want = want or got
                if not got or got != want:  # before a time is kept
                    raise RuntimeError("run %d, leg %s: its directory differs from the first leg's" % (r, k))
                if k.endswith("/this"):
                    # the plain and the BGZF leg must take their source in every run.  A gzip stream may leave the device route with a
                    # status of the shared decode (a false block-start candidate) and is then read through zcat, as the
                    # switch promises: that leg's times are kept, with "device_route_in_every_run": false and the controls below
                    name = k.split("/")[0]
                    took = infos[k].get("source") == want_source[name] and "fallback" not in infos[k]
                    if infos[k].get("route") != "long-reads-q" or (name != "gzip6" and not took):
                        raise RuntimeError("run %d, leg %s: the route was not taken (%s)" % (r, k, infos[k]))
                    sources[k].append([infos[k].get("source"), infos[k].get("fallback")])
                walls[k].append(dt)
            print("run %d: %s" % (r, {k: round(v[-1], 3) for k, v in walls.items()}), file=sys.stderr, flush=True)
        keys = sum(len(v) for n, v in want.items() if ".index." not in n) // 4
        res = {"bench": "longreads_q", "what": "wall seconds from process start to exit (directory on disk): dist -n %d -Q %d of the parent commit (host framer; zcat "
               "child for the .gz) against --long-reads-q / --long-inflate-q of this build on the same file, reads of %d bases, L3K11, median of %d runs, the legs "
               "taking turns, files in the page cache" % (M, Q, a.read_len, a.runs),
               "reads": a.reads, "bases": bases, "read_len": a.read_len, "runs": a.runs, "keys": keys, "quality_bytes_below_Q": round(low_share, 5),
               "directories_equal": True, "writing_the_files_s": round(write_s, 1), "file_bytes": {k: os.path.getsize(p) for k, p in files.items()}, "inputs": {}}
        for k in files:
            p, t = bl.spread(walls[k + "/parent"]), bl.spread(walls[k + "/this"])
            route = {f: v for f, v in infos[k + "/this"].items() if f not in ("input", "timing")}
            res["inputs"][k] = {"parent": p, "this": t, "gbases_s": {"parent": round(bases / p["wall_s"] / 1e9, 3), "this": round(bases / t["wall_s"] / 1e9, 3)},
                                "ratio_parent_over_this": round(p["wall_s"] / t["wall_s"], 3),
                                "outside_the_spread": t["wall_min_s"] > p["wall_max_s"] or t["wall_max_s"] < p["wall_min_s"], "route_line_of_the_last_run": route,
                                "source_wanted": want_source[k], "source_and_fallback_of_every_run": sources[k + "/this"],
                                "device_route_in_every_run": all(x == [want_source[k], None] for x in sources[k + "/this"])}
        if not res["inputs"]["gzip6"]["device_route_in_every_run"]:
            # controls, one run each: the parent's dist -A --long-inflate on the same file (the same decode, none of this route), and this
            # route with other spans (a candidate is the first valid header of a span, so the spans decide which candidates are taken)
            ctl = {}
            cmds = {"parent -A --long-inflate": [a.parent_cli, "dist", "-L", shuf, "-A", "--long-inflate", "--quiet", "--timing", "-o", os.path.join(tmp, "out_ctl"), gz]}
            for kib in (32, 512, 2048):
                cmds["this --long-inflate-q --gunzip-span-bytes %d" % (kib << 10)] = legs["gzip6/this"][:-3] + ["--gunzip-span-bytes", str(kib << 10)] + legs["gzip6/this"][-3:]
            for name, cmd in cmds.items():
                shutil.rmtree(cmd[-2], ignore_errors=True)
                dt, info = bl.run(cmd)
                if "long-inflate-q" in name and bl.combco(cmd[-2]) != want:
                    raise RuntimeError("control %s: its directory differs" % name)
                ctl[name] = {"wall_s": round(dt, 4), "source": info.get("source"), "fallback": info.get("fallback")}
            res["gzip6_controls"] = ctl
        if a.rocprof:
            os.makedirs(a.rocprof, exist_ok=True)
            nbytes = os.path.getsize(fq)
            prof = {}
            runs = (("longreads_q", legs["plain/this"], ("mk_fqq_summary_kernel", "mk_fqq_scan_kernel", "mk_fqq_emit_kernel", "mk_fqq_first_kernel")),
                    ("longreads_A", [CLI, "dist", "-L", shuf, "-A", "--long-reads", "--quiet", "--timing", "-o", os.path.join(tmp, "out_A"), fq],
                     ("mk_fql_summary_kernel", "mk_fql_scan_kernel", "mk_fql_emit_kernel")))
            for name, cmd, kernels in runs:  # (each under the profiler in a run of its own)
                shutil.rmtree(cmd[-2], ignore_errors=True)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", name, "--"] + cmd + ["--slow-exit"],
                               stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1700, check=True)
                tot = bl.kernel_totals(a.rocprof, name)
                mine = {k: v for k, v in tot.items() if k in kernels}
                prof[name] = {"text_bytes": nbytes, "kernels_ms": {k: v[0] for k, v in sorted(tot.items())}, "calls": {k: v[1] for k, v in sorted(mine.items())},
                              "framing_kernels_ms": round(sum(v[0] for v in mine.values()), 3),
                              "framing_kernels_ps_per_text_byte": round(sum(v[0] for v in mine.values()) * 1e9 / nbytes, 3)}
            q, p = prof["longreads_q"], prof["longreads_A"]
            prof["ratio_q_over_A"] = round(q["framing_kernels_ms"] / p["framing_kernels_ms"], 3) if p["framing_kernels_ms"] else None
            prof["q_emit_over_A_summary_plus_emit"] = round(q["kernels_ms"].get("mk_fqq_emit_kernel", 0.0) /
                                                            max(p["kernels_ms"].get("mk_fql_summary_kernel", 0.0) + p["kernels_ms"].get("mk_fql_emit_kernel", 0.0), 1e-9), 3)
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
