#!/usr/bin/env python3
"""tools/bench_gunzip_repair.py -- `--gunzip-repair` on the file DESIGN.md 4.21 says falls off the device route: the
seeded 50 000 x 10 000-base long-read FASTQ of tools/bench_longreads_q.py, `gzip -6`, 172 MB.  The parent commit and this build
without the switch return MK_INFL_MISSED on it and read it through `zcat`; with the switch a false piece start is repaired.

Legs, --runs times, taking turns, wall from process start to exit, files in the page cache:
  q/parent      --parent-cli: dist -n 2 -Q 53 --long-inflate-q            (expected: zcat, the fallback recorded)
  q/this        this build, the same line                                  (expected: the same)
  q/repair      this build with --gunzip-repair
  A/parent      --parent-cli: dist -A --long-inflate
  A/repair      this build: dist -A --long-inflate --gunzip-repair
  clean/plain   this build: dist -A --long-inflate on DESIGN.md 4.20's file (qualities all 'I', gzip -6): a file without a false start
  clean/repair  ... with --gunzip-repair: what the switch costs where there is nothing to repair
Per run the --timing source, fallback, repairs, pieces and decode / find ms are kept.  The directories of a group (q, A, clean) are
compared byte for byte (combco.*) in every run BEFORE a time is kept.  Nothing is asserted about the route: a leg that left the device
route says so in its record (status text, piece count), which is the finding.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_longreads as bl  # noqa: E402
import bench_longreads_q as blq  # noqa: E402

CLI = bl.CLI
KEEP = ("route", "source", "fallback", "repairs", "pieces", "batches", "find_ms", "decode_ms", "resolve_ms", "text_bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--clean-gbases", type=float, default=0.5, help="size of the file without a false start (0: no clean legs)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-cli", required=True, help="metakssd of the parent commit")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from golden_cases import make_shuf
    tmp = tempfile.mkdtemp(prefix="bench_gunzip_repair_", dir=a.tmp)
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        t0 = time.perf_counter()
        fq, gz, bases, _ = blq.write_inputs(tmp, a.reads, a.read_len)
        os.remove(fq)
        files = {"q": gz}
        if a.clean_gbases:
            long_fq, chopped, fa, _, clean_bases = bl.write_inputs(tmp, a.clean_gbases, a.read_len, 22, False)
            clean = long_fq + ".gz"
            with open(clean, "wb") as out:
                subprocess.run(["gzip", "-6", "-n", "-c", long_fq], stdout=out, check=True)
            for p in (long_fq, chopped, fa):
                os.remove(p)
            files["clean"] = clean
        write_s = time.perf_counter() - t0
        for p in files.values():  # into the page cache
            with open(p, "rb") as f:
                while f.read(64 << 20):
                    pass
        occ = ["-n", str(blq.M), "-Q", str(blq.Q), "--long-inflate-q"]
        A = ["-A", "--long-inflate"]

        def leg(cli, flags, name, path):
            return [cli, "dist", "-L", shuf] + flags + ["--quiet", "--timing", "-o", os.path.join(tmp, "out_" + name.replace("/", "_")), path]
        legs = {"q/parent": leg(a.parent_cli, occ, "q/parent", gz), "q/this": leg(CLI, occ, "q/this", gz), "q/repair": leg(CLI, occ + ["--gunzip-repair"], "q/repair", gz),
                "A/parent": leg(a.parent_cli, A, "A/parent", gz), "A/repair": leg(CLI, A + ["--gunzip-repair"], "A/repair", gz)}
        if a.clean_gbases:
            legs["clean/plain"] = leg(CLI, A, "clean/plain", files["clean"])
            legs["clean/repair"] = leg(CLI, A + ["--gunzip-repair"], "clean/repair", files["clean"])
        walls, lines, want = {k: [] for k in legs}, {k: [] for k in legs}, {}
        for r in range(a.runs):
            for k, cmd in legs.items():  # taking turns: a drift of the machine hits all legs alike
                shutil.rmtree(cmd[-2], ignore_errors=True)
                dt, info = bl.run(cmd)
                got = bl.combco(cmd[-2])
                group = k.split("/")[0]
                want.setdefault(group, got)
                if not got or got != want[group]:  # before a time is kept
                    raise RuntimeError("run %d, leg %s: its directory differs from the first leg's of its group" % (r, k))
                walls[k].append(dt)
                lines[k].append({f: info.get(f) for f in KEEP if f in info})
            print("run %d: %s" % (r, {k: round(v[-1], 3) for k, v in walls.items()}), file=sys.stderr, flush=True)
        res = {"bench": "gunzip_repair", "what": "wall seconds from process start to exit (directory on disk), L3K11, %d runs a leg, the legs taking turns, files in "
               "the page cache; q: dist -n %d -Q %d --long-inflate-q, A and clean: dist -A --long-inflate; parent = the parent commit's command line" % (a.runs, blq.M, blq.Q),
               "reads": a.reads, "read_len": a.read_len, "bases": bases, "runs": a.runs, "directories_equal_within_each_group": True,
               "writing_the_files_s": round(write_s, 1), "file_bytes": {k: os.path.getsize(p) for k, p in files.items()}, "legs": {}}
        for k in legs:
            res["legs"][k] = dict(bl.spread(walls[k]), runs=lines[k],
                                  device_route_in_every_run=all(x.get("source") == "device-gunzip" and not x.get("fallback") for x in lines[k]))

        def apart(x, y):
            return res["legs"][x]["wall_min_s"] > res["legs"][y]["wall_max_s"] or res["legs"][x]["wall_max_s"] < res["legs"][y]["wall_min_s"]
        pairs = [("q/parent", "q/repair"), ("q/this", "q/repair"), ("A/parent", "A/repair")] + ([("clean/plain", "clean/repair")] if a.clean_gbases else [])
        res["compared"] = {"%s over %s" % (x, y): {"ratio_of_medians": round(res["legs"][x]["wall_s"] / res["legs"][y]["wall_s"], 3), "ranges_do_not_overlap": apart(x, y)}
                           for x, y in pairs}
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
