#!/usr/bin/env python3
"""tools/bench_gzfasta.py -- BASELINE config 5 on COMPRESSED genomes: a directory of single-member `.fna.gz` files through
`metakssd dist -L <shuf> -o out <dir>`, the device route (mk_sketch_batch_begin_gz: one wavefront inflates one file, CRC32 by
slices) against `--no-device-inflate` (one `zcat -fc` child per file on the prefetch workers), optionally against another build's
binary (--parent-cli: the parent commit's), and the plain-text directory beside them; prints one JSON line.

The genomes are bench.py's (write_genomes: same pool, same seed), compressed here with `gzip -<level>` per file.  Per geometry
(L3K10, L2K11) and level the legs run --runs times taking turns, process start to directory on disk by this process's clock;
medians are reported and the sketch directories of every leg must be byte-equal to the plain-text directory's.

--gunzip adds the route that gives every file many wavefronts (`--device-gunzip`, mk_sketch_batch_begin_gunzip): one
leg per span size of --span-bytes, beside the others in every turn; the result says pieces per genome, the best span, and that
span's ratio over the one-wavefront route, the zcat route and the parent's binary.  --json-out keeps what is known after every cell;
--rocprof then takes one more run per cell under `rocprofv3 --kernel-trace --stats` and gathers the kernels' totals in one CSV."""
import argparse
import csv
import glob
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")


def run_cli(cli, shuf, out, inp, extra):
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    r = subprocess.run([cli, "dist", "-L", shuf, "-o", out, "--quiet", "--timing"] + extra + [inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=3000)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode(errors="replace")[-500:])
    routes = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return dt, routes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1024)
    ap.add_argument("--mbases", type=float, default=4.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--levels", default="6,1")
    ap.add_argument("--geometries", default="L3K10,L2K11")
    ap.add_argument("--procs", type=int, default=16, help="gzip processes that compress the fixture")
    ap.add_argument("--parent-cli", default=None, help="another build's metakssd binary (the parent commit's), run on the same files")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--rocprof", default=None, help="directory: one more device-route run per geometry under `rocprofv3 --kernel-trace --stats`")
    ap.add_argument("--gunzip", action="store_true", help="a leg per span size with --device-gunzip (many wavefronts per file)")
    ap.add_argument("--span-bytes", default="16384,32768,65536,131072", help="the span sizes of --gunzip")
    ap.add_argument("--json-out", default=None, help="file: the result so far, rewritten after every cell")
    a = ap.parse_args()
    spans = [int(x) for x in a.span_bytes.split(",")] if a.gunzip else []
    stats_rows = []
    import bench
    from metakssd_amd import capi
    if capi.device_count() < 1:
        sys.exit("bench_gzfasta: no HIP device")
    tmp = tempfile.mkdtemp(prefix="mkgzfa_", dir=a.workdir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    out = {"what": "`metakssd dist -L <shuf> -o out <dir>` on %d genomes of %.1f Mbases as single-member .fna.gz, process start to directory on disk, "
                   "median of %d runs, legs taking turns" % (a.genomes, a.mbases, a.runs), "genomes": a.genomes, "geometries": {}}
    specs = {"L3K10": (10, 6, 3, 10), "L2K11": (11, 5, 2, 211)}
    try:
        plain = os.path.join(tmp, "plain")
        bases_each, _ = bench.write_genomes(plain, a.genomes, a.mbases)
        out["bases_per_genome"] = bases_each
        names = sorted(os.listdir(plain))
        gzdirs = {}
        for level in [int(x) for x in a.levels.split(",")]:
            d = os.path.join(tmp, "gz%d" % level)
            os.makedirs(d)
            t0 = time.perf_counter()

            def pack(n, d=d, level=level):
                with open(os.path.join(d, n + ".gz"), "wb") as g:
                    subprocess.run(["gzip", "-%d" % level, "-n", "-c", os.path.join(plain, n)], stdout=g, check=True)
            with ThreadPoolExecutor(a.procs) as ex:
                list(ex.map(pack, names))
            gzdirs[level] = (d, sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)), time.perf_counter() - t0)
        for geo in a.geometries.split(","):
            shuf = os.path.join(tmp, geo + ".shuf")
            capi.Shuf.generate(*specs[geo]).write(shuf)
            d_plain = os.path.join(tmp, "o_plain")
            tp = []
            for _ in range(3):
                bench.wait_device_quiet()
                tp.append(run_cli(CLI, shuf, d_plain, plain, [])[0])
            res = {"plain_text": {"wall_s": round(statistics.median(tp), 4), "genomes_s": round(a.genomes / statistics.median(tp), 1)}, "levels": {}}
            for level, (gd, comp, t_gz) in gzdirs.items():
                legs = {"device_route": (CLI, ["--device-inflate"]), "no_device_inflate": (CLI, ["--no-device-inflate"])}
                for S in spans:
                    legs["gunzip_%d" % S] = (CLI, ["--device-gunzip", "--gunzip-span-bytes", str(S)])
                pieces = {}
                if a.parent_cli:
                    legs["parent"] = (a.parent_cli, [])
                walls = {k: [] for k in legs}
                equal = True
                for _ in range(a.runs):
                    for k, (cli, extra) in legs.items():
                        od = os.path.join(tmp, "o_" + k)
                        bench.wait_device_quiet()
                        dt, routes = run_cli(cli, shuf, od, gd, extra)
                        if k == "device_route":
                            assert len(routes) == a.genomes and all(x["route"] == "device-inflate" for x in routes), "the device route was not taken"
                        if k.startswith("gunzip_"):
                            assert len(routes) == a.genomes and all(x["route"] == "device-gunzip" and "fallback" not in x for x in routes), "the gunzip route was not taken"
                            pieces[k] = round(sum(x["pieces"] for x in routes) / len(routes), 1)
                        walls[k].append(dt)
                        equal = equal and same_dirs_names(d_plain, od)
                med = {k: statistics.median(v) for k, v in walls.items()}
                print("bench_gzfasta: %s level %d: %s" % (geo, level, {k: round(v, 3) for k, v in med.items()}), file=sys.stderr, flush=True)
                res["levels"][str(level)] = {"comp_bytes": comp, "ratio": round(a.genomes * bases_each * 71 / 70 / comp, 3), "gzip_s": round(t_gz, 1), "sketches_equal_plain": bool(equal)}
                for k in legs:
                    res["levels"][str(level)][k] = {"wall_s": round(med[k], 4), "genomes_s": round(a.genomes / med[k], 1), "runs_s": [round(x, 4) for x in walls[k]]}
                res["levels"][str(level)]["speedup_vs_no_device_inflate"] = round(med["no_device_inflate"] / med["device_route"], 2)
                if a.parent_cli:
                    res["levels"][str(level)]["speedup_vs_parent"] = round(med["parent"] / med["device_route"], 2)
                if spans:
                    cell = res["levels"][str(level)]
                    best = min(("gunzip_%d" % S for S in spans), key=lambda k: med[k])
                    for k, v in pieces.items():
                        cell[k]["pieces_per_genome"] = v
                    cell["gunzip_best"] = best
                    cell["gunzip_over_device_route"] = round(med["device_route"] / med[best], 2)
                    # faster by more than either leg's spread: the slowest gunzip run against the fastest one-wavefront run
                    cell["gunzip_faster_beyond_spread"] = bool(max(walls[best]) < min(walls["device_route"]))
                    cell["gunzip_over_no_device_inflate"] = round(med["no_device_inflate"] / med[best], 2)
                    if a.parent_cli:
                        cell["gunzip_over_parent"] = round(med["parent"] / med[best], 2)
                    if a.rocprof:
                        os.makedirs(a.rocprof, exist_ok=True)
                        tag = "gunzip_%s_l%d" % (geo, level)
                        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", tag, "--", CLI, "dist", "-L", shuf, "-o", os.path.join(tmp, "prof"),
                                        "--quiet", "--slow-exit"] + legs[best][1] + [gd], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
                        for f in glob.glob(os.path.join(a.rocprof, "**", tag + "_kernel_stats.csv"), recursive=True):
                            rows = list(csv.reader(open(f)))
                            if not stats_rows and rows:
                                stats_rows.append(["cell", "span_bytes"] + rows[0])
                            stats_rows.extend([["%s_gzip%d" % (geo, level), best.split("_")[1]] + r for r in rows[1:]])
                if a.json_out:
                    out["geometries"][geo] = res
                    with open(a.json_out, "w") as f:
                        json.dump(out, f)
                    if stats_rows:
                        with open(os.path.splitext(a.json_out)[0] + "_kernel_stats.csv", "w", newline="") as f:
                            csv.writer(f).writerows(stats_rows)
            if a.rocprof and not spans:
                os.makedirs(a.rocprof, exist_ok=True)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "gzfasta_" + geo, "--", CLI, "dist", "-L", shuf, "-o", os.path.join(tmp, "prof"),
                                "--quiet", "--slow-exit", "--device-inflate", gzdirs[sorted(gzdirs)[-1]][0]], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
            out["geometries"][geo] = res
        out["ok"] = all(v["sketches_equal_plain"] for g in out["geometries"].values() for v in g["levels"].values())
        if a.json_out:
            with open(a.json_out, "w") as f:
                json.dump(out, f)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    return 0 if out.get("ok") else 1


def same_dirs_names(plain_out, gz_out):
    """combco.* byte-equal; cofiles.stat differs in the recorded file names (.fna against .fna.gz) and only there"""
    files = sorted(os.listdir(plain_out))
    if files != sorted(os.listdir(gz_out)):
        return False
    for f in files:
        if f == "cofiles.stat":
            if os.path.getsize(os.path.join(plain_out, f)) != os.path.getsize(os.path.join(gz_out, f)):
                return False
            continue
        if not filecmp.cmp(os.path.join(plain_out, f), os.path.join(gz_out, f), shallow=False):
            return False
    return True


if __name__ == "__main__":
    sys.exit(main())
