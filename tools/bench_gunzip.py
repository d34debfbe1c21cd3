#!/usr/bin/env python3
"""tools/bench_gunzip.py -- an ordinary single-member `.fastq.gz` through `metakssd dist -L L3K11.shuf -A`: the opt-in device route
(`--device-gunzip`: finder, decode to symbols, window chain, resolve, CRC32 and FASTQ framing on the GPU) against
the default route (the `zcat -fc` pipe; with --parent-cli also a binary built from the parent commit), `zcat -fc` alone and the
uncompressed file; prints one JSON line.  Built on tools/bench_bgzf.py's plan.

The input is bench.py's read stream (mk_synth_fastq_write_mt, same seed and read length) compressed as ONE gzip member with zlib at
level 1 and level 6.  Per level the legs run --runs times taking turns, each from process start to the directory on disk; medians
are reported and the sketch directories must be byte-equal.  Then the span size S is timed at 128 KiB .. 1 MiB on the last level's
file, and mk_inflate_stream's piece table gives the largest text-to-compressed ratio any piece showed (what R must stay above).

--members N[,N...]: the same reads as a CONCATENATION of N equal members (cut at byte offsets, so records straddle the boundaries), per
level and N: `--device-gunzip --gunzip-members`, the run without switches and, with --parent-cli, that binary with
`--device-gunzip` (which falls back to zcat for more than one member), taking turns; with --rocprof one more run per file under
`rocprofv3 --kernel-trace --stats`, whose kernel totals go into the JSON line and, as CSV, into that directory.

--reader nQ: the same legs through the other FASTQ reader, `dist -L L3K11.shuf -n 2 -Q 53` (fastq2co's record rule and quality mask,
mk_sketch_push_gzip_q), for the one-member form and for --members.  --parent-switch: the parent's binary gets
`--device-gunzip` too (the shared sink must cost the -A route nothing).  --span-runs 0 leaves out the span sweep and the piece ratios."""
import argparse
import filecmp
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
SEED, READ_LEN = 20261002, 150  # bench.py's SEED and READ_LEN
SPANS = (128 << 10, 256 << 10, 512 << 10, 1 << 20)
READERS = {"A": ["-A"], "nQ": ["-n", "2", "-Q", "53"]}
READER = READERS["A"]  # --reader


def compress(args):
    src, dst, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    with open(src, "rb") as f, open(dst, "wb") as g:
        while True:
            b = f.read(16 << 20)
            if not b:
                break
            g.write(c.compress(b))
        g.write(c.flush())
    return os.path.getsize(dst)


def compress_part(args):
    src, at, n, level = args
    with open(src, "rb") as f:
        f.seek(at)
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        return c.compress(f.read(n)) + c.flush()


def write_members(src, dst, level, members, ex):
    """src as `members` gzip members of equal text size, one behind the other"""
    size = os.path.getsize(src)
    cuts = [size * k // members for k in range(members + 1)]
    with open(dst, "wb") as g:
        for part in ex.map(compress_part, [(src, a, b - a, level) for a, b in zip(cuts, cuts[1:])], chunksize=max(1, members // 64)):
            g.write(part)
    return os.path.getsize(dst)


def kernel_totals(directory, name):
    """{kernel: total ms} from the kernel_stats CSV rocprofv3 wrote for -o `name`; {} when there is none"""
    import csv
    import glob
    out = {}
    for path in glob.glob(os.path.join(directory, "**", name + "_kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            m = re.search(r"\bmk_[a-z0-9_]+", row.get("Name", ""))  # (names come with return type, namespace and argument list)
            if m:
                out[m.group(0)] = round(out.get(m.group(0), 0.0) + float(row["TotalDurationNs"]) / 1e6, 3)
    return out


def bench_members(a, tmp, shuf, fq, levels, out):
    text_bytes, bases = os.path.getsize(fq), a.reads * READ_LEN
    gb = lambda t: round(bases / t / 1e9, 3)
    leg = lambda ts: {"wall_s": med(ts), "gbases_s": gb(statistics.median(ts)), "runs_s": [round(x, 4) for x in ts]}
    counts = [int(x) for x in a.members.split(",")]
    out["members"] = {}
    gz = os.path.join(tmp, "reads.members.fq.gz")
    with ProcessPoolExecutor(16) as ex:
        for lv in levels:
            for n in counts:
                comp = write_members(fq, gz, lv, n, ex)
                print("bench_gunzip: level %d, %d members, %d bytes" % (lv, n, comp), file=sys.stderr, flush=True)
                dev, zc, par, routes, par_routes = [], [], [], [], []
                d_dev, d_zc, d_par = os.path.join(tmp, "dev"), os.path.join(tmp, "zc"), os.path.join(tmp, "par")
                for _ in range(a.runs):
                    dt, route = run_cli(CLI, shuf, d_dev, gz, ["--device-gunzip", "--gunzip-members"])
                    assert route and route["route"] == "device-gunzip" and route["members"] == n, route
                    dev.append(dt); routes.append(route)
                    dt, route = run_cli(CLI, shuf, d_zc, gz, [])
                    assert route and route["route"] == "zcat" and "fallback" not in route, route
                    zc.append(dt)
                    if a.parent_cli:
                        dt, route = run_cli(a.parent_cli, shuf, d_par, gz, ["--device-gunzip"])
                        par.append(dt); par_routes.append(route)
                k = {f: med([r[f] for r in routes]) for f in ("find_ms", "decode_ms", "resolve_ms", "frame_ms", "read_s", "route_total_s")}
                e = {"comp_bytes": comp, "pieces": routes[0]["pieces"], "batches": routes[0]["batches"], "members": routes[0]["members"],
                     "device_gunzip_members": leg(dev), "zcat_route": leg(zc), "kernels_ms": k,
                     "sketch_dirs_equal": bool(same(d_dev, d_zc) and (not par or same(d_dev, d_par)))}
                if par:
                    e["parent_device_gunzip"] = dict(leg(par), route=par_routes[0]["route"], fallback=par_routes[0].get("fallback"))
                    e["speedup_vs_parent"] = round(statistics.median(par) / statistics.median(dev), 2)
                if a.rocprof:
                    os.makedirs(a.rocprof, exist_ok=True)
                    name = "gunzip_members_%sl%d_m%d" % ("" if a.reader == "A" else a.reader + "_", lv, n)
                    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", name, "--", CLI, "dist", "-L", shuf] + READER + [
                                    "-o", os.path.join(tmp, "prof"), "--quiet", "--slow-exit", "--device-gunzip", "--gunzip-members", gz],
                                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
                    e["rocprof_kernel_totals_ms"] = kernel_totals(a.rocprof, name)
                out["members"]["l%d_m%d" % (lv, n)] = e
    out["ok"] = all(v["sketch_dirs_equal"] for v in out["members"].values())


def run_cli(cli, shuf, out, inp, extra):
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    r = subprocess.run([cli, "dist", "-L", shuf] + READER + ["-o", out, "--quiet", "--timing"] + extra + [inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=3000)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode(errors="replace")[-500:])
    route = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return dt, route[0] if route else None


def zcat_alone(gz):
    t0 = time.perf_counter()
    subprocess.run(["zcat", "-fc", "--", gz], stdout=subprocess.DEVNULL, check=True)
    return time.perf_counter() - t0


def same(a, b):
    files = sorted(os.listdir(a))
    return files == sorted(os.listdir(b)) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in files)


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--span-runs", type=int, default=3)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--parent-cli", default=None, help="a metakssd binary built from the parent commit: its default route is timed too")
    ap.add_argument("--members", default=None, help="N[,N...]: the reads as N equal gzip members; times the --gunzip-members route instead of the one-member legs")
    ap.add_argument("--reader", choices=sorted(READERS), default="A", help="A: dist -A (the counted sketch); nQ: dist -n 2 -Q 53 (fastq2co's reader)")
    ap.add_argument("--parent-switch", action="store_true", help="the parent's binary runs with --device-gunzip too, not on its default route")
    ap.add_argument("--rocprof", default=None, help="directory: one more device-route run per level under `rocprofv3 --kernel-trace --stats`")
    a = ap.parse_args()
    global READER
    READER = READERS[a.reader]
    from golden_cases import make_shuf
    from metakssd_amd import capi
    if capi.device_count() < 1:
        sys.exit("bench_gunzip: no HIP device")
    tmp = tempfile.mkdtemp(prefix="mkgunzip_", dir=a.workdir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    levels = [int(x) for x in a.levels.split(",")]
    out = {"what": "`metakssd dist -L L3K11.shuf %s` on %d reads of %d bases as ONE gzip member, median of %d runs from process start to the "
                   "directory on disk, legs taking turns" % (" ".join(READER), a.reads, READ_LEN, a.runs), "reader": a.reader, "reads": a.reads, "levels": {}}
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        fq = os.path.join(tmp, "reads.fq")
        assert capi.lib.mk_synth_fastq_write_mt(fq.encode(), SEED, 0, a.reads, READ_LEN, 16) == 0
        text_bytes, bases = os.path.getsize(fq), a.reads * READ_LEN
        out["text_bytes"] = text_bytes
        if a.members:
            bench_members(a, tmp, shuf, fq, levels, out)
            print(json.dumps(out))
            return 0 if out.get("ok") else 1
        gzs = {lv: os.path.join(tmp, "reads.l%d.fq.gz" % lv) for lv in levels}
        with ProcessPoolExecutor(len(levels)) as ex:
            comps = dict(zip(levels, ex.map(compress, [(fq, gzs[lv], lv) for lv in levels])))
        d_plain = os.path.join(tmp, "plain")
        t_plain = statistics.median(run_cli(CLI, shuf, d_plain, fq, [])[0] for _ in range(3))
        out["plain_fastq"] = {"wall_s": round(t_plain, 4), "gbases_s": round(bases / t_plain / 1e9, 3)}
        gb = lambda t: round(bases / t / 1e9, 3)
        prof = {}
        for lv in levels:
            print("bench_gunzip: level %d, %d bytes" % (lv, comps[lv]), file=sys.stderr, flush=True)
            gz = gzs[lv]
            dev, zc, par, zo, routes = [], [], [], [], []
            d_dev, d_zc = os.path.join(tmp, "dev"), os.path.join(tmp, "zc")
            for _ in range(a.runs):
                dt, route = run_cli(CLI, shuf, d_dev, gz, ["--device-gunzip"])
                assert route and route["route"] == "device-gunzip", route
                dev.append(dt); routes.append(route)
                dt, route = run_cli(CLI, shuf, d_zc, gz, [])
                assert route and route["route"] == "zcat" and "fallback" not in route, route
                zc.append(dt)
                if a.parent_cli and a.parent_switch:
                    # a device-route process right behind another GPU process takes 0.2 s longer from start to exit than one behind
                    # two seconds of `zcat` alone (profiles/r16_gunzip_q_bench.json): both binaries' device legs follow such a leg
                    zo.append(zcat_alone(gz))
                    par.append(run_cli(a.parent_cli, shuf, os.path.join(tmp, "par"), gz, ["--device-gunzip"])[0])
                elif a.parent_cli:
                    par.append(run_cli(a.parent_cli, shuf, os.path.join(tmp, "par"), gz, [])[0])
                zo.append(zcat_alone(gz))
            if a.rocprof:
                os.makedirs(a.rocprof, exist_ok=True)
                name = "gunzip_%sl%d" % ("" if a.reader == "A" else a.reader + "_", lv)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.rocprof, "-o", name, "--", CLI, "dist", "-L", shuf] + READER + ["-o",
                                os.path.join(tmp, "prof"), "--quiet", "--slow-exit", "--device-gunzip", gz], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
                prof[lv] = kernel_totals(a.rocprof, name)
            k = {f: med([r[f] for r in routes]) for f in ("find_ms", "decode_ms", "resolve_ms", "frame_ms", "read_s", "route_total_s")}
            out["levels"][str(lv)] = {
                "comp_bytes": comps[lv], "ratio": round(text_bytes / comps[lv], 3), "pieces": routes[0]["pieces"], "batches": routes[0]["batches"],
                "device_gunzip": {"wall_s": med(dev), "gbases_s": gb(statistics.median(dev)), "runs_s": [round(x, 4) for x in dev]},
                "zcat_route": {"wall_s": med(zc), "gbases_s": gb(statistics.median(zc)), "runs_s": [round(x, 4) for x in zc]},
                "parent_device_gunzip" if a.parent_switch else "parent_zcat_route":
                    {"wall_s": med(par), "gbases_s": gb(statistics.median(par)), "runs_s": [round(x, 4) for x in par]} if par else None,
                "zcat_alone": {"wall_s": med(zo), "gbases_s": gb(statistics.median(zo))},
                "speedup_vs_zcat_route": round(statistics.median(zc) / statistics.median(dev), 2),
                "speedup_vs_parent": round(statistics.median(par) / statistics.median(dev), 2) if par else None,
                "kernels_ms": k,
                "rocprof_kernel_totals_ms": prof.get(lv),
                "decode_text_gb_s": round(text_bytes / k["decode_ms"] / 1e6, 2),
                "sketch_dirs_equal": bool(same(d_dev, d_zc) and (not par or same(d_dev, os.path.join(tmp, "par")))),
            }
        if a.span_runs <= 0:
            out["ok"] = all(v["sketch_dirs_equal"] for v in out["levels"].values())
            print(json.dumps(out))
            return 0 if out["ok"] else 1
        # the span size, on the last level's file
        gz, sweep = gzs[levels[-1]], {}
        for S in SPANS:
            print("bench_gunzip: span %d" % S, file=sys.stderr, flush=True)
            ts, rs = [], []
            for _ in range(a.span_runs):
                dt, route = run_cli(CLI, shuf, os.path.join(tmp, "dev"), gz, ["--device-gunzip", "--gunzip-span-bytes", str(S)])
                assert route and route["route"] == "device-gunzip", route
                ts.append(dt); rs.append(route)
            sweep[str(S)] = {"wall_s": med(ts), "pieces": rs[0]["pieces"], "batches": rs[0]["batches"],
                             "find_ms": med([r["find_ms"] for r in rs]), "decode_ms": med([r["decode_ms"] for r in rs]), "resolve_ms": med([r["resolve_ms"] for r in rs])}
        out["span_sweep_level_%d" % levels[-1]] = sweep
        # the largest ratio a piece showed, at the default span
        worst = {}
        infl = capi.Inflate(0)
        for lv in levels:
            comp = open(gzs[lv], "rb").read()
            info = capi.gzip_scan_stream(comp)
            text, st, pieces, n = infl.stream(comp, cap=text_bytes)
            assert st == 0 and n == text_bytes and zlib.crc32(text) == info["crc32"]
            ends = [p for p, _ in pieces[1:]] + [8 * info["pay_len"]]
            worst[str(lv)] = round(max(n / ((e + 7) // 8 - p // 8) for (p, n), e in zip(pieces, ends)), 2)
            del comp, text
        infl.close()
        out["largest_piece_ratio"] = worst
        out["ok"] = all(v["sketch_dirs_equal"] for v in out["levels"].values())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    return 0 if out.get("ok") else 1


if __name__ == "__main__":
    sys.exit(main())
