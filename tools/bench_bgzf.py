#!/usr/bin/env python3
"""tools/bench_bgzf.py -- BGZF-compressed FASTQ through `metakssd dist -L L3K11.shuf -A`: the device route (inflate, CRC32 and
FASTQ framing on the GPU) against `--no-device-inflate` (the `zcat -fc` pipe, what every other .gz takes) and against `zcat -fc`
alone; prints one JSON line.  `--reader nQ`: the same legs on the other FASTQ reader (`-n 2 -Q 53` in place of `-A`), whose device route
is opt-in: the device leg passes `--device-inflate`, and `--no-device-inflate` is what the command does without a switch.

The input is bench.py's read stream (mk_synth_fastq_write_mt, same seed and read length), compressed to BGZF here with Python's
zlib at level 1 and at level 6 (members of 65280 bytes of text, one raw deflate stream each, the end marker last).  Per level the
three legs run --runs times taking turns; medians are reported and the two sketch directories must be byte-equal.  The inflate
kernel's GB/s are compressed bytes in and text bytes out over its HIP-event time (`--timing`'s route line)."""
import argparse
import filecmp
import json
import os
import shutil
import statistics
import struct
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
SEED, READ_LEN, PAYLOAD = 20261002, 150, 65280  # bench.py's SEED and READ_LEN
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def member(args):
    data, level = args
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    d = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff\x06\x00BC" + struct.pack("<HH", 2, len(d) + 25) + d +
            struct.pack("<II", zlib.crc32(data), len(data)))


def write_bgzf(src, dst, level, procs):
    with open(src, "rb") as f, open(dst, "wb") as g, ProcessPoolExecutor(procs) as ex:
        while True:
            batch = f.read(PAYLOAD * 256)
            if not batch:
                break
            for m in ex.map(member, [(batch[a:a + PAYLOAD], level) for a in range(0, len(batch), PAYLOAD)], chunksize=8):
                g.write(m)
        g.write(EOF_MARKER)
    return os.path.getsize(dst)


READERS = {"A": (["-A"], []), "nQ": (["-n", "2", "-Q", "53"], ["--device-inflate"])}  # reader -> (its flags, the device leg's switch)
READER = READERS["A"]


def run_cli(shuf, out, inp, extra):
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    r = subprocess.run([CLI, "dist", "-L", shuf] + READER[0] + ["-o", out, "--quiet", "--timing"] + extra + [inp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=3000)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode(errors="replace")[-500:])
    route = [json.loads(ln) for ln in r.stdout.decode().splitlines() if ln.startswith('{"input"')]
    return dt, route[0] if route else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--levels", default="1,6")
    ap.add_argument("--procs", type=int, default=16, help="processes that compress the fixture")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--reader", default="A", choices=sorted(READERS), help="A: `dist -A` (mt_shortreads2koc's reader); nQ: `dist -n 2 -Q 53` (fastq2co's)")
    ap.add_argument("--rocprof", default=None, help="directory: one more device-route run per level under `rocprofv3 --kernel-trace --stats`")
    a = ap.parse_args()
    global READER
    READER = READERS[a.reader]
    from golden_cases import make_shuf
    from metakssd_amd import capi
    if capi.device_count() < 1:
        sys.exit("bench_bgzf: no HIP device")
    tmp = tempfile.mkdtemp(prefix="mkbgzf_", dir=a.workdir or ("/dev/shm" if os.path.isdir("/dev/shm") else None))
    out = {"what": "`metakssd dist -L L3K11.shuf %s` on %d reads of %d bases as BGZF (members of %d text bytes), median of %d runs, legs taking turns"
                   % (" ".join(READER[0]), a.reads, READ_LEN, PAYLOAD, a.runs), "reads": a.reads, "device_leg_switch": READER[1], "levels": {}}
    try:
        shuf = os.path.join(tmp, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        fq = os.path.join(tmp, "reads.fq")
        assert capi.lib.mk_synth_fastq_write_mt(fq.encode(), SEED, 0, a.reads, READ_LEN, 16) == 0
        text_bytes = os.path.getsize(fq)
        bases = a.reads * READ_LEN
        out["text_bytes"] = text_bytes
        t_plain = statistics.median(run_cli(shuf, os.path.join(tmp, "plain"), fq, [])[0] for _ in range(3))
        out["plain_fastq"] = {"wall_s": round(t_plain, 4), "gbases_s": round(bases / t_plain / 1e9, 3)}
        for level in [int(x) for x in a.levels.split(",")]:
            gz = os.path.join(tmp, "reads.l%d.fq.gz" % level)
            comp = write_bgzf(fq, gz, level, a.procs)
            dev, zc, zo, kin, kout, infl_ms, frame_ms = [], [], [], [], [], [], []
            d_dev, d_zc = os.path.join(tmp, "dev"), os.path.join(tmp, "zc")
            for _ in range(a.runs):
                dt, route = run_cli(shuf, d_dev, gz, READER[1])
                assert route and route["route"] == "device-inflate" and "fallback" not in route, route
                dev.append(dt)
                infl_ms.append(route["inflate_ms"]); frame_ms.append(route["frame_ms"])
                kin.append(route["comp_bytes"] / route["inflate_ms"] / 1e6)
                kout.append(route["text_bytes"] / route["inflate_ms"] / 1e6)
                dt, route = run_cli(shuf, d_zc, gz, ["--no-device-inflate"])
                assert route and route["route"] == "zcat", route
                zc.append(dt)
                t0 = time.perf_counter()
                subprocess.run(["zcat", "-fc", "--", gz], stdout=subprocess.DEVNULL, check=True)
                zo.append(time.perf_counter() - t0)
            if a.rocprof:
                os.makedirs(a.rocprof, exist_ok=True)
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "bgzf%s_l%d" % ("" if a.reader == "A" else "_" + a.reader, level), "--", CLI, "dist", "-L", shuf] + READER[0] + ["-o",
                                os.path.join(tmp, "prof"), "--quiet", "--slow-exit"] + READER[1] + [gz], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            files = sorted(os.listdir(d_dev))
            equal = files == sorted(os.listdir(d_zc)) and all(filecmp.cmp(os.path.join(d_dev, f), os.path.join(d_zc, f), shallow=False) for f in files)
            md, mz, mo = statistics.median(dev), statistics.median(zc), statistics.median(zo)
            out["levels"][str(level)] = {
                "comp_bytes": comp, "ratio": round(text_bytes / comp, 3),
                "device_route": {"wall_s": round(md, 4), "gbases_s": round(bases / md / 1e9, 3), "runs_s": [round(x, 4) for x in dev]},
                "no_device_inflate": {"wall_s": round(mz, 4), "gbases_s": round(bases / mz / 1e9, 3), "runs_s": [round(x, 4) for x in zc]},
                "zcat_alone": {"wall_s": round(mo, 4), "gbases_s": round(bases / mo / 1e9, 3)},
                "speedup_vs_no_device_inflate": round(mz / md, 2),
                "inflate_kernel": {"ms": round(statistics.median(infl_ms), 3), "gb_s_in": round(statistics.median(kin), 2), "gb_s_out": round(statistics.median(kout), 2)},
                "frame_kernels_ms": round(statistics.median(frame_ms), 3),
                "sketch_dirs_equal": bool(equal),
            }
            os.remove(gz)
        out["ok"] = all(v["sketch_dirs_equal"] for v in out["levels"].values())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out))
    return 0 if out.get("ok") else 1


if __name__ == "__main__":
    sys.exit(main())
