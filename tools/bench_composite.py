#!/usr/bin/env python3
"""tools/bench_composite.py -- `composite -r <markerdb> -q <sketch_dir>` on a synthetic marker database and query directory written
directly as sketch-directory files; prints one JSON line.

Defaults are the README's join figure: about 100 M reference ids over 20 000 sketches (every id private to one sketch, as `set -q`
leaves them), samples of about 1.5 M ids of which 3 % are markers of 50 species.  For every sample count of --counts the command is
timed (wall, process start to exit, median of --runs, the legs taking turns) on
  resident    the marker database resident on the device (--resident)
  per_query   the reference's loop, one join per sample and component (--per-query)
  parent      --parent-cli <metakssd of the parent commit>: the behaviour before the resident route existed
  reference   oracle/_ref/metakssd -p <all cores>, where it exists, at --ref-samples samples only (it takes minutes beyond that)
with the kernel times of --timing beside them, and every leg's stdout is compared byte for byte in the same run.  `per_sample_s` is the
slope between the smallest and the largest count: what one more sample costs.  `crossover` is the smallest measured count from which
on the resident route is the faster one."""
import argparse
import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
MULT = 2654435761  # odd: j -> j * MULT mod 2^32 is a bijection, so distinct j give distinct, scattered ids


def write_stat(d, koc, names):
    n = len(names)
    with open(os.path.join(d, "cofiles.stat"), "wb") as f:
        f.write(struct.pack("<IBxxxiiiiQ", 4242, koc, 22, 6, 1, n, 0))
        f.write(np.zeros(n, np.uint32).tobytes())
        for nm in names:
            f.write(nm.encode().ljust(256, b"\0"))


def ids_of(j):
    return ((j.astype(np.uint64) * MULT) & 0xFFFFFFFF).astype(np.uint32)


def write_db(d, nsketch, per):
    os.makedirs(d)
    write_stat(d, 0, ["species_%05d" % i for i in range(nsketch)])
    n = nsketch * per
    with open(os.path.join(d, "combco.0"), "wb") as f:
        for a in range(0, n, 1 << 24):
            f.write(ids_of(np.arange(a, min(n, a + (1 << 24)), dtype=np.uint64)).tobytes())
    (np.arange(nsketch + 1, dtype=np.uint64) * per).tofile(os.path.join(d, "combco.index.0"))
    return n


def write_queries(d, nsamples, nsketch, per, qlen, hit_frac, species, seed):
    os.makedirs(d)
    write_stat(d, 1, ["sample_%03d.fq" % i for i in range(nsamples)])
    rs = np.random.RandomState(seed)
    nref = nsketch * per
    nhit = int(qlen * hit_frac)
    index = [0]
    with open(os.path.join(d, "combco.0"), "wb") as fi, open(os.path.join(d, "combco.0.a"), "wb") as fa:
        for s in range(nsamples):
            sp = rs.choice(nsketch, size=min(species, nsketch), replace=False)
            each = min(per, max(1, nhit // len(sp)))
            hit = (sp[:, None].astype(np.int64) * per + np.stack([rs.permutation(per)[:each] for _ in sp])).ravel()
            need = qlen - hit.size
            miss = nref + np.unique(rs.randint(0, 1 << 31, size=need + need // 50 + 16))[:need]  # j >= nref: ids no sketch holds
            ids = ids_of(rs.permutation(np.concatenate([hit, miss])))
            fi.write(ids.tobytes())
            fa.write(np.minimum(rs.geometric(0.1, ids.size), 65535).astype(np.uint16).tobytes())
            index.append(index[-1] + ids.size)
    np.asarray(index, np.uint64).tofile(os.path.join(d, "combco.index.0"))


def run(cmd, timing):
    t0 = time.perf_counter()
    r = subprocess.run(cmd + (["--timing"] if timing else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1700)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (cmd[:6], r.stderr.decode(errors="replace")[-500:]))
    lines = r.stdout.split(b"\n")
    tl = [ln for ln in lines if ln.startswith(b'{"composite_timing"')]
    out = b"\n".join(ln for ln in lines if not ln.startswith(b'{"composite_timing"'))
    return dt, hashlib.sha256(out).hexdigest(), out.count(b"\n"), (json.loads(tl[0])["composite_timing"] if tl else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sketches", type=int, default=20000)
    ap.add_argument("--ids-per-sketch", type=int, default=5000)
    ap.add_argument("--sample-ids", type=int, default=1500000)
    ap.add_argument("--hit-frac", type=float, default=0.03)
    ap.add_argument("--species", type=int, default=50, help="species a sample's markers come from")
    ap.add_argument("--counts", default="1,2,4,16,64", help="sample counts to time")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-cli", default=None)
    ap.add_argument("--ref-samples", type=int, default=2)
    ap.add_argument("--no-reference", action="store_true")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    counts = sorted({int(x) for x in a.counts.split(",")})
    tmp = tempfile.mkdtemp(prefix="bench_composite_", dir=a.tmp)
    try:
        db = os.path.join(tmp, "db")
        nref = write_db(db, a.sketches, a.ids_per_sketch)
        res = {"bench": "composite", "ref_ids": nref, "sketches": a.sketches, "sample_ids": a.sample_ids, "hit_frac": a.hit_frac,
               "runs": a.runs, "counts": {}, "outputs_equal": True}
        legs = {"resident": [CLI, "composite", "--resident"], "per_query": [CLI, "composite", "--per-query"]}
        if a.parent_cli:
            legs["parent"] = [a.parent_cli, "composite"]
        for n in counts:
            q = os.path.join(tmp, "q%d" % n)
            write_queries(q, n, a.sketches, a.ids_per_sketch, a.sample_ids, a.hit_frac, a.species, 1000 + n)
            walls = {k: [] for k in legs}
            info, shas, lines = {}, set(), 0
            for _ in range(a.runs):
                for k, cmd in legs.items():    # taking turns: a drift of the machine hits every leg alike
                    dt, h, lines, t = run(cmd + ["-r", db, "-q", q], k != "parent")
                    walls[k].append(dt)
                    shas.add(h)
                    if t:
                        info[k] = t
                print("count %d: %s" % (n, {k: round(v[-1], 3) for k, v in walls.items()}), file=sys.stderr, flush=True)
            row = {"lines": lines}
            for k in legs:
                row[k] = {"wall_s": float(np.median(walls[k])), "wall_runs": [round(x, 4) for x in walls[k]]}
                if k in info:
                    row[k].update({x: info[k][x] for x in ("batches", "hits", "load_kernel_ms", "query_kernel_ms")})
            if os.path.exists(REF) and not a.no_reference and n == a.ref_samples:
                threads = int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count())  # all the cores this process may use
                t0 = time.perf_counter()
                r = subprocess.run([REF, "composite", "-r", db, "-q", q, "-p", str(threads)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   timeout=1700)
                row["reference"] = {"wall_s": time.perf_counter() - t0, "threads": threads, "samples": n}
                shas.add(hashlib.sha256(r.stdout).hexdigest())
            row["outputs_equal"] = len(shas) == 1
            res["outputs_equal"] = res["outputs_equal"] and row["outputs_equal"]
            res["counts"][str(n)] = row
            shutil.rmtree(q)
        lo, hi = str(counts[0]), str(counts[-1])
        if hi != lo:
            res["per_sample_s"] = {k: (res["counts"][hi][k]["wall_s"] - res["counts"][lo][k]["wall_s"]) / (counts[-1] - counts[0]) for k in legs}
        res["crossover"] = None
        for n in reversed(counts):
            if res["counts"][str(n)]["resident"]["wall_s"] < res["counts"][str(n)]["per_query"]["wall_s"]:
                res["crossover"] = n
            else:
                break
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
