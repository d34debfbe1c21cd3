#!/usr/bin/env python3
"""tools/bench_abv.py -- `composite -i` / `composite -s` on a synthetic database the size of the GTDB r214 marker database
(85 205 species), 10^5 samples of 300 species each; prints one JSON line.

  index   device time of mk_abv_index (HIP events), wall time of `metakssd composite -r db -i` and of the reference's
  search  device time of mk_abv_search per metric for 1 and for 64 queries (after one warm-up call of the same shape)
  cli     wall time of `composite -r db -s M <64 queries>` per metric, split into read / device / format (MK_ABV_TIMES), and
          the reference's wall time for the same command; output_equals_reference compares the stdout bytes
  bytes   what the kernels have to move (computed from the shapes) against the 8 TB/s HBM roofline
oracle/_ref/metakssd is used where it exists (built by `make -C oracle ref`); without it the reference fields are null."""
import argparse
import hashlib
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
import numpy as np  # noqa: E402

import abv_model as am  # noqa: E402
from metakssd_amd import capi  # noqa: E402

CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
HBM = 8e12


def vec(rs, nref, k):
    r = np.unique(rs.randint(0, nref, size=k + k // 4 + 16))
    r = rs.permutation(r)[:k]
    v = np.zeros(len(r), am.BINVEC)
    v["r"] = r
    p = rs.gamma(0.7, 1.0, size=len(r)) + 1e-3
    v["p"] = (p * 100.0 / p.sum()).astype(np.float32)
    return v


def timed(cmd, out_path=None, env=None):
    t0 = time.perf_counter()
    with open(out_path or os.devnull, "wb") as f:
        r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, env=env, timeout=1800)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (cmd[:4], r.stderr.decode(errors="replace")[-500:]))
    return dt, r.stderr.decode(errors="replace")


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--species", type=int, default=85205)
    ap.add_argument("--per", type=int, default=300)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("bench_abv: no HIP device")
    work = tempfile.mkdtemp(dir=a.workdir)
    res = {"what": "composite -i / -s", "samples": a.samples, "species": a.species, "species_per_sample": a.per, "queries": a.queries}
    try:
        rs = np.random.RandomState(a.seed)
        db = os.path.join(work, "db")
        vecs = [vec(rs, a.species, a.per) for _ in range(a.samples)]
        am.write_db(db, a.species, [("s%06d.abv" % i, v) for i, v in enumerate(vecs)])
        qdir = os.path.join(work, "q")
        os.makedirs(qdir)
        queries = [vec(rs, a.species, a.per) for _ in range(a.queries)]
        qpaths = []
        for i, q in enumerate(queries):
            qpaths.append(os.path.join(qdir, "q%03d.abv" % i))
            q.tofile(qpaths[-1])
        n = sum(len(v) for v in vecs)
        res["entries"] = n

        # -i: the command line (wall), the library (device), the reference (wall)
        wall, _ = timed([CLI, "composite", "-r", db, "-i"])
        res["index_cli_wall_s"] = round(wall, 4)
        mine = {s: sha(os.path.join(db, "abundance_Vec." + s)) for s in ("name", "yl2n", "abm", "abmi")}
        names = am.dir_order(db)
        order = [int(nm[1:7]) for nm in names]
        ab = capi.Abv(0)
        ab.index([vecs[i] for i in order], a.species)
        abm, abmi, yl2n = ab.index([vecs[i] for i in order], a.species)
        res["index_device_ms"] = round(ab.last_kernel_ms()[0], 4)
        if os.path.exists(REF):
            wall, _ = timed([REF, "composite", "-r", db, "-i"])
            res["index_ref_wall_s"] = round(wall, 4)
            res["index_equals_reference"] = mine == {s: sha(os.path.join(db, "abundance_Vec." + s)) for s in mine}
        else:
            res["index_ref_wall_s"] = res["index_equals_reference"] = None

        # -s through the library: device time per metric, 1 and 64 queries
        ab.load(abm, abmi, yl2n)
        col = np.diff(np.concatenate([[0], abmi.astype(np.int64)]))
        search = {}
        for metric in (0, 1, 2):
            for nq in (1, a.queries):
                ab.search(metric, queries[:nq])
                out = ab.search(metric, queries[:nq])
                ms = ab.last_kernel_ms()[1]
                matched = sum(len(o[0]) for o in out)
                touched = int(sum(col[q["r"]].sum() for q in queries[:nq]))
                # column entries read (8 B), dense first/measure written and read back (16 B per query and sample), the matched
                # samples through compaction, three sorts of up to four passes and the output (about 100 B each)
                byts = touched * 8 + nq * a.samples * 16 + matched * 100
                search["m%d_q%d" % (metric, nq)] = {"device_ms": round(ms, 4), "matched": matched, "bytes": byts,
                                                    "hbm_roofline_ms": round(byts / HBM * 1e3, 5)}
        res["search"] = search
        ab.close()
        res["index_bytes"] = n * 100  # prep 16, three radix passes of 20, gather 20, norms 8 (per entry, computed)
        res["index_hbm_roofline_ms"] = round(n * 100 / HBM * 1e3, 5)

        # -s on the command line, 64 queries per metric
        cli = {}
        env = dict(os.environ, MK_ABV_TIMES="1")
        for metric in (0, 1, 2):
            po = os.path.join(work, "mine_s%d.txt" % metric)
            wall, err = timed([CLI, "composite", "-r", db, "-s", str(metric)] + qpaths, po, env)
            split = json.loads(err.strip().splitlines()[-1])
            e = {"wall_s": round(wall, 4), "read_s": round(split["read_s"], 4), "device_s": round(split["device_s"], 4),
                 "format_s": round(split["format_s"], 4), "stdout_bytes": os.path.getsize(po)}
            if os.path.exists(REF):
                ro = os.path.join(work, "ref_s%d.txt" % metric)
                rw, _ = timed([REF, "composite", "-r", db, "-s", str(metric)] + qpaths, ro)
                e["ref_wall_s"] = round(rw, 4)
                e["output_equals_reference"] = sha(po) == sha(ro)
                os.remove(ro)
            else:
                e["ref_wall_s"] = e["output_equals_reference"] = None
            os.remove(po)
            cli["m%d" % metric] = e
        res["cli"] = cli
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
