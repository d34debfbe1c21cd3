#!/usr/bin/env python3
"""tests/golden/make_golden_longreads_q.py -- the golden data of the long route of the -n / -Q reader (tests/longreads_q_cases.py),
made by the REAL reference.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`).  For every `lengths_q`
case it writes the CHOPPED file -- sequence and quality lines cut at the same places, every TL-window with its qualities in exactly
one piece, in file order -- and runs `metakssd dist -L <shuf> -n M -Q q -p 1 -o out` on it for (M, q) = (1, 0), (1, 53), (2, 53).
The combco* files go to tests/golden/longreads_q/<case>/n<M>_Q<q>/: what `dist -n M -Q q --long-reads-q` must write for the
unchopped file.  Before anything is kept the recipe asserts on the REFERENCE's output that every directory reaches the case's
minimum of keys, that the mask removes keys (Q 53 against Q 0) and that the threshold removes keys but not all (-n 2 against -n 1).
manifest.json records the key counts, the stat fields and the sha256 of every file, of both input flavours and of every .shuf.
Nothing here is reference source: the outputs are data produced by executing the reference.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byread_model as bm  # noqa: E402
import longreads_cases as lc  # noqa: E402
import longreads_q_cases as qc  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
OUT = os.path.join(HERE, "longreads_q")
STAT_KEYS = ("shuf_id", "koc", "kmerlen", "dim_rd_len", "comp_num", "infile_num", "all_ctx_ct", "ctx_ct")


def sha(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


def sub(M, Q):
    return "n%d_Q%d" % (M, Q)


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/metakssd is missing: make -C oracle ref")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = {"cases": {}, "shufs": {}}
    for case in qc.FIXTURE_CASES:
        geom = qc.CASES[case][1]
        work = tempfile.mkdtemp(prefix="golden_longreads_q_")
        try:
            shuf = os.path.join(work, geom + ".shuf")
            lc.get_shuf(geom).write(shuf)
            manifest["shufs"][geom] = sha(shuf)
            chopped = os.path.join(work, case + ".fq")
            open(chopped, "wb").write(qc.chopped(case))
            assert max(len(ln) for ln in qc.chopped(case).split(b"\n")) <= lc.FQ_MAX
            sets, dirs = {}, {}
            for M, Q in qc.MQ:
                out = os.path.join(work, sub(M, Q))
                r = subprocess.run([REF, "dist", "-L", shuf, "-n", str(M), "-Q", str(Q), "-p", "1", "-o", out, chopped], cwd=work,
                                   stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                if r.returncode != 0:
                    raise SystemExit("the reference failed on %s %s:\n%s" % (case, sub(M, Q), r.stderr.decode(errors="replace")[-400:]))
                st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
                ids = [np.fromfile(os.path.join(out, "combco.%d" % c), dtype="<u4") for c in range(st["comp_num"])]
                sets[(M, Q)] = {(c, int(x)) for c, a in enumerate(ids) for x in a}
                dirs[(M, Q)] = (out, st)
            # on the reference's output, before anything is kept
            assert all(len(s) >= qc.MIN_KEYS[case] for s in sets.values()), (case, {k: len(s) for k, s in sets.items()})
            assert sets[(1, 53)] < sets[(1, 0)], (case, "the mask removes nothing")
            assert sets[(2, 53)] and sets[(2, 53)] < sets[(1, 53)], (case, "the threshold removes nothing, or everything")
            entry = {"geometry": geom, "reads": len(qc.reads(case)), "longest_read": max(len(s) for s in qc.reads(case)),
                     "pieces": len(qc.chop_q(qc.reads(case), qc.quals(case), qc.TL(case))),
                     "fastq_sha256": hashlib.sha256(qc.fastq(case)).hexdigest(), "chopped_sha256": sha(chopped), "runs": {}}
            for (M, Q), (out, st) in dirs.items():
                dst = os.path.join(OUT, case, sub(M, Q))
                os.makedirs(dst)
                for f in sorted(os.listdir(out)):
                    if f.startswith("combco"):
                        shutil.copy(os.path.join(out, f), os.path.join(dst, f))
                entry["runs"][sub(M, Q)] = {"M": M, "Q": Q, "keys": len(sets[(M, Q)]), "stat": {k: st[k] for k in STAT_KEYS},
                                            "files": {f: sha(os.path.join(dst, f)) for f in sorted(os.listdir(dst))}}
            manifest["cases"][case] = entry
            print("%-16s %s reads=%d pieces=%d" % (case, {sub(*k): len(s) for k, s in sets.items()}, entry["reads"], entry["pieces"]), flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    sizes = [(os.path.getsize(os.path.join(dp, f)), os.path.relpath(os.path.join(dp, f), OUT)) for dp, _, fs in os.walk(OUT) for f in fs]
    assert max(sizes)[0] <= 256 << 10, max(sizes)
    print("tests/golden/longreads_q: %d files, %.1f KiB, largest %s" % (len(sizes), sum(s for s, _ in sizes) / 1024.0, max(sizes)))


if __name__ == "__main__":
    main()
