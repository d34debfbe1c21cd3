#!/usr/bin/env python3
"""tests/golden/make_golden_longreads.py -- the golden data of the long-read route (tests/longreads_cases.py), made by the REAL
reference.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`).  The reference cannot
read a FASTQ line of 4 095 characters or more (its fgets() width, iseq2comem.c:656,673), so for every case it runs
`metakssd dist -L <shuf> -A -p 1 -o out` on the CHOPPED file -- every read cut into pieces of at most 4 094 characters that start
every 4 094 - (TL - 1) characters, so that every TL-window lies in exactly one piece, in file order -- and keeps the combco* files
under tests/golden/longreads/<case>/ (the count files combco.N.a as combco.N.a.u16).  That directory is what `dist -A --long-reads`
must write for the unchopped file.  Before anything is kept the recipe asserts on the REFERENCE's output that the case is not
trivial (distinct keys, a count above 1); manifest.json records those numbers, the stat fields and the sha256 of every file, of
both input flavours and of every .shuf.  Nothing here is reference source: the outputs are data produced by executing the reference.
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

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
OUT = os.path.join(HERE, "longreads")
STAT_KEYS = ("shuf_id", "koc", "kmerlen", "dim_rd_len", "comp_num", "infile_num", "all_ctx_ct", "ctx_ct")


def sha(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


def fixture_name(f):
    return f + ".u16" if f.endswith(".a") else f


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/metakssd is missing: make -C oracle ref")
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    manifest = {"cases": {}, "shufs": {}}
    for case, (kind, geom) in lc.CASES.items():
        work = tempfile.mkdtemp(prefix="golden_longreads_")
        try:
            shuf = os.path.join(work, geom + ".shuf")
            lc.get_shuf(geom).write(shuf)
            manifest["shufs"][geom] = sha(shuf)
            chopped = os.path.join(work, case + ".fq")
            open(chopped, "wb").write(lc.chopped(case))
            assert max(len(ln) for ln in lc.chopped(case).split(b"\n")) <= lc.FQ_MAX
            out = os.path.join(work, "out")
            r = subprocess.run([REF, "dist", "-L", shuf, "-A", "-p", "1", "-o", out, chopped], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if r.returncode != 0:
                raise SystemExit("the reference failed on %s:\n%s" % (case, r.stderr.decode(errors="replace")[-400:]))
            st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
            C = st["comp_num"]
            ids = [np.fromfile(os.path.join(out, "combco.%d" % c), dtype="<u4") for c in range(C)]
            cnt = [np.fromfile(os.path.join(out, "combco.%d.a" % c), dtype="<u2") for c in range(C)]
            keys, top = sum(len(x) for x in ids), max(int(x.max()) if len(x) else 0 for x in cnt)
            assert keys >= lc.MIN_KEYS[case] and top > 1, (case, keys, top)  # on the reference's output, before anything is kept
            dst = os.path.join(OUT, case)
            os.makedirs(dst)
            for f in sorted(os.listdir(out)):
                if f.startswith("combco"):
                    shutil.copy(os.path.join(out, f), os.path.join(dst, fixture_name(f)))
            text = lc.fastq(case)
            manifest["cases"][case] = {"kind": kind, "geometry": geom, "stat": {k: st[k] for k in STAT_KEYS}, "keys": keys, "max_count": top,
                                       "reads": len(lc.reads(case)), "longest_read": max(len(s) for s in lc.reads(case)),
                                       "pieces": len(lc.chop(lc.reads(case), lc.TL(geom))),
                                       "fastq_sha256": hashlib.sha256(text).hexdigest(), "chopped_sha256": sha(chopped),
                                       "files": {f: sha(os.path.join(dst, f)) for f in sorted(os.listdir(dst))}}
            print("%-14s keys=%d max_count=%d reads=%d pieces=%d" % (case, keys, top, len(lc.reads(case)), manifest["cases"][case]["pieces"]), flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    sizes = [(os.path.getsize(os.path.join(dp, f)), os.path.relpath(os.path.join(dp, f), OUT)) for dp, _, fs in os.walk(OUT) for f in fs]
    assert max(sizes)[0] <= 256 << 10, max(sizes)
    print("tests/golden/longreads: %d files, %.1f KiB, largest %s" % (len(sizes), sum(s for s, _ in sizes) / 1024.0, max(sizes)))


if __name__ == "__main__":
    main()
