#!/usr/bin/env python3
"""tests/golden/make_golden_seams.py -- the golden data of the seam inputs (tests/seam_cases.py), made by the REAL reference.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`).  The oracle is pinned to
the reference at 150-base reads and at L0K6 / L1K7 long reads; this pins it at the TUNED geometries with long ragged rows: for the
pitch-272 input of L3K11, L3K10, L3K9 and L2K11 and for the L3K11 pitch-4096 input with rows of at most 4 094 bases (the
reference's fgets() width, iseq2comem.c:656,673) it runs `metakssd dist -L <shuf> -A -p 1 -o out` on the FASTQ form of the rows and
keeps the combco* files under tests/golden/seams/<case>/ (the count files combco.N.a as combco.N.a.u16).  Before anything is kept
the recipe asserts on the REFERENCE's output that every planted key is there with its expected count (seam_cases.check_conditions);
manifest.json records those counts, the stat fields and the sha256 of every file, of the input and of every .shuf.  Nothing here is
reference source: the outputs are data produced by executing the reference.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byread_model as bm  # noqa: E402
import seam_cases as sc  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
OUT = sc.GOLD
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
    for name, (geom, pitch, lmax) in sc.GOLDEN.items():
        work = tempfile.mkdtemp(prefix="golden_seams_")
        try:
            shuf = os.path.join(work, geom + ".shuf")
            sc.get_shuf(geom).write(shuf)
            manifest["shufs"][geom] = sha(shuf)
            case = sc.get_case(geom, pitch, lmax)
            text = case.fastq()
            assert max(len(ln) for ln in text.split(b"\n")) <= 4094
            fq = os.path.join(work, name + ".fq")
            open(fq, "wb").write(text)
            out = os.path.join(work, "out")
            r = subprocess.run([REF, "dist", "-L", shuf, "-A", "-p", "1", "-o", out, fq], cwd=work, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            if r.returncode != 0:
                raise SystemExit("the reference failed on %s:\n%s" % (name, r.stderr.decode(errors="replace")[-400:]))
            st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
            info = sc.check_conditions(case, sc.load_dir(out, st["comp_num"]))  # on the reference's output, before anything is kept
            assert info["distinct_keys"] == st["all_ctx_ct"], (name, info["distinct_keys"], st["all_ctx_ct"])
            dst = os.path.join(OUT, name)
            os.makedirs(dst)
            for f in sorted(os.listdir(out)):
                if f.startswith("combco"):
                    shutil.copy(os.path.join(out, f), os.path.join(dst, fixture_name(f)))
            manifest["cases"][name] = {"geometry": geom, "pitch": pitch, "longest_row": case.lmax, "stat": {k: st[k] for k in STAT_KEYS},
                                       "keys": info["distinct_keys"], "rows": info["rows"], "planted": info["planted"],
                                       "planted_counts": info["planted_counts"], "fastq_sha256": hashlib.sha256(text).hexdigest(),
                                       "files": {f: sha(os.path.join(dst, f)) for f in sorted(os.listdir(dst))}}
            print("%-12s rows=%d planted=%d keys=%d" % (name, info["rows"], info["planted"], info["distinct_keys"]), flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    sizes = [(os.path.getsize(os.path.join(dp, f)), os.path.relpath(os.path.join(dp, f), OUT)) for dp, _, fs in os.walk(OUT) for f in fs]
    assert max(sizes)[0] <= 256 << 10, max(sizes)
    print("tests/golden/seams: %d files, %.1f KiB, largest %s" % (len(sizes), sum(s for s, _ in sizes) / 1024.0, max(sizes)))


if __name__ == "__main__":
    main()
