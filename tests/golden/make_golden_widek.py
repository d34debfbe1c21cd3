#!/usr/bin/env python3
"""tests/golden/make_golden_widek.py -- the golden data of the wide k-mer geometries (k 12-16, tests/widek_cases.py), made by the
REAL reference.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`).  For every geometry
it runs `metakssd dist -L <shuf> -p 1 -o out` on the planted input as FASTA, FASTA -u, FASTQ -A and FASTQ -n 2 -Q 53 and keeps the
combco* files under tests/golden/widek/<geometry>_<flavour>/ (the count files combco.N.a as combco.N.a.u16); for the geometries of
widek_cases.BYREAD also `dist --byread` with
`reverse -b` (stdout, gzip-compressed) and plain `reverse -o` on a sketch directory laid out by oracle/kssd_oracle_cli (the
reference's dist shuffles its inputs by the clock).  Before anything is kept, widek_cases.check_conditions() asserts on the
REFERENCE's output what the inputs were built for (distinct keys, top bits, both strands, counts, colliding unituples, sixteen
non-empty components); its counts go to manifest.json beside the stat fields and the sha256 of every file and every .shuf.
Nothing here is reference source: the outputs are data produced by executing the reference.
"""
import gzip
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
import widek_cases as wc  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
ORA = os.path.join(ROOT, "oracle", "kssd_oracle_cli")
OUT = os.path.join(HERE, "widek")
STAT_KEYS = ("shuf_id", "koc", "kmerlen", "dim_rd_len", "comp_num", "infile_num", "all_ctx_ct")


def sha(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise SystemExit("failed: %s\n%s" % (" ".join(cmd), r.stderr.decode(errors="replace")[-400:]))
    return r.stdout


def keep_combco(src, dst):
    os.makedirs(dst)
    for f in sorted(os.listdir(src)):
        if f.startswith("combco"):
            shutil.copy(os.path.join(src, f), os.path.join(dst, wc.fixture_name(f)))


def tree(d):
    return {os.path.relpath(os.path.join(dp, f), d): sha(os.path.join(dp, f)) for dp, _, fs in os.walk(d) for f in sorted(fs)}


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/metakssd is missing: make -C oracle ref")
    only = sys.argv[1:]
    manifest = {"geometries": {}, "cases": {}, "byread_cases": {}, "reverse_cases": {}}
    if only:  # remake some geometries, keep the others
        manifest = json.load(open(os.path.join(OUT, "manifest.json")))
    else:
        shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT, exist_ok=True)
    for name in (only or list(wc.GEOMS)):
        work = tempfile.mkdtemp(prefix="golden_widek_")
        try:
            k, subk, drl, seed = wc.GEOMS[name]
            shuf = os.path.join(work, name + ".shuf")
            wc.get_shuf(name).write(shuf)
            inp, P = wc.get_input(name), wc.params(name)
            files = {"fa": os.path.join(work, name + ".fa"), "fq": os.path.join(work, name + ".fq")}
            open(files["fa"], "wb").write(inp.fasta())
            open(files["fq"], "wb").write(inp.fastq())
            outs = {}
            for flavour, (kind, flags) in wc.FLAVOURS.items():
                case = name + "_" + flavour
                out = os.path.join(work, case + ".out")
                run([REF, "dist", "-L", shuf] + flags + ["-p", "1", "-o", out, files[kind]], work)
                outs[flavour] = out
            C = P.component_num
            koc_ids = [np.fromfile(os.path.join(outs["fq_A"], "combco.%d" % c), dtype="<u4") for c in range(C)]
            koc_cnt = [np.fromfile(os.path.join(outs["fq_A"], "combco.%d.a" % c), dtype="<u2") for c in range(C)]
            set_ids = [np.fromfile(os.path.join(outs["fa"], "combco.%d" % c), dtype="<u4") for c in range(C)]
            cond = wc.check_conditions(name, koc_ids, koc_cnt, set_ids)  # on the reference's output, before anything is kept
            assert sum(os.path.getsize(os.path.join(outs["fq_n2Q53"], "combco.%d" % c)) for c in range(C)) >= 4 * 100, name
            manifest["geometries"][name] = {"k": k, "subk": subk, "drlevel": drl, "seed": seed, "shuf_sha256": sha(shuf),
                                            "clamped": wc.clamped(name), "hashsize": int(wc.get_shuf(name).params().hashsize),
                                            "fasta_sha256": hashlib.sha256(inp.fasta()).hexdigest(),
                                            "fastq_sha256": hashlib.sha256(inp.fastq()).hexdigest(), "conditions": cond}
            for flavour, (kind, flags) in wc.FLAVOURS.items():
                case = name + "_" + flavour
                shutil.rmtree(os.path.join(OUT, case), ignore_errors=True)
                keep_combco(outs[flavour], os.path.join(OUT, case))
                st = bm.parse_stat(os.path.join(outs[flavour], "cofiles.stat"))
                manifest["cases"][case] = {"geometry": name, "input": kind, "flags": flags, "stat": {x: st[x] for x in STAT_KEYS + ("ctx_ct",)},
                                           "files": tree(os.path.join(OUT, case))}
            print("%-8s %s" % (name, cond), flush=True)
            if name in wc.BYREAD:
                case = name + "_byread"
                out, again = os.path.join(work, "br.out"), os.path.join(work, "br.again")
                run([REF, "dist", "-L", shuf, "--byread", "-p", "1", "-o", out, files["fa"]], work)
                run([REF, "dist", "-L", shuf, "--byread", "-p", "1", "-o", again, files["fa"]], work)
                text = run([REF, "reverse", "-L", shuf, "-b", out], work)
                d = os.path.join(OUT, case)
                shutil.rmtree(d, ignore_errors=True)
                keep_combco(out, d)
                for f in os.listdir(d):  # (no count files in a by-read directory: the names are the reference's)
                    assert open(os.path.join(d, f), "rb").read() == open(os.path.join(again, f), "rb").read(), (case, f)
                with gzip.GzipFile(os.path.join(d, "reverse_b.txt.gz"), "wb", mtime=0) as g:
                    g.write(text)
                st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
                ids = sum(os.path.getsize(os.path.join(d, "combco.%d" % c)) // 4 for c in range(C))
                assert ids >= wc.MIN_KEYS[name]
                manifest["byread_cases"][case] = {"geometry": name, "header": {x: st[x] for x in STAT_KEYS}, "ids": ids,
                                                  "records": os.path.getsize(os.path.join(d, "combco.index.0")) // 8 - 1,
                                                  "reverse_b_sha256": hashlib.sha256(text).hexdigest(), "files": tree(d)}
                # plain reverse: a sketch directory of the FASTA text, a file too short for any id, and the text's second half
                case = name + "_reverse"
                names = [name + ".fa", "tiny.fa", name + "_half.fa"]
                open(os.path.join(work, "tiny.fa"), "wb").write(wc.TINY)
                open(os.path.join(work, names[2]), "wb").write(b"".join(inp.fasta_files(2)[1:]))
                sk, rv = os.path.join(work, "rv.sk"), os.path.join(work, "rv.out")
                run([ORA, "-L", shuf, "-o", sk] + [os.path.join(work, n) for n in names], work)
                os.makedirs(rv)
                run([REF, "reverse", "-L", shuf, "-o", rv, "-p", "1", sk], work)
                d = os.path.join(OUT, case)
                shutil.rmtree(d, ignore_errors=True)
                keep_combco(sk, os.path.join(d, "sketch"))
                os.makedirs(os.path.join(d, "kmers"))
                for f in sorted(os.listdir(rv)):
                    with gzip.GzipFile(os.path.join(d, "kmers", f + ".gz"), "wb", mtime=0) as g:
                        g.write(open(os.path.join(rv, f), "rb").read())
                st = bm.parse_stat(os.path.join(sk, "cofiles.stat"))
                assert sorted(os.listdir(rv)) == sorted([names[0], names[2]]) and st["ctx_ct"][1] == 0
                manifest["reverse_cases"][case] = {"geometry": name, "inputs": names, "header": {x: st[x] for x in STAT_KEYS}, "ctx_ct": st["ctx_ct"],
                                                   "names": [os.path.basename(n) for n in st["names"]],
                                                   "outputs": {f: sha(os.path.join(rv, f)) for f in sorted(os.listdir(rv))}, "files": tree(d)}
                print("%-8s byread ids=%d, reverse -b %d bytes, reverse -o %s" % (name, ids, len(text), st["ctx_ct"]), flush=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
    json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    sizes = [(os.path.getsize(os.path.join(dp, f)), os.path.relpath(os.path.join(dp, f), OUT)) for dp, _, fs in os.walk(OUT) for f in fs]
    assert max(sizes)[0] <= 256 << 10, max(sizes)
    print("tests/golden/widek: %d files, %.1f KiB, largest %s" % (len(sizes), sum(s for s, _ in sizes) / 1024.0, max(sizes)))


if __name__ == "__main__":
    main()
