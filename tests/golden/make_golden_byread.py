#!/usr/bin/env python3
"""tests/golden/make_golden_byread.py -- the golden data of `dist --byread`, `reverse -b` and `reverse`, made by the REAL reference.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`).  For every case of
CASES it runs `metakssd dist -L <shuf> --byread -o out <input>` and `metakssd reverse -L <shuf> -b out`, and keeps under
tests/golden/byread/<case>/ the combco.<c> and combco.index.<c> files and the reference's stdout (reverse_b.txt.gz: the text is
gzip-compressed so that every committed file stays below 256 KiB).  For plain `reverse` it lays out a sketch directory of three
inputs in a fixed order with oracle/kssd_oracle_cli (the reference's dist shuffles its inputs by the clock), one of them with no
ids at all, gives the last recorded path a space (cofiles.stat is patched: the oracle reads its inputs through a shell), runs
`metakssd reverse -L <shuf> -o outdir <dir>` and keeps the directory's combco files and the recovered k-mer files (gzip).  manifest.json holds the header fields of every cofiles.stat, the recorded names and the sha256 of
every fixture.  synthetic.fa is byread_model.synthetic_text().
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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import byread_model as bm  # noqa: E402
from golden_cases import make_shuf  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
ORA = os.path.join(ROOT, "oracle", "kssd_oracle_cli")
OUT = os.path.join(HERE, "byread")

# case -> (input under tests/golden/inputs or "synthetic", name of the plain file the commands see, .shuf)
CASES = {
    "fa_sA_L3K10": ("fa_sA.fa.gz", "fa_sA.fa", "L3K10"),
    "fa_sA_L2K11": ("fa_sA.fa.gz", "fa_sA.fa", "L2K11"),
    "fa_genome_L1K7": ("fa_genome.fa.gz", "fa_genome.fa", "L1K7"),
    "fa_genome_L0K6": ("fa_genome.fa.gz", "fa_genome.fa", "L0K6"),
    "fq_mix_L1K7": ("fq_mix.fq.gz", "fq_mix.fq", "L1K7"),
    "synthetic_L1K7": ("synthetic", "synthetic.fa", "L1K7"),
    "synthetic_L0K6": ("synthetic", "synthetic.fa", "L0K6"),
}
# plain reverse: case -> (.shuf, inputs in directory order)
REVERSE_CASES = {
    "reverse_L1K7": ("L1K7", ["fa_sA.fa", "tiny.fa", "fa_genome.fa"]),
    "reverse_L2K11": ("L2K11", ["fa_sA.fa", "tiny.fa", "fa_genome.fa"]),
}
TINY = b">tiny\nACGTAC\n"  # shorter than any 2k: a sketch without ids, for which `reverse` writes no file


def sha(p):
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


def plain_input(work, src, name):
    p = os.path.join(work, name)
    if not os.path.exists(p):
        if src == "synthetic":
            data = bm.synthetic_text()
        elif src == "tiny":
            data = TINY
        else:
            data = gzip.open(os.path.join(HERE, "inputs", src)).read()
        open(p, "wb").write(data)
    return p


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise SystemExit("failed: %s\n%s" % (" ".join(cmd), r.stderr.decode(errors="replace")[-400:]))
    return r.stdout


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/metakssd is missing: make -C oracle ref")
    work = tempfile.mkdtemp(prefix="golden_byread_")
    manifest = {"cases": {}, "reverse_cases": {}}
    try:
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        open(os.path.join(OUT, "synthetic.fa"), "wb").write(bm.synthetic_text())
        shufs = {}
        for name in sorted({c[2] for c in CASES.values()} | {c[0] for c in REVERSE_CASES.values()}):
            shufs[name] = os.path.join(work, name + ".shuf")
            make_shuf(name, shufs[name])
        for case, (src, fname, shuf) in CASES.items():
            inp = plain_input(work, src, fname)
            out = os.path.join(work, case + ".out")
            run([REF, "dist", "-L", shufs[shuf], "--byread", "-p", "1", "-o", out, inp], work)
            again = os.path.join(work, case + ".again")
            run([REF, "dist", "-L", shufs[shuf], "--byread", "-p", "1", "-o", again, inp], work)
            text = run([REF, "reverse", "-L", shufs[shuf], "-b", out], work)
            d = os.path.join(OUT, case)
            os.makedirs(d)
            for f in sorted(os.listdir(out)):
                if f.startswith("combco"):
                    assert open(os.path.join(out, f), "rb").read() == open(os.path.join(again, f), "rb").read(), (case, f)
                    shutil.copy(os.path.join(out, f), os.path.join(d, f))
            with gzip.GzipFile(os.path.join(d, "reverse_b.txt.gz"), "wb", mtime=0) as g:
                g.write(text)
            st = bm.parse_stat(os.path.join(out, "cofiles.stat"))
            manifest["cases"][case] = {
                "input": src, "name": fname, "shuf": shuf, "shuf_sha256": sha(shufs[shuf]),
                "header": {k: st[k] for k in ("shuf_id", "koc", "kmerlen", "dim_rd_len", "comp_num", "infile_num", "all_ctx_ct")},
                "recorded_name": os.path.basename(st["names"][0]),
                "ids": sum(os.path.getsize(os.path.join(d, f)) // 4 for f in os.listdir(d) if f.startswith("combco.") and ".index." not in f),
                "records": os.path.getsize(os.path.join(d, "combco.index.0")) // 8 - 1,
                "reverse_b_sha256": hashlib.sha256(text).hexdigest(),
                "files": {f: sha(os.path.join(d, f)) for f in sorted(os.listdir(d))}}
            print("%-18s ids=%-6d records=%-4d reverse -b: %d bytes" % (case, manifest["cases"][case]["ids"],
                                                                      manifest["cases"][case]["records"], len(text)))
        for case, (shuf, names) in REVERSE_CASES.items():
            inputs = [plain_input(work, "tiny" if n.startswith("tiny") else n + ".gz", n) for n in names]
            sk, rv = os.path.join(work, case + ".sk"), os.path.join(work, case + ".rv")
            run([ORA, "-L", shufs[shuf], "-o", sk] + inputs, work)
            stp = os.path.join(sk, "cofiles.stat")
            b = bytearray(open(stp, "rb").read())
            o = 32 + 4 * len(names) + bm.PATHLEN * (len(names) - 1)
            old = b[o:o + bm.PATHLEN].split(b"\0", 1)[0]
            new = old.replace(b"fa_genome.fa", b"fa genome.fa")  # the file name `reverse` writes has '_' for ' '
            assert new != old
            b[o:o + len(new)] = new
            open(stp, "wb").write(bytes(b))
            os.makedirs(rv)
            run([REF, "reverse", "-L", shufs[shuf], "-o", rv, "-p", "1", sk], work)
            d = os.path.join(OUT, case)
            os.makedirs(os.path.join(d, "sketch"))
            os.makedirs(os.path.join(d, "kmers"))
            for f in sorted(os.listdir(sk)):
                if f.startswith("combco"):
                    shutil.copy(os.path.join(sk, f), os.path.join(d, "sketch", f))
            for f in sorted(os.listdir(rv)):
                with gzip.GzipFile(os.path.join(d, "kmers", f + ".gz"), "wb", mtime=0) as g:
                    g.write(open(os.path.join(rv, f), "rb").read())
            st = bm.parse_stat(os.path.join(sk, "cofiles.stat"))
            manifest["reverse_cases"][case] = {
                "shuf": shuf, "shuf_sha256": sha(shufs[shuf]), "inputs": names,
                "header": {k: st[k] for k in ("shuf_id", "koc", "kmerlen", "dim_rd_len", "comp_num", "infile_num", "all_ctx_ct")},
                "ctx_ct": st["ctx_ct"], "names": [os.path.basename(n) for n in st["names"]],
                "outputs": {f: sha(os.path.join(rv, f)) for f in sorted(os.listdir(rv))},
                "files": {os.path.relpath(os.path.join(dp, f), d): sha(os.path.join(dp, f)) for dp, _, fs in os.walk(d) for f in sorted(fs)}}
            print("%-18s ctx_ct=%s outputs=%s" % (case, st["ctx_ct"], sorted(os.listdir(rv))))
        json.dump(manifest, open(os.path.join(OUT, "manifest.json"), "w"), indent=1, sort_keys=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    sizes = [(os.path.getsize(os.path.join(dp, f)), os.path.relpath(os.path.join(dp, f), OUT)) for dp, _, fs in os.walk(OUT) for f in fs]
    assert max(sizes)[0] <= 256 << 10, max(sizes)
    assert sum(s for s, _ in sizes) < 1 << 20, sum(s for s, _ in sizes)
    print("tests/golden/byread: %d files, %.1f KiB, largest %s" % (len(sizes), sum(s for s, _ in sizes) / 1024.0, max(sizes)))


if __name__ == "__main__":
    main()
