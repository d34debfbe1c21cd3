#!/usr/bin/env python3
"""tests/golden/make_golden_abv.py -- the golden data of `composite -i` / `composite -s`, made by the REAL reference.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`).  Writes a small
fixed database (seeded numpy: 60 sample vectors over 200 species, with two copies of one file, a species listed twice,
an empty and an all-zero vector), lets the reference index it (`composite -r db -i`) and search it with the committed query
vectors (`composite -r db -s 0|1|2 q*.abv`), and keeps under tests/golden/abv/:
  abundance_Vec.{name,yl2n,abm,abmi}   the reference's index files
  q*.abv                               the query vectors
  search_s{0,1,2}.txt                  the reference's stdout per metric
The sample vectors themselves are not kept: the test searches the reference's index, so readdir order does not matter.
Nothing here is reference source: the outputs are data produced by executing the reference.
"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import abv_model as am  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
OUT = os.path.join(HERE, "abv")


def main():
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/metakssd is missing: make -C oracle ref")
    rs = np.random.RandomState(2024)
    nref = 200
    files = [("sample%02d.abv" % i, am.random_vec(rs, nref, int(rs.randint(1, 40)))) for i in range(60)]
    files.append(("twinA.abv", files[5][1]))
    files.append(("twinB.abv", files[5][1]))
    rep = am.random_vec(rs, nref, 10)
    files.append(("repeat.abv", np.concatenate([rep, rep[:2]])))
    files.append(("empty.abv", np.zeros(0, am.BINVEC)))
    files.append(("allzero.abv", am.random_vec(rs, nref, 8, zero=True)))
    queries = [am.random_vec(rs, nref, 30), files[5][1], np.concatenate([rep, rep[:2]]), am.random_vec(rs, nref, 6, zero=True),
               am.random_vec(rs, nref, 120)]
    tmp = tempfile.mkdtemp()
    try:
        db = os.path.join(tmp, "db")
        am.write_db(db, nref, files)
        subprocess.check_call([REF, "composite", "-r", db, "-i"], stdout=subprocess.DEVNULL)
        shutil.rmtree(OUT, ignore_errors=True)
        os.makedirs(OUT)
        for s in ("name", "yl2n", "abm", "abmi"):
            shutil.copy(os.path.join(db, "abundance_Vec." + s), OUT)
        args = []
        for i, q in enumerate(queries):
            p = os.path.join(OUT, "q%d.abv" % i)
            q.tofile(p)
            args.append(p)
        for metric in (0, 1, 2):
            out = subprocess.check_output([REF, "composite", "-r", db, "-s", str(metric)] + args)
            open(os.path.join(OUT, "search_s%d.txt" % metric), "wb").write(out)
    finally:
        shutil.rmtree(tmp)
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
