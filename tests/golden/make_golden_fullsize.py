#!/usr/bin/env python3
"""tests/golden/make_golden_fullsize.py -- the reference's own sketches of the bench workload at full size, kept as digests.

Runs only where oracle/_ref/metakssd exists (compiled from the reference's sources by `make -C oracle ref`); CPU only.  For every
entry of ENTRIES the compiled reference sketches a prefix of the bench's read stream (seed 20261002, 150 bp) at `-p 1` -- the only
thread count at which its slot order, and with it the bytes of combco.0 / combco.0.a, are reproducible:

    oracle/_ref/metakssd dist -L <shuf> -A -p 1 -P "<python> gen.py" -o out x.fq

No FASTQ file is written: the reference popen()s "<pipecmd> <file>", and gen.py ignores the one-record placeholder x.fq and
streams mk_synth_fastq_write("/dev/stdout", seed, 0, N, 150) instead (config 4 would be 159 GB on disk).  The .shuf tables come
from the product's seeded generator and must have the sha256 tests/golden/manifest.json records.

Writes tests/golden/fullsize_digests.json: per entry the input's description, keys / sum_counts / max_count, sha256 of the two files,
sha256(ids || counts) (bench.py's sketch_digest) and multiset_sha256 = sha256 of sort(id << 16 | count) as little-endian u64, which
tells a difference of CONTENT from one of ORDER.  It does not touch manifest.json.  Nothing here is reference source: the file
holds numbers and hex digests produced by executing the reference.

    python tests/golden/make_golden_fullsize.py [--jobs 4] [--only NAME ...]

Entries run `--jobs` at a time, longest first (each is two single-threaded processes: the generator and the reference; config 4
takes about 40 minutes, config 3 about 4).  With --only the other entries are taken over from the existing file.  When every result
equals what the existing file holds, the file is left as it is (the wall times in it are those of the run that made it).
"""
import argparse
import concurrent.futures
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from conftest import SHUF_SPECS  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")
OUT = os.path.join(HERE, "fullsize_digests.json")
SEED, READ_LEN = 20261002, 150

# name -> (shuf, reads); every L3K11 entry is a prefix of config 4's stream
ENTRIES = {
    "L3K11_1M": ("L3K11", 1_000_000),
    "L3K11_4M": ("L3K11", 4_000_000),
    "L3K11_16M": ("L3K11", 16_000_000),
    "config3": ("L3K11", 50_000_000),
    "config4": ("L3K11", 500_000_000),
    # config 4's collision regime in the 2 097 143-slot table: N chosen so that the REFERENCE's key count is 0.40..0.50 of the
    # slots (131 windows a read, 1/4096 accepted), under its own abort limit of 0.6
    "L3K10_dense": ("L3K10", 30_000_000),
}
DENSE_LOAD = (0.40, 0.50)

GEN = """import ctypes, sys
lib = ctypes.CDLL(%r)
lib.mk_synth_fastq_write.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
sys.exit(lib.mk_synth_fastq_write(b"/dev/stdout", %d, 0, %d, %d))
"""


def digests(ids, cnt):
    key = (ids.astype(np.uint64) << np.uint64(16)) | cnt.astype(np.uint64)
    key.sort()
    return {"keys": int(ids.size), "sum_counts": int(cnt.astype(np.int64).sum()), "max_count": int(cnt.max()) if cnt.size else 0,
            "combco_sha256": hashlib.sha256(ids.tobytes()).hexdigest(), "combco_a_sha256": hashlib.sha256(cnt.tobytes()).hexdigest(),
            "sketch_sha256": hashlib.sha256(ids.tobytes() + cnt.tobytes()).hexdigest(),
            "multiset_sha256": hashlib.sha256(key.astype("<u8").tobytes()).hexdigest()}


def run_entry(name, shuf_path, shuf_sha, slots, work):
    shuf, n = ENTRIES[name]
    d = os.path.join(work, name)
    os.makedirs(d)
    gen = os.path.join(d, "gen.py")
    open(gen, "w").write(GEN % (os.path.join(ROOT, "metakssd_amd", "lib", "libmetakssd_hip.so"), SEED, n, READ_LEN))
    open(os.path.join(d, "x.fq"), "w").write("@placeholder\nACGT\n+\nIIII\n")
    flags = ["-A", "-p", "1"]
    t0 = time.perf_counter()
    r = subprocess.run([REF, "dist", "-L", shuf_path] + flags + ["-P", "%s %s" % (sys.executable, gen), "-o", "out", "x.fq"], cwd=d,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    wall = time.perf_counter() - t0
    out = os.path.join(d, "out")
    if r.returncode != 0 or not os.path.exists(os.path.join(out, "cofiles.stat")):
        raise SystemExit("%s: the reference failed (rc %d): %s" % (name, r.returncode, r.stderr.decode(errors="replace")[-400:]))
    assert not os.path.exists(os.path.join(out, "combco.1")), "one component expected"
    ids = np.fromfile(os.path.join(out, "combco.0"), dtype=np.uint32)
    cnt = np.fromfile(os.path.join(out, "combco.0.a"), dtype=np.uint16)
    assert ids.size == cnt.size
    e = {"shuf": shuf, "shuf_spec": list(SHUF_SPECS[shuf]), "shuf_sha256": shuf_sha, "slots": slots, "seed": SEED, "reads": n,
         "read_len": READ_LEN, "flags": flags}
    e.update(digests(ids, cnt))
    e["load"] = round(ids.size / slots, 6)
    e["reference_wall_s"] = round(wall, 1)
    shutil.rmtree(d, ignore_errors=True)
    if name == "L3K10_dense" and not DENSE_LOAD[0] <= ids.size / slots <= DENSE_LOAD[1]:
        raise SystemExit("L3K10_dense: load %.3f is outside %r: choose another N" % (ids.size / slots, DENSE_LOAD))
    print("%-12s N=%-10d keys=%-9d load=%.4f sketch=%s  (%.1f s)" % (name, n, e["keys"], e["load"], e["sketch_sha256"][:16], wall), flush=True)
    return name, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    if not os.path.exists(REF):
        sys.exit("oracle/_ref/metakssd is missing: make -C oracle ref")
    from metakssd_amd import capi
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))
    old = json.load(open(OUT)) if os.path.exists(OUT) else None
    names = list(ENTRIES) if a.only is None else a.only
    for nm in names:
        if nm not in ENTRIES:
            sys.exit("unknown entry %s" % nm)
    if a.only is not None and (old is None or set(ENTRIES) - set(names) - set(old["entries"])):
        sys.exit("--only needs the other entries in the existing file")
    work = tempfile.mkdtemp(prefix="golden_full_")
    try:
        shufs = {}
        for s in sorted({ENTRIES[nm][0] for nm in names}):
            p = os.path.join(work, s + ".shuf")
            sh = capi.Shuf.generate(*SHUF_SPECS[s])
            sh.write(p)
            sha = hashlib.sha256(open(p, "rb").read()).hexdigest()
            if sha != manifest["shufs"][s]["sha256"]:
                sys.exit("%s.shuf: sha256 %s is not the one manifest.json records: the table generator changed" % (s, sha))
            shufs[s] = (p, sha, int(sh.params().hashsize))
        got = {}
        with concurrent.futures.ThreadPoolExecutor(max(1, a.jobs)) as ex:
            futs = [ex.submit(run_entry, nm, *shufs[ENTRIES[nm][0]], work) for nm in sorted(names, key=lambda x: -ENTRIES[x][1])]
            for f in futs:
                nm, e = f.result()
                got[nm] = e
    finally:
        shutil.rmtree(work, ignore_errors=True)
    entries = {}
    for nm in ENTRIES:
        entries[nm] = got[nm] if nm in got else old["entries"][nm]
    strip = lambda e: {k: v for k, v in e.items() if k != "reference_wall_s"}  # noqa: E731
    if old is not None and {k: strip(v) for k, v in old["entries"].items()} == {k: strip(v) for k, v in entries.items()}:
        print("every result equals %s: file left as it is" % os.path.relpath(OUT, ROOT))
        return
    if old is not None:
        for nm in got:
            if nm in old["entries"] and strip(old["entries"][nm]) != strip(got[nm]):
                print("NOTE: %s differs from the existing file" % nm)
    doc = {"what": "the compiled reference's `dist -A -p 1` sketches of the bench read stream; made by tests/golden/make_golden_fullsize.py",
           "sketch_sha256": "sha256(combco.0 bytes || combco.0.a bytes)",
           "multiset_sha256": "sha256 of sort(id << 16 | count) as little-endian u64",
           "host_cores": os.cpu_count(), "jobs": a.jobs, "entries": entries}
    json.dump(doc, open(OUT, "w"), indent=1, sort_keys=True)
    open(OUT, "a").write("\n")
    print("wrote %s (%d bytes)" % (os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
