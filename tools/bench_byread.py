#!/usr/bin/env python3
"""tools/bench_byread.py -- `dist --byread`, `reverse -b` and `reverse` on seeded synthetic inputs; prints one JSON line.

  byread   a seeded synthetic FASTA (default about 1 GB: contigs of 4 Mbases in lines of 80) at L3K10 and at L0K6 (every window
           is emitted: the worst case): wall time of `metakssd dist --byread`, the kernels' time (HIP events of the handle,
           through the library on the same text), and the compiled reference's wall time on the same file
  reverse_b  `reverse -b` of the by-read directory at L3K10 (and at L0K6 with --reverse-l0), product and reference
  reverse  `reverse` of a one-sketch directory of --keys random ids (default 1 573 525, the key count of the config-3 sketch)
Outputs are compared by sha256; oracle/_ref/metakssd is used where it exists, otherwise the reference fields are null."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from golden_cases import make_shuf  # noqa: E402
from metakssd_amd import capi  # noqa: E402

CLI = os.path.join(ROOT, "metakssd_amd", "bin", "metakssd")
REF = os.path.join(ROOT, "oracle", "_ref", "metakssd")


def timed(cmd, out_path=None):
    t0 = time.perf_counter()
    with open(out_path or os.devnull, "wb") as f:
        r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, timeout=3000)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (cmd[:4], r.stderr.decode(errors="replace")[-500:]))
    return round(dt, 4)


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def dir_sha(d):
    return {f: sha(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.startswith("combco")}


def write_fasta(path, nbytes, seed):
    """contigs of 4 Mbases in lines of 80, about nbytes in all"""
    rs = np.random.RandomState(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(path, "wb") as f:
        done, i = 0, 0
        while done < nbytes:
            n = min(4 << 20, max(nbytes - done, 1000))
            a = letters[rs.randint(0, 4, size=(n + 79) // 80 * 80)].reshape(-1, 80)
            body = np.concatenate([a, np.full((a.shape[0], 1), 10, np.uint8)], axis=1).tobytes()
            f.write(b">contig%d\n" % i + body)
            done += len(body)
            i += 1
    return os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=1000, help="size of the synthetic FASTA in MB")
    ap.add_argument("--keys", type=int, default=1573525)
    ap.add_argument("--reverse-l0", action="store_true", help="also reverse -b the L0K6 directory (13 bytes of text per input base)")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("bench_byread: no HIP device")
    have_ref = os.path.exists(REF) and not a.no_ref
    work = tempfile.mkdtemp(dir=a.workdir)
    res = {"what": "dist --byread / reverse", "fasta_mb": a.mb, "reference": have_ref}
    try:
        fa = os.path.join(work, "synth.fa")
        res["fasta_bytes"] = write_fasta(fa, a.mb * 1000000, 1)
        text = open(fa, "rb").read()
        for name in ("L3K10", "L0K6"):
            shuf = os.path.join(work, name + ".shuf")
            make_shuf(name, shuf)
            e = {}
            out = os.path.join(work, name + ".mine")
            timed([CLI, "dist", "-L", shuf, "--byread", "--quiet", "-o", out, fa])  # warm-up: page cache, code objects
            e["cli_wall_s"] = timed([CLI, "dist", "-L", shuf, "--byread", "--quiet", "-o", out, fa])
            e["ids"] = sum(os.path.getsize(os.path.join(out, f)) // 4 for f in os.listdir(out) if f.startswith("combco.") and ".index." not in f)
            h = capi.ByRead(capi.Shuf.read(shuf), 0)
            t0 = time.perf_counter()
            h.begin()
            step = capi.MK_BYREAD_MAX_PUSH
            for o in range(0, len(text), step):
                h.push_text(text[o:o + step], final=o + step >= len(text))
                for c in range(h.params.component_num):
                    h._ids[c].clear()
                    h._index[c].clear()
            e["library_wall_s"] = round(time.perf_counter() - t0, 4)
            e["kernel_ms"] = round(h.last_kernel_ms()[0], 3)
            h.close()
            # the kernels read the text twice (summary, emit), write and read the stream three times (emit, count, write) and write
            # 8 bytes per id (id + record) before 4 of them go back to the host
            byts = 2 * len(text) + 3 * len(text) + 12 * e["ids"]
            e["kernel_bytes"] = byts
            e["hbm_roofline_ms"] = round(byts / 8e12 * 1e3, 3)
            if have_ref:
                ro = os.path.join(work, name + ".ref")
                e["ref_wall_s"] = timed([REF, "dist", "-L", shuf, "--byread", "-p", "1", "-o", ro, fa])
                e["output_equals_reference"] = dir_sha(out) == dir_sha(ro)
            else:
                e["ref_wall_s"] = e["output_equals_reference"] = None
            res["byread_" + name] = e
            if name == "L3K10" or a.reverse_l0:
                r = {}
                po = os.path.join(work, "rb_mine.txt")
                timed([CLI, "reverse", "-L", shuf, "-b", out], po)
                r["cli_wall_s"] = timed([CLI, "reverse", "-L", shuf, "-b", out], po)
                r["stdout_bytes"] = os.path.getsize(po)
                if have_ref:
                    rp = os.path.join(work, "rb_ref.txt")
                    r["ref_wall_s"] = timed([REF, "reverse", "-L", shuf, "-b", ro], rp)
                    r["output_equals_reference"] = sha(po) == sha(rp)
                    os.remove(rp)
                else:
                    r["ref_wall_s"] = r["output_equals_reference"] = None
                os.remove(po)
                res["reverse_b_" + name] = r
            shutil.rmtree(out, ignore_errors=True)
            if have_ref:
                shutil.rmtree(ro, ignore_errors=True)
        del text
        # plain reverse: one sketch of --keys distinct ids at L3K11 (the config-3 geometry: 22-mers, one component)
        shuf = os.path.join(work, "L3K11.shuf")
        make_shuf("L3K11", shuf)
        s = capi.Shuf.read(shuf)
        rs = np.random.RandomState(3)
        ids = np.unique(rs.randint(0, 1 << 32, size=a.keys + a.keys // 8, dtype=np.int64).astype(np.uint32))[:a.keys]
        ids = rs.permutation(ids)
        sk = os.path.join(work, "sk")
        os.makedirs(sk)
        ids.tofile(os.path.join(sk, "combco.0"))
        np.array([0, ids.size], np.uint64).tofile(os.path.join(sk, "combco.index.0"))
        name = os.fsencode(os.path.join(work, "config3.fq"))
        with open(os.path.join(sk, "cofiles.stat"), "wb") as f:
            f.write(struct.pack("<IB3xiiiiQ", s.c.id & 0xFFFFFFFF, 0, 22, 6, 1, 1, ids.size) + struct.pack("<I", ids.size) + name + b"\0" * (256 - len(name)))
        r = {"keys": int(ids.size)}
        mo = os.path.join(work, "kmers_mine")
        os.makedirs(mo)
        timed([CLI, "reverse", "-L", shuf, "-o", mo, sk])
        r["cli_wall_s"] = timed([CLI, "reverse", "-L", shuf, "-o", mo, sk])
        r["text_bytes"] = os.path.getsize(os.path.join(mo, "config3.fq"))
        h = capi.ByRead(s, 0)
        h.reverse_ids(ids, 0)
        before = h.last_kernel_ms()[1]
        h.reverse_ids(ids, 0)
        r["kernel_ms"] = round(h.last_kernel_ms()[1] - before, 4)
        r["kernel_bytes"] = int(ids.size) * (4 + 23)
        r["hbm_roofline_ms"] = round(r["kernel_bytes"] / 8e12 * 1e3, 5)
        h.close()
        if have_ref:
            ro = os.path.join(work, "kmers_ref")
            os.makedirs(ro)
            r["ref_wall_s"] = timed([REF, "reverse", "-L", shuf, "-o", ro, "-p", "1", sk])
            r["output_equals_reference"] = sha(os.path.join(mo, "config3.fq")) == sha(os.path.join(ro, "config3.fq"))
        else:
            r["ref_wall_s"] = r["output_equals_reference"] = None
        res["reverse"] = r
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
