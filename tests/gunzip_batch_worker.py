"""mk_sketch_batch_begin_gunzip (a gz batch inflated by many wavefronts per file) against mk_sketch_batch_begin on the same texts,
array for array, and its piece counts against tests/gunzip_model.py.  Imported by tests/test_gpu_gunzip_batch.py, and run by it as a
process of its own where the environment matters (MK_POISON is read once per process)."""
import functools
import gzip
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gunzip_model as gm  # noqa: E402
import gz_batch_worker as gw  # noqa: E402

SPAN, RATIO = 1024, 64
LEVELS = (6, 1, 9, 6, 6)


@functools.lru_cache(maxsize=None)
def genomes():
    """-> (texts, gzip files, the model's piece count per file)"""
    texts = gw.fasta_texts()
    gzs = [gw.gz(t, lvl, nm) for t, lvl, nm in zip(texts, LEVELS, ("", "a.fna", "", "", ""))]
    for i, mem in ((0, 1), (2, 2)):  # small blocks (zlib's memLevel): many block starts, many pieces
        c = zlib.compressobj(LEVELS[i], zlib.DEFLATED, 31, mem)
        gzs[i] = c.compress(texts[i]) + c.flush()
    counts = []
    for t, f in zip(texts, gzs):
        assert gzip.decompress(f) == t
        raw = f[f.index(b"\0", 10) + 1 if f[3] & 8 else 10:-8]
        st, text, pieces = gm.run(raw, SPAN, RATIO)
        assert st == gm.OK and text == t
        counts.append(len(pieces))
    assert max(counts) > 5 and min(counts) == 1
    return texts, gzs, counts


def check_parity(capi, shuf, tab_bits=0):
    texts, gzs, counts = genomes()
    opts = dict(span_bytes=SPAN, ratio=RATIO)
    eng = capi.Engine(shuf, 0)
    try:
        if tab_bits:
            eng.set_option(capi.MK_OPT_BATCH_TAB_BITS, tab_bits)
        for mode in (capi.MK_MODE_SET, capi.MK_MODE_UNIQ_SET):
            eng.batch_begin(texts, mode)
            want = eng.batch_end()
            assert eng.batch_gz_pieces(len(gzs)) == [0] * len(gzs)
            assert any(len(c) for _, _, comps in want for c in comps)
            if tab_bits:
                assert any(alone for _, alone, _ in want), "no file fell out of its batch: the 512-slot case tests nothing"
            for one_buffer in (False, True):
                eng.batch_begin_gz(gzs, mode, one_buffer=one_buffer, gunzip=opts)
                got = eng.batch_end()
                assert eng.batch_gz_status(len(gzs)) == [0] * len(gzs)
                assert eng.batch_gz_pieces(len(gzs)) == counts
                gw.same(got, want, "mode %d one_buffer %s" % (mode, one_buffer))
            # two batches in flight, one by each route
            eng.batch_begin_gz(gzs[:2], mode, gunzip=opts)
            eng.batch_begin_gz(gzs[2:], mode, one_buffer=True)
            gw.same(eng.batch_end(), want[:2], "first of two")
            assert eng.batch_gz_pieces(2) == counts[:2]
            eng.batch_begin_gz(gzs, mode, gunzip=opts)
            gw.same(eng.batch_end(), want[2:], "second of two")
            assert eng.batch_gz_pieces(3) == [0, 0, 0] and eng.batch_gz_status(3) == [0, 0, 0]
            gw.same(eng.batch_end(), want, "the same context again")
            assert eng.batch_gz_pieces(len(gzs)) == counts
    finally:
        eng.close()


if __name__ == "__main__":
    from metakssd_amd import capi
    k, subk, drl, seed = (int(x) for x in sys.argv[1:5])
    check_parity(capi, capi.Shuf.generate(k, subk, drl, seed), int(sys.argv[5]))
    print("gunzip batch parity ok")
