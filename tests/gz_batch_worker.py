"""mk_sketch_batch_begin_gz against mk_sketch_batch_begin on the same texts, array for array.  Imported by tests/test_gpu_gzfasta.py,
and run by it as a process of its own where the environment matters (MK_POISON is read once per process)."""
import gzip
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import util_inputs as ui  # noqa: E402


def fasta_texts():
    """five small FASTA texts, 2 KB to 200 KB: several records, CRLF, empty behind its header, no newline at the end, one contig"""
    rs = np.random.RandomState(911)
    one = ui.fasta_bytes([ui.rand_seq(rs, 200000)])
    several = ui.fasta_bytes([ui.rand_seq(rs, n) for n in (5000, 17, 30000, 1, 12000)], width=60)
    crlf = ui.fasta_bytes([ui.rand_seq(rs, 40000), ui.rand_seq(rs, 901)]).replace(b"\n", b"\r\n")
    empty = b">nothing behind this header\n"
    nonl = ui.fasta_bytes([ui.rand_seq(rs, 2000)]).rstrip(b"\n")
    return [one, several, crlf, empty, nonl]


def gz(text, level=6, name=""):
    b = io.BytesIO()
    with gzip.GzipFile(name, "wb", level, b, mtime=0) as g:
        g.write(text)
    return b.getvalue()


def same(a, b, label):
    assert len(a) == len(b), label
    for i, ((sa, aa, ca), (sb, ab, cb)) in enumerate(zip(a, b)):
        assert sa == sb == 0, "%s file %d: status %d / %d" % (label, i, sa, sb)
        assert aa == ab, "%s file %d: sketched alone %d / %d" % (label, i, aa, ab)
        assert len(ca) == len(cb)
        for k, (x, y) in enumerate(zip(ca, cb)):
            assert np.array_equal(x, y), "%s file %d component %d" % (label, i, k)


def check_parity(capi, shuf, tab_bits=0):
    texts = fasta_texts()
    gzs = [gz(t, lvl, nm) for t, lvl, nm in zip(texts, (6, 1, 9, 6, 6), ("", "a.fna", "", "", ""))]
    eng = capi.Engine(shuf, 0)
    try:
        if tab_bits:
            eng.set_option(capi.MK_OPT_BATCH_TAB_BITS, tab_bits)
        for mode in (capi.MK_MODE_SET, capi.MK_MODE_UNIQ_SET):
            eng.batch_begin(texts, mode)
            want = eng.batch_end()
            assert any(len(c) for _, _, comps in want for c in comps)
            if tab_bits:
                assert any(alone for _, alone, _ in want), "no file fell out of its batch: the 512-slot case tests nothing"
            for one_buffer in (False, True):
                eng.batch_begin_gz(gzs, mode, one_buffer=one_buffer)
                got = eng.batch_end()
                assert eng.batch_gz_status(len(gzs)) == [0] * len(gzs)
                same(got, want, "mode %d one_buffer %s" % (mode, one_buffer))
            # two batches in flight, a text batch between two gz batches of different sizes
            eng.batch_begin_gz(gzs[:2], mode)
            eng.batch_begin_gz(gzs[2:], mode, one_buffer=True)
            same(eng.batch_end(), want[:2], "first of two")
            eng.batch_begin(texts, mode)
            same(eng.batch_end(), want[2:], "second of two")
            assert eng.batch_gz_status(3) == [0, 0, 0]
            same(eng.batch_end(), want, "text batch behind them")
    finally:
        eng.close()


if __name__ == "__main__":
    from metakssd_amd import capi
    k, subk, drl, seed = (int(x) for x in sys.argv[1:5])
    check_parity(capi, capi.Shuf.generate(k, subk, drl, seed), int(sys.argv[5]))
    print("gz batch parity ok")
