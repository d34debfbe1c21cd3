"""get_species_abundance() (command_composite.c:446-640) restated over in-memory arrays: the model that mk_composite and the
resident route of `composite -q` are held against.

A sketch directory is, per component c, combco.c (uint32 ids), combco.index.c (uint64 positions, one more than sketches) and -- for a
query made with -A -- combco.c.a (uint16 counts).  For every query sample and reference sketch the reference collects the sample's
counts of the k-mers the two share, over all components, and reports order statistics of them:

  * the sample's dictionary finds the FIRST occurrence of an id in the sample's slice (:538-546, :551-554): a later repeat of the id
    never counts, whatever its count;
  * every position of a reference sketch is looked up (:549): an id that occurs twice in a sketch contributes twice;
  * sketches with fewer than 6 shared k-mers are dropped (:600); the others come by decreasing number, ties by sketch number
    (glibc's merge-sort qsort, :584).
"""
import os
import struct

import numpy as np

MIN_KM_S = 6
ROW_FIELDS = ("ref", "kmer_num", "sum", "lastsum", "lastn", "median", "top")


def stats(ref, vals):
    """the integers of :599-613 for one reference sketch; vals = the shared k-mers' counts (any order)"""
    v = np.sort(np.asarray(vals, dtype=np.int64), kind="stable")
    k = int(v.size)
    s = int(v.sum()) & 0xFFFFFFFF
    s = s - (1 << 32) if s >= (1 << 31) else s      # int sum
    n = int(k * 0.98)                                # ST_PCTL, in double
    lastsum = lastn = 0
    while n <= k * 0.99:                             # ED_PCTL
        lastsum += int(v[n - 1])                     # the reference's array is 1-based
        lastn += 1
        n += 1
    return (int(ref), k, s, lastsum, lastn, int(v[k // 2 - 1]), int(v[k - 1]))


def rows_from_hits(refs, counts):
    """(reference sketch, count) pairs of one sample, all components -> its rows in print order"""
    refs = np.asarray(refs, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    if refs.size == 0:
        return []
    order = np.lexsort((counts, refs))
    refs, counts = refs[order], counts[order]
    heads = np.flatnonzero(np.concatenate([[True], refs[1:] != refs[:-1]]))
    ends = np.concatenate([heads[1:], [refs.size]])
    rows = [stats(refs[a], counts[a:b]) for a, b in zip(heads, ends) if b - a >= MIN_KM_S]
    rows.sort(key=lambda r: (-r[1], r[0]))
    return rows


def sample_hits(ref_ids, ref_index, q_ids, q_counts):
    """one component, one sample: (reference sketch, count) for every reference position whose id the sample holds"""
    ref_ids = np.asarray(ref_ids, dtype=np.uint32)
    ref_index = np.asarray(ref_index, dtype=np.uint64).astype(np.int64)
    q_ids = np.asarray(q_ids, dtype=np.uint32)
    q_counts = np.asarray(q_counts, dtype=np.uint16)
    if ref_ids.size == 0 or q_ids.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    uniq, first = np.unique(q_ids, return_index=True)      # return_index: the first occurrence
    at = np.searchsorted(uniq, ref_ids)
    at[at == uniq.size] = 0
    hit = uniq[at] == ref_ids
    sketch = np.repeat(np.arange(ref_index.size - 1, dtype=np.int64), np.diff(ref_index))
    return sketch[hit], q_counts[first[at[hit]]].astype(np.int64)


def composite_rows(ref_num, ref_comps, nsamples, qry_comps):
    """ref_comps: per component (ids, index[ref_num + 1]); qry_comps: per component (ids, counts, index[nsamples + 1]).
    -> per sample the list of rows (ref, kmer_num, sum, lastsum, lastn, median, top) in print order"""
    assert len(ref_comps) == len(qry_comps)
    out = []
    for s in range(nsamples):
        rr, cc = [], []
        for (rids, rindex), (qids, qcounts, qindex) in zip(ref_comps, qry_comps):
            assert len(rindex) == ref_num + 1 and len(qindex) == nsamples + 1
            a, b = int(qindex[s]), int(qindex[s + 1])
            r, c = sample_hits(rids, rindex, np.asarray(qids)[a:b], np.asarray(qcounts)[a:b])
            rr.append(r)
            cc.append(c)
        out.append(rows_from_hits(np.concatenate(rr) if rr else [], np.concatenate(cc) if cc else []))
    return out


# ---- sketch directories ------------------------------------------------------------------------------------------------------------
def read_stat(d):
    b = open(os.path.join(d, "cofiles.stat"), "rb").read()
    comp_num, infile_num = struct.unpack_from("<ii", b, 16)
    names = [b[32 + 4 * infile_num + 256 * i: 32 + 4 * infile_num + 256 * (i + 1)].split(b"\0", 1)[0].decode() for i in range(infile_num)]
    return comp_num, infile_num, names


def read_dir(d, counts=False):
    """-> (number of sketches, names, per component (ids, index) or (ids, counts, index))"""
    comp_num, n, names = read_stat(d)
    comps = []
    for c in range(comp_num):
        ids = np.fromfile(os.path.join(d, "combco.%d" % c), np.uint32)
        index = np.fromfile(os.path.join(d, "combco.index.%d" % c), np.uint64)[:n + 1]
        if counts:
            comps.append((ids, np.fromfile(os.path.join(d, "combco.%d.a" % c), np.uint16), index))
        else:
            comps.append((ids, index))
    return n, names, comps


def format_rows(qryname, refnames, rows):
    """the lines `composite -q` prints for one sample (:624): the two divisions are float divisions"""
    out = []
    for ref, k, s, lastsum, lastn, median, top in rows:
        mean = np.float32(s) / np.float32(k)
        last = np.float32(lastsum) / np.float32(lastn)
        out.append("%s\t%s\t%d\t%f\t%f\t%d\t%d" % (qryname, refnames[ref], k, float(mean), float(last), median, top))
    return out


def composite_dirs(refdir, qrydir):
    """the stdout lines of `composite -r refdir -q qrydir`"""
    ref_num, refnames, ref_comps = read_dir(refdir)
    nsamples, qrynames, qry_comps = read_dir(qrydir, counts=True)
    lines = []
    for s, rows in enumerate(composite_rows(ref_num, ref_comps, nsamples, qry_comps)):
        lines += format_rows(qrynames[s], refnames, rows)
    return lines


def build_marker_db(case, shuf_files, tmp_path, dist_cmd, set_cmd, query_files=None):
    """the README's MarkerDB recipe on a golden composite case (as tests/test_golden.py::run_composite_case): dist -> set -g -> set -q ->
    set -i, and the -A sketch directory of the query files (query_files: other FASTQ files than the case's own).
    -> (marker database, query sketch directory)"""
    import json
    import subprocess
    import golden_cases as gc
    entry = json.load(open(os.path.join(gc.GOLDEN, "manifest.json")))["composite_cases"][case]
    refs, qry = gc.build_composite_inputs(case, str(tmp_path))
    if query_files is not None:
        qry = list(query_files)
    sk, grp, uq, db, qsk = (str(tmp_path / n) for n in ("sk", "grp", "uq", "db", "qsk"))
    taxf = str(tmp_path / "tax.tsv")
    open(taxf, "w").write("".join(t + "\n" for t in entry["tax"]))
    for cmd in (dist_cmd + ["-L", shuf_files(entry["shuf"]), "-o", sk] + refs,
                set_cmd + ["-g", taxf, "-o", grp, sk], set_cmd + ["-q", "-o", uq, grp], set_cmd + ["-i", uq, "-o", db, grp],
                dist_cmd + ["-L", shuf_files(entry["shuf"]), "-A", "-o", qsk] + qry):
        r = subprocess.run(cmd, input=b"N\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (cmd, r.stderr.decode())
    return db, qsk


def strain_mix_fastq(path, seed, weights, nreads=1500):
    """metagenome-like reads as golden_cases' "mix": 150 bp reads of both strands from the golden strains sA / sB / sC, drawn with the
    given weights"""
    import golden_cases as gc
    import util_inputs as ui
    rs = np.random.RandomState(seed)
    genomes = [b"".join(gc._strain(n)) for n in ("sA", "sB", "sC")]
    w = np.asarray(weights, dtype=np.float64) / np.sum(weights)
    out = []
    for _ in range(nreads):
        g = genomes[int(rs.choice(3, p=w))]
        a = rs.randint(0, len(g) - 150)
        r = g[a:a + 150]
        out.append(ui.revcomp(r) if rs.rand() < 0.5 else r)
    open(path, "wb").write(ui.fastq_bytes(out))
    return path
