"""numpy restatement of `composite -i` / `composite -s` (index_abv() and abv_search(), command_composite.c:212-440) and
synthetic abundance-vector databases, for tests/test_gpu_abv.py and tools/bench_abv.py.

The arithmetic is the reference's, step by step in np.float32 (numpy does not fuse a multiply into an add): the search
loops over the query's entries d in file order and adds a column at a time with np.add.at, which applies repeated indices
one after the other, in float32.  Orders use kind="stable" sorts; a query with a NaN measure is ordered by a restatement of
glibc's merge sort (what the reference's qsort runs), because its comparator is then no strict order."""
import os
import struct

import numpy as np

BINVEC = np.dtype([("r", "<i4"), ("p", "<f4")])  # binVec_t, command_composite.h:12-16
METRIC_NAME = {0: "CosineXY", 1: "L1norm", 2: "L2norm"}


def write_db(root, nref, files):
    """<root>/cofiles.stat (infile_num = nref at offset 20) and <root>/abundance_Vec/<name> for (name, BINVEC array)"""
    os.makedirs(os.path.join(root, "abundance_Vec"), exist_ok=True)
    with open(os.path.join(root, "cofiles.stat"), "wb") as f:
        f.write(struct.pack("<IiiiiiQ", 0, 0, 0, 0, 1, nref, 0))
    for name, vec in files:
        with open(os.path.join(root, "abundance_Vec", name), "wb") as f:
            f.write(np.ascontiguousarray(vec, dtype=BINVEC).tobytes())


def random_vec(rs, nref, k, zero=False):
    """k distinct species of nref with positive float32 percentages summing to about 100 (as composite -b scales them)"""
    v = np.zeros(k, BINVEC)
    v["r"] = rs.choice(nref, size=k, replace=False)
    p = rs.gamma(0.7, 1.0, size=k) + 1e-3
    v["p"] = 0.0 if zero else (p * 100.0 / p.sum()).astype(np.float32)
    return v


def dir_order(root):
    """the file names the way readdir() lists them (what both programs index): os.listdir is readdir"""
    return [n for n in os.listdir(os.path.join(root, "abundance_Vec")) if "." in n and n.rsplit(".", 1)[1] == "abv"]


def read_vec(path):
    return np.fromfile(path, dtype=BINVEC)


def index_model(root, nref):
    """the four files of index_abv(): {name, yl2n, abm, abmi} -> bytes"""
    names = dir_order(root)
    vecs = [read_vec(os.path.join(root, "abundance_Vec", n)) for n in names]
    ent = np.concatenate(vecs) if vecs else np.zeros(0, BINVEC)
    fileno = np.repeat(np.arange(len(vecs), dtype=np.int32), [len(v) for v in vecs])
    order = np.argsort(ent["r"], kind="stable")
    abm = np.zeros(len(ent), BINVEC)
    abm["r"] = fileno[order]
    abm["p"] = ent["p"][order]
    abmi = np.cumsum(np.bincount(ent["r"], minlength=nref)[:nref]).astype(np.int32) if nref else np.zeros(0, np.int32)
    yl2n = np.zeros(len(vecs), np.float64)
    for i, v in enumerate(vecs):
        pp = (v["p"] * v["p"]).astype(np.float32).astype(np.float64)
        yl2n[i] = np.sqrt(np.cumsum(pp)[-1]) if len(pp) else 0.0  # cumsum: one add after the other (np.sum pairs them)
    return {"name": "".join(n + "\n" for n in names).encode(), "yl2n": yl2n.tobytes(), "abm": abm.tobytes(), "abmi": abmi.tobytes()}


def read_index(root):
    pre = os.path.join(root, "abundance_Vec")
    names = open(pre + ".name", "rb").read().decode().split("\n")[:-1]
    return names, np.fromfile(pre + ".yl2n", np.float64), np.fromfile(pre + ".abm", BINVEC), np.fromfile(pre + ".abmi", np.int32)


def _glibc_msort(idx, meas):
    """msort_with_tmp of glibc 2.35 with comparator_measure (:660-665): n1 = n / 2, a tie takes from the left"""
    def cmp(a, b):
        r = np.float32(meas[a] - meas[b])
        return 1 if r > 0 else (-1 if r < 0 else 0)

    def rec(b):
        n = len(b)
        if n <= 1:
            return b
        n1 = n // 2
        left, right = rec(b[:n1]), rec(b[n1:])
        out, i, j = [], 0, 0
        while i < len(left) and j < len(right):
            if cmp(left[i], right[j]) <= 0:
                out.append(left[i]); i += 1
            else:
                out.append(right[j]); j += 1
        return out + left[i:] + right[j:]
    return rec(list(idx))


def search_model(index, q, metric):
    """abv_search() for one query vector -> (sample ids in print order, float32 measures in that order)"""
    names, yl2n, abm, abmi = index
    S = len(names)
    m = np.zeros(S, np.float32)
    x = np.zeros(S, np.float32)
    y = np.zeros(S, np.float32)
    first = np.full(S, -1, np.int64)
    xl2n = np.float32(0)
    with np.errstate(all="ignore"):
        for d in range(len(q)):
            r, xp = int(q["r"][d]), np.float32(q["p"][d])
            xl2n = np.float32(xl2n + np.float32(xp * xp))
            lo, hi = (int(abmi[r - 1]) if r else 0), int(abmi[r])
            cs, cp = abm["r"][lo:hi], abm["p"][lo:hi]
            fresh = cs[first[cs] < 0]
            first[fresh] = d
            if metric == 1:
                np.add.at(m, cs, np.abs(cp - xp).astype(np.float32))
                np.add.at(x, cs, np.full(len(cs), xp, np.float32))
                np.add.at(y, cs, cp)
            elif metric == 2:
                dd = (cp - xp).astype(np.float32)
                np.add.at(m, cs, (dd * dd).astype(np.float32))
            else:
                np.add.at(m, cs, (cp * xp).astype(np.float32))
        hit = np.nonzero(first >= 0)[0]
        if metric == 1:
            v = (m[hit] + ((np.float32(200.0) - x[hit]) - y[hit])).astype(np.float32)
        elif metric == 2:
            v = m[hit]
        else:
            v = (m[hit].astype(np.float64) / (np.sqrt(np.float64(xl2n)) * yl2n[hit])).astype(np.float32)
    disc = hit[np.lexsort((hit, first[hit]))]  # discovery order: first entry, then sample
    meas = dict(zip(hit.tolist(), v.tolist()))
    mv = np.array([meas[s] for s in disc], np.float32)
    if np.isnan(mv).any():
        order = [disc[i] for i in _glibc_msort(range(len(disc)), mv)]
    else:
        order = disc[np.argsort(mv + np.float32(0.0), kind="stable")].tolist()  # + 0: -0 and +0 compare equal
    if metric == 0:
        order = order[::-1]
    return np.array(order, np.int64), np.array([meas[s] for s in order], np.float32)


def fmt_value(v):
    """printf("%lf") of the double the reference prints; glibc writes a NaN with its sign bit as -nan"""
    if np.isnan(v):
        return "-nan" if np.signbit(v) else "nan"
    return "%f" % v


def search_stdout(index, queries, metric):
    """stdout of `composite -r <ref> -s <metric> <queries...>`: queries = list of (argument, BINVEC array or None = skipped)"""
    names = index[0]
    out = []
    for i, (arg, q) in enumerate(queries):
        if q is None:
            out.append("%dth argument %s is not a .abv file, skipped\n" % (i, arg))
            continue
        ids, mv = search_model(index, q, metric)
        out.append("#Sample\t%s\n" % METRIC_NAME[metric])
        for s, v in zip(ids.tolist(), mv.tolist()):
            val = np.sqrt(np.float64(v)) if metric == 2 else np.float64(np.float32(v))
            out.append("%s\t%s\n" % (names[s], fmt_value(np.float64(val))))
    return "".join(out)
