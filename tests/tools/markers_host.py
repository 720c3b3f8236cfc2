"""Host restatement of Seqwin's per-subgraph marker step (markers.py: ConnectedKmers.__get_loc and __get_rep_order semantics),
in numpy and plain Python, without pandas.

Written independently of the reference, as the oracle of tests/test_gpu_markers.py and tests/tools/marker_locs_time.py; the
goldens under tests/golden/markers/ (recorded from the reference itself) pin it.  Per subgraph, on the kept index:
  items   all occurrences of its nodes, ordered by (global record_idx, pos);
  runs    a new run at the first item, at every change of record, and where 2 * (pos - prev_pos) > 3 * w;
  rows    per assembly with an item: the run with the most items (the earliest on ties), the number of runs, start = first pos,
          stop = last pos + k (uint32), local record_idx, the hashes of the run in order;
  vote    over target rows (assembly < n_tar): c = count per ordering in order of first appearance, cc = count per canonical
          ordering (the smaller of t and t[::-1]) in order of first appearance while walking c, the first key of cc maximising
          len * cc, the more common orientation of it (the canonical one on ties), n_rep = cc of it, flags single / dup, and the
          lowest-assembly row with that ordering.
"""
from __future__ import annotations

import numpy as np

ROW_DTYPE = np.dtype([("assembly_idx", "<u4"), ("record_idx", "<u4"), ("start", "<u4"), ("stop", "<u4"), ("n_kmers", "<u4"),
                      ("n_repeats", "<u4")])
REP_DTYPE = np.dtype(ROW_DTYPE.descr + [("n_rep", "<u4"), ("flags", "<u4")])
SINGLE, DUP, NO_TARGET = 1, 2, 4


def loc(kmers, nodes, node_idx, record_offsets, kmerlen: int, windowsize: int):
    """(rows[ROW_DTYPE], list of hash tuples) of one subgraph given as indices into ``nodes``."""
    ro = np.asarray(record_offsets, np.int64)
    node_idx = np.asarray(node_idx, np.int64)
    st = nodes["start"][node_idx].astype(np.int64)
    ln = nodes["stop"][node_idx].astype(np.int64) - st
    if ln.sum() == 0:
        return np.zeros(0, ROW_DTYPE), []
    which = np.repeat(np.arange(len(node_idx)), ln)
    at = np.repeat(st, ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    rec = kmers["record_idx"][at].astype(np.int64)
    pos = kmers["pos"][at].astype(np.int64)
    h = nodes["hash"][node_idx][which]
    o = np.lexsort((pos, rec))
    rec, pos, h = rec[o], pos[o], h[o]
    new = np.ones(len(rec), bool)
    new[1:] = (rec[1:] != rec[:-1]) | (2 * (pos[1:] - pos[:-1]) > 3 * int(windowsize))
    starts = np.flatnonzero(new)
    ends = np.append(starts[1:], len(rec))
    asm = np.searchsorted(ro, rec[starts], side="right") - 1
    rows, seqs = [], []
    for a in np.unique(asm):
        runs = np.flatnonzero(asm == a)
        best = runs[np.argmax(ends[runs] - starts[runs])]   # the first of the largest
        i, j = int(starts[best]), int(ends[best])
        rows.append((a, rec[i] - ro[a], pos[i], (pos[j - 1] + int(kmerlen)) & 0xFFFFFFFF, j - i, len(runs)))
        seqs.append(tuple(int(x) for x in h[i:j]))
    return np.array(rows, ROW_DTYPE), seqs


def rep_order(rows, seqs, n_tar: int):
    """(index of the representative row, n_rep, flags), or None when no target assembly has a row."""
    tar = [t for r, t in zip(rows, seqs) if r["assembly_idx"] < n_tar]
    if not tar:
        return None
    c = {}
    for t in tar:
        c[t] = c.get(t, 0) + 1
    cc = {}
    for t, n in c.items():
        key = min(t, t[::-1])
        cc[key] = cc.get(key, 0) + n
    best = None
    for key, n in cc.items():
        if best is None or len(key) * n > len(best) * cc[best]:
            best = key
    rev = best[::-1]
    order = best if c.get(best, 0) >= c.get(rev, 0) else rev
    flags = (SINGLE if len(order) == 1 else 0) | (DUP if len(set(order)) < len(order) else 0)
    return seqs.index(order), cc[best], flags


def markers(kmers, nodes, sg_offsets, sg_nodes, record_offsets, n_tar: int, kmerlen: int, windowsize: int):
    """Every subgraph: list of dict(rows, seqs, rep) with rep = REP_DTYPE scalar values as a tuple + the ordering, flags NO_TARGET
    and n_rep 0 when no target has a row."""
    so = np.asarray(sg_offsets, np.int64)
    out = []
    for s in range(len(so) - 1):
        rows, seqs = loc(kmers, nodes, np.asarray(sg_nodes[so[s]:so[s + 1]], np.int64), record_offsets, kmerlen, windowsize)
        r = rep_order(rows, seqs, n_tar)
        rep = np.zeros((), REP_DTYPE)
        order = ()
        if r is None:
            rep["flags"] = NO_TARGET
        else:
            i, n_rep, flags = r
            for f in ROW_DTYPE.names:
                rep[f] = rows[i][f]
            rep["n_rep"], rep["flags"] = n_rep, flags
            order = seqs[i]
        out.append(dict(rows=rows, seqs=seqs, rep=rep, order=order))
    return out


def tables(res):
    """The result of :func:`markers` as flat arrays: reps, rep_offsets, rep_hashes, row_offsets, rows, kmer_offsets, row_hashes."""
    reps = np.array([r["rep"] for r in res], REP_DTYPE) if res else np.zeros(0, REP_DTYPE)
    rep_off = np.concatenate([[0], np.cumsum([len(r["order"]) for r in res])]).astype(np.uint64)
    rep_h = np.array([x for r in res for x in r["order"]], np.uint64)
    row_off = np.concatenate([[0], np.cumsum([len(r["rows"]) for r in res])]).astype(np.uint64)
    rows = np.concatenate([r["rows"] for r in res]) if res else np.zeros(0, ROW_DTYPE)
    k_off = np.concatenate([[0], np.cumsum([len(t) for r in res for t in r["seqs"]])]).astype(np.uint64)
    row_h = np.array([x for r in res for t in r["seqs"] for x in t], np.uint64)
    return dict(reps=reps, rep_offsets=rep_off, rep_hashes=rep_h, row_offsets=row_off, rows=rows, kmer_offsets=k_off, row_hashes=row_h)


def resident_inputs(kmers, nodes, fnodes, sg_offsets, sg_hashes):
    """What the device's resident route works on, from host arrays: filter_kmers(f, used) restated (the nodes of ``fnodes`` whose
    hash is a subgraph node, their occurrences, ranges re-based) and the subgraphs as indices into those kept nodes."""
    used = np.unique(np.asarray(sg_hashes, np.uint64))
    keep = fnodes[np.isin(fnodes["hash"], used)]
    src = nodes[np.searchsorted(nodes["hash"], keep["hash"])]
    ln = (src["stop"] - src["start"]).astype(np.int64)
    at = np.repeat(src["start"].astype(np.int64), ln) + (np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln))
    kept_nodes = keep.copy()
    kept_nodes["stop"] = np.cumsum(ln)
    kept_nodes["start"] = kept_nodes["stop"] - ln.astype(np.uint64)
    return kmers[at], kept_nodes, np.searchsorted(kept_nodes["hash"], np.asarray(sg_hashes, np.uint64)).astype(np.uint64)
