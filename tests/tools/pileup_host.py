"""Host restatement of the pileup (the device side is the pile walk of seqwin_amd/csrc/align.hip).  Nothing in
the reference computes this quantity; this file is its yardstick.

* A pair (query, strand, record, start, stop) has the script of section 3.2f (tests/tools/align_host.py): its ops in pattern order from
  a_start to end.  m = |query|, i' the pattern index from 0, j the text index from a_start, g the pair's group.
* The table is uint32 T[total query bases][G][8], the queries one behind the other; classes A 0, C 1, G 2, T 3, N 4, DEL 5, INS 6,
  INS_BASES 7.
* `=` / `X`: c = the code of text base j (invalid: N); u = i' (strand 0) or m - 1 - i' (strand 1); the class is c (strand 0) or 3 - c
  (strand 1), N stays N; T[u][g][class] += 1; i' and j advance.  The query's own base plays no part.
* `I`: T[u][g][DEL] += 1 with the same u; i' advances.
* A maximal run of L `D` before pattern index i': u = i' (strand 0) or m - i' (strand 1); T[u][g][INS] += 1, T[u][g][INS_BASES] += L; j
  advances by L.  A script neither begins nor ends with `D`, so 1 <= u <= m - 1 (asserted here).
* depth[q][g] = the pairs of q piled into g.  A pair is piled iff its label is below G and dist * 1000 <= max_dist_permille * m; label
  0xFF leaves it out.  An empty query has no rows; an empty text piles m DEL.

Two forms that share nothing but this text: :func:`pile_ops` walks the op arrays of ``align_host.alignments`` in NumPy;
:func:`pile_literal` writes the two gapped rows of ``align_host.align_literal_one``'s alignment as strings, turns a strand-1 alignment
round into the query's orientation, and counts columns.  :func:`best_hits_pileup` piles the winners of ``align_host.best_hits_aligned``.
"""
from __future__ import annotations

import numpy as np

import align_host as A
import hits_host as H

CLASSES = ("A", "C", "G", "T", "N", "DEL", "INS", "INS_BASES")
A_, C_, G_, T_, N_, DEL, INS, INS_BASES = range(8)
LEAVE_OUT = 0xFF


def check_args(labels, n_groups: int, max_dist_permille: int) -> None:
    if not 1 <= n_groups <= 8:
        raise ValueError(f"the pileup takes 1..8 groups (got {n_groups})")
    if not 0 <= max_dist_permille <= 1000:
        raise ValueError(f"max_dist_permille must lie in 0..1000 (got {max_dist_permille})")
    for x in labels:
        if not (0 <= int(x) < n_groups or int(x) == LEAVE_OUT):
            raise ValueError(f"group label {x} is neither below the {n_groups} groups nor 255")


def is_piled(label: int, n_groups: int, dist: int, m: int, max_dist_permille: int) -> bool:
    return int(label) < n_groups and int(dist) * 1000 <= int(max_dist_permille) * int(m)


def _offsets(queries) -> np.ndarray:
    offs = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(H._bytes(q)) for q in queries], out=offs[1:])
    return offs


def _empty(queries, n_groups):
    offs = _offsets(queries)
    return offs, np.zeros((int(offs[-1]), n_groups, 8), np.uint32), np.zeros((len(queries), n_groups), np.uint32)


# ---- the NumPy form: the op arrays ---------------------------------------------------------------------------------------------------

def add_script(rows: np.ndarray, g: int, strand: int, ops: np.ndarray, text_codes: np.ndarray) -> None:
    """Adds one script to rows ([m, G, 8] of its query); text_codes are the codes (4 = invalid) of the record from a_start on."""
    m = len(rows)
    ops = np.asarray(ops)
    pat = ops != 3                                               # ops that consume a pattern base
    ip = np.cumsum(pat) - pat                                    # the pattern index at every op
    txt = ops != 2
    jt = np.cumsum(txt) - txt                                    # the text index at every op
    assert int(pat.sum()) == m
    col = np.flatnonzero(ops <= 1)
    c = text_codes[jt[col]].astype(np.int64)
    u = m - 1 - ip[col] if strand else ip[col]
    cls = np.where(c > 3, N_, 3 - c if strand else c)
    np.add.at(rows, (u, g, cls), 1)
    gap = np.flatnonzero(ops == 2)
    np.add.at(rows, (m - 1 - ip[gap] if strand else ip[gap], g, DEL), 1)
    d = np.flatnonzero(ops == 3)
    if len(d):
        head = d[np.concatenate(([True], np.diff(d) > 1))]       # the first op of every maximal run
        length = np.diff(np.concatenate((np.flatnonzero(np.concatenate(([True], np.diff(d) > 1))), [len(d)])))
        slot = m - ip[head] if strand else ip[head]
        assert (slot >= 1).all() and (slot <= m - 1).all(), "a script neither begins nor ends with D"
        np.add.at(rows, (slot, g, INS), 1)
        np.add.at(rows, (slot, g, INS_BASES), length.astype(np.uint32))


def pile_ops(queries, records, pairs, groups, n_groups: int, max_dist_permille: int = 1000, al=None) -> dict:
    """table, depth, offsets, piled (bool per pair) and the alignment arrays of ``align_host.alignments`` (``al``: already made)."""
    check_args(groups, n_groups, max_dist_permille)
    al = A.alignments(queries, records, pairs) if al is None else al
    offs, table, depth = _empty(queries, n_groups)
    o = al["offsets"].astype(np.int64)
    piled = np.zeros(len(pairs), bool)
    for x, p in enumerate(pairs):
        q, strand, rec, start, stop = H._check_pair(p, len(queries), records)
        m = int(offs[q + 1] - offs[q])
        if not is_piled(groups[x], n_groups, al["dist"][x], m, max_dist_permille):
            continue
        piled[x] = True
        depth[q, int(groups[x])] += 1
        if m:
            add_script(table[offs[q]:offs[q + 1]], int(groups[x]), strand, al["ops"][o[x]:o[x + 1]], H._codes(records[rec])[int(al["start"][x]):])
    return dict(al, table=table, depth=depth, q_offsets=offs, piled=piled)


# ---- the literal form: two gapped rows ---------------------------------------------------------------------------------------------

def gapped_rows(pattern: str, text: str):
    """(dist, pattern row, text row) of the canonical alignment of a pattern in a text, both over ACGT and '#', gaps as '-'."""
    d, js, j0, _, _, _, ops = A.align_literal_one(pattern, text)
    top, bottom, i, j = [], [], 0, j0
    for op in ops:
        if op == "D":
            top.append("-"); bottom.append(text[j]); j += 1
        elif op == "I":
            top.append(pattern[i]); bottom.append("-"); i += 1
        else:
            top.append(pattern[i]); bottom.append(text[j]); i += 1; j += 1
    assert i == len(pattern) and j == js
    return d, "".join(top), "".join(bottom)


def count_columns(rows: np.ndarray, g: int, top: str, bottom: str) -> None:
    """Adds an alignment written in the QUERY's orientation to rows ([m, G, 8])."""
    m, u, run = len(rows), 0, 0
    for qc, tc in zip(top, bottom):
        if qc == "-":
            run += 1
            continue
        if run:
            assert 1 <= u <= m - 1, "an insertion lies between two query positions"
            rows[u, g, INS] += 1
            rows[u, g, INS_BASES] += run
            run = 0
        rows[u, g, DEL if tc == "-" else "ACGT#".index(tc)] += 1
        u += 1
    assert run == 0 and u == m


_COMP = str.maketrans("ACGT", "TGCA")


def add_rows(rows: np.ndarray, g: int, strand: int, top: str, bottom: str) -> None:
    """Adds an alignment written in the PATTERN's orientation: on strand 1 it is first read from the other strand."""
    if strand:
        top, bottom = top.translate(_COMP)[::-1], bottom.translate(_COMP)[::-1]
    count_columns(rows, g, top, bottom)


def pile_literal(queries, records, pairs, groups, n_groups: int, max_dist_permille: int = 1000) -> dict:
    check_args(groups, n_groups, max_dist_permille)
    offs, table, depth = _empty(queries, n_groups)
    for x, p in enumerate(pairs):
        q, strand, rec, start, stop = H._check_pair(p, len(queries), records)
        query = H._text(queries[q])
        d, top, bottom = gapped_rows(H._rc(query) if strand else query, H._text(records[rec])[start:stop])
        if not (int(groups[x]) < n_groups and d * 1000 <= max_dist_permille * len(query)):
            continue
        depth[q, int(groups[x])] += 1
        add_rows(table[offs[q]:offs[q + 1]], int(groups[x]), strand, top, bottom)
    return dict(table=table, depth=depth, q_offsets=offs)


# ---- best hits -------------------------------------------------------------------------------------------------------------------

def best_hits_pileup(queries, assemblies, k: int, assembly_group, n_groups: int, max_dist_permille: int = 1000, hits=None) -> dict:
    """``align_host.best_hits_aligned`` (``hits``: already made) plus the pileup of its winners, the winner in assembly a labelled
    assembly_group[a]: `table`, `depth`, `q_offsets`."""
    check_args(assembly_group, n_groups, max_dist_permille)
    out = A.best_hits_aligned(queries, assemblies, k) if hits is None else hits
    records = [r for recs in assemblies for r in recs]
    offs, table, depth = _empty(queries, n_groups)
    nq, na = out["seeds"].shape
    for q in range(nq):
        m = int(offs[q + 1] - offs[q])
        for a in range(na):
            if not out["seeds"][q, a] or not is_piled(assembly_group[a], n_groups, out["dist"][q, a], m, max_dist_permille):
                continue
            g = int(assembly_group[a])
            depth[q, g] += 1
            if m:
                add_script(table[offs[q]:offs[q + 1]], g, int(out["strand"][q, a]), out["scripts"][(q, a)],
                           H._codes(records[int(out["record"][q, a])])[int(out["start"][q, a]):])
    return dict(out, table=table, depth=depth, q_offsets=offs)


def invariants(table, depth, q_offsets, nident, mismatch, n_ins_ops, n_del_ops) -> None:
    """Column sum == depth at every position, no insertion before position 0, and the classes add up to the ops that made them
    (sums over the piled pairs: `=` + `X`, `I`, `D`)."""
    offs = np.asarray(q_offsets).astype(np.int64)
    for q in range(len(offs) - 1):
        rows = table[offs[q]:offs[q + 1]]
        assert (rows[:, :, :6].sum(axis=2) == depth[q][None, :]).all(), q
        if len(rows):
            assert not rows[0, :, INS].any() and not rows[0, :, INS_BASES].any(), q
    assert int(table[:, :, :5].sum()) == int(nident) + int(mismatch)
    assert int(table[:, :, DEL].sum()) == int(n_ins_ops)
    assert int(table[:, :, INS_BASES].sum()) == int(n_del_ops)
    assert (table[:, :, INS] <= table[:, :, INS_BASES]).all()
