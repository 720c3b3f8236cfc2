"""Host restatement of the oligo windows (the device side is the window walk of seqwin_amd/csrc/align.hip).
Nothing in the reference computes this quantity; this file is its yardstick.

* The pairs that count are the pairs the pileup piles (section 3.2k, tests/tools/pileup_host.py): label below G and
  dist * 1000 <= max_dist_permille * m.
* A piled pair (query of m bases, strand, group g) has the script of section 3.2f (tests/tools/align_host.py).  Per pattern index i':
  x[i'] = 1 iff the column that consumes i' is `X`; ins[i'] = 1 iff it is `I`; for 1 <= i' <= m - 1, b[i'] = 1 iff a run of `D` lies
  before pattern index i'.
* The pattern window [s, s + L), 0 <= s <= m - L: e = the sum of x over it; gapped iff some ins lies in it or some b[i'] has
  s < i' < s + L (a run exactly at an edge does not gap it).
* Its start in query coordinates is u = s (strand 0) or m - L - s (strand 1).  right_bad iff an `X` faces one of the query positions
  u + L - c .. u + L - 1, left_bad iff one of u .. u + c - 1 (c = three_prime; with c = 0 neither).
* W[offsets[q] + u][l][g][class] += 1 for exactly one of MM0 0, MM1 1, MM2 2, MM3 3 (ungapped, e = 0..3), MM4P 4 (ungapped, e >= 4),
  GAPPED 5; and for FWD_OK 6 (ungapped, e <= max_mismatch, not right_bad) and REV_OK 7 (ungapped, e <= max_mismatch, not left_bad)
  where they hold.  Rows with u > m - L stay 0.

Two forms that share nothing but this text and the script: :func:`add_script_loops` reads the definitions above literally, window by
window and base by base, in the pattern's orientation; :func:`add_script_prefix` first turns x, ins and b into the query's orientation
and then takes every window of a length at once from prefix sums.
"""
from __future__ import annotations

import numpy as np

import align_host as A
import hits_host as H
import pileup_host as P

CLASSES = ("MM0", "MM1", "MM2", "MM3", "MM4P", "GAPPED", "FWD_OK", "REV_OK")
MM0, MM1, MM2, MM3, MM4P, GAPPED, FWD_OK, REV_OK = range(8)


def check_args(lengths, max_mismatch: int, three_prime: int) -> None:
    lengths = [int(x) for x in lengths]
    if not 1 <= len(lengths) <= 8:
        raise ValueError(f"the windows take 1..8 lengths (got {len(lengths)})")
    for x in lengths:
        if not 8 <= x <= 32:
            raise ValueError(f"window length {x} lies outside 8..32")
    if len(set(lengths)) != len(lengths):
        raise ValueError("a window length is given twice")
    if not 0 <= max_mismatch <= 8 or max_mismatch >= min(lengths):
        raise ValueError(f"max_mismatch must lie in 0..8 and below the shortest length (got {max_mismatch})")
    if not 0 <= three_prime <= 8:
        raise ValueError(f"three_prime must lie in 0..8 (got {three_prime})")


# ---- form 1: the definitions, literally ----------------------------------------------------------------------------------------------

def add_script_loops(rows: np.ndarray, g: int, strand: int, ops, lengths, max_mismatch: int, three_prime: int) -> None:
    """Adds one script to rows ([m, n_lengths, G, 8] of its query)."""
    m = len(rows)
    column = []                                                 # the op that consumes every pattern index
    run_before = set()                                          # pattern indices with a run of D before them
    for op in ops:
        op = int(op)
        if op == 3:
            run_before.add(len(column))
        else:
            column.append(op)
    assert len(column) == m and 0 not in run_before and m not in run_before, "a script neither begins nor ends with D"
    for l, L in enumerate(lengths):
        for s in range(0, m - L + 1):
            e = 0
            gapped = False
            for i in range(s, s + L):
                if column[i] == 1:
                    e += 1
                if column[i] == 2:
                    gapped = True
                if s < i and i in run_before:
                    gapped = True
            u = m - L - s if strand else s

            def faces_x(query_position):
                return column[m - 1 - query_position if strand else query_position] == 1

            right_bad = any(faces_x(p) for p in range(u + L - three_prime, u + L))
            left_bad = any(faces_x(p) for p in range(u, u + three_prime))
            if gapped:
                rows[u, l, g, GAPPED] += 1
                continue
            rows[u, l, g, min(e, 4)] += 1
            if e <= max_mismatch and not right_bad:
                rows[u, l, g, FWD_OK] += 1
            if e <= max_mismatch and not left_bad:
                rows[u, l, g, REV_OK] += 1


# ---- form 2: prefix sums in the query's orientation ------------------------------------------------------------------------------------

def script_arrays(ops, m: int):
    """x, ins, b (uint8[m] each, b[0] = 0) of a script, in the pattern's orientation."""
    ops = np.asarray(ops)
    pat = ops != 3
    ip = np.cumsum(pat) - pat                                   # the pattern index at every op; for a D: the index it lies before
    assert int(pat.sum()) == m
    x, ins, b = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m + 1, np.int64)
    x[ip[ops == 1]] = 1
    ins[ip[ops == 2]] = 1
    b[ip[ops == 3]] = 1
    assert not b[0] and not b[m]
    return x, ins, b[:m]


def add_script_prefix(rows: np.ndarray, g: int, strand: int, ops, lengths, max_mismatch: int, three_prime: int) -> None:
    m = len(rows)
    if not m:
        return
    x, ins, b = script_arrays(ops, m)
    if strand:                                                  # query position m - 1 - i'; a run before i' lies before query position m - i'
        x, ins = x[::-1], ins[::-1]
        b = np.concatenate(([0], b[1:][::-1]))
    cx, ci, cb = (np.concatenate(([0], np.cumsum(a))) for a in (x, ins, b))
    c = three_prime
    for l, L in enumerate(lengths):
        if m < L:
            continue
        u = np.arange(m - L + 1)
        e = cx[u + L] - cx[u]
        gapped = (ci[u + L] - ci[u] > 0) | (cb[u + L] - cb[u + 1] > 0)      # b at u + 1 .. u + L - 1
        right_bad = cx[u + L] - cx[u + L - c] > 0
        left_bad = cx[u + c] - cx[u] > 0
        cls = np.where(gapped, GAPPED, np.minimum(e, 4))
        np.add.at(rows, (u, l, g, cls), 1)
        ok = ~gapped & (e <= max_mismatch)
        rows[u[ok & ~right_bad], l, g, FWD_OK] += 1
        rows[u[ok & ~left_bad], l, g, REV_OK] += 1


FORMS = {"loops": add_script_loops, "prefix": add_script_prefix}


# ---- lists of pairs and best hits ------------------------------------------------------------------------------------------------------

def windows_ops(queries, records, pairs, groups, n_groups: int, lengths, max_mismatch: int = 2, three_prime: int = 3, max_dist_permille: int = 1000,
                al=None, form: str = "prefix") -> dict:
    """wtable ([total, n_lengths, G, 8]), depth, q_offsets, piled and the alignment arrays of ``align_host.alignments`` (``al``:
    already made)."""
    P.check_args(groups, n_groups, max_dist_permille)
    check_args(lengths, max_mismatch, three_prime)
    al = A.alignments(queries, records, pairs) if al is None else al
    offs = P._offsets(queries)
    wtable = np.zeros((int(offs[-1]), len(lengths), n_groups, 8), np.uint32)
    depth = np.zeros((len(queries), n_groups), np.uint32)
    o = al["offsets"].astype(np.int64)
    piled = np.zeros(len(pairs), bool)
    for i, p in enumerate(pairs):
        q, strand, rec, start, stop = H._check_pair(p, len(queries), records)
        m = int(offs[q + 1] - offs[q])
        if not P.is_piled(groups[i], n_groups, al["dist"][i], m, max_dist_permille):
            continue
        piled[i] = True
        depth[q, int(groups[i])] += 1
        FORMS[form](wtable[offs[q]:offs[q + 1]], int(groups[i]), strand, al["ops"][o[i]:o[i + 1]], list(lengths), max_mismatch, three_prime)
    return dict(al, wtable=wtable, depth=depth, q_offsets=offs, piled=piled)


def best_hits_windows(queries, assemblies, k: int, assembly_group, n_groups: int, lengths, max_mismatch: int = 2, three_prime: int = 3,
                      max_dist_permille: int = 1000, hits=None, form: str = "prefix") -> dict:
    """``align_host.best_hits_aligned`` (``hits``: already made) plus the windows of its winners, the winner in assembly a labelled
    assembly_group[a]: `wtable`, `depth`, `q_offsets`."""
    P.check_args(assembly_group, n_groups, max_dist_permille)
    check_args(lengths, max_mismatch, three_prime)
    out = A.best_hits_aligned(queries, assemblies, k) if hits is None else hits
    offs = P._offsets(queries)
    wtable = np.zeros((int(offs[-1]), len(lengths), n_groups, 8), np.uint32)
    depth = np.zeros((len(queries), n_groups), np.uint32)
    nq, na = out["seeds"].shape
    for q in range(nq):
        m = int(offs[q + 1] - offs[q])
        for a in range(na):
            if not out["seeds"][q, a] or not P.is_piled(assembly_group[a], n_groups, out["dist"][q, a], m, max_dist_permille):
                continue
            g = int(assembly_group[a])
            depth[q, g] += 1
            FORMS[form](wtable[offs[q]:offs[q + 1]], g, int(out["strand"][q, a]), out["scripts"][(q, a)], list(lengths), max_mismatch, three_prime)
    return dict(out, wtable=wtable, depth=depth, q_offsets=offs)


def invariants(wtable, depth, q_offsets, lengths) -> None:
    """Classes 0..5 add up to the depth at every window start u <= m - L, rows behind it are 0, and FWD_OK / REV_OK never exceed the
    ungapped pairs."""
    offs = np.asarray(q_offsets).astype(np.int64)
    for q in range(len(offs) - 1):
        rows = wtable[offs[q]:offs[q + 1]]
        m = len(rows)
        for l, L in enumerate(lengths):
            n = max(m - L + 1, 0)
            assert (rows[:n, l, :, :6].sum(axis=2) == depth[q][None, :]).all(), (q, L)
            assert not rows[n:, l].any(), (q, L)
            ungapped = rows[:n, l, :, :5].sum(axis=2)
            assert (rows[:n, l, :, FWD_OK] <= ungapped).all() and (rows[:n, l, :, REV_OK] <= ungapped).all(), (q, L)
