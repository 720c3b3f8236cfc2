"""Host restatement of the oligo search with indels (csrc/oligo.hip, Batch.oligo_hits(max_edits=)), twice.

A text is one valid run T of a record (a maximal stretch of ACGTU in either case, U = T), n bases.  An oligo P is L sets of bases,
Q = P[:L - c] its part before the 3' clamp of c letters.  On strand 0, for an end 1 <= e <= n:

    E(e) = Dm[|Q|][e - c]   if e >= c and T[e - c + i] lies in P[L - c + i] for every i < c, else infinite
    Dm[0][j] = 0, Dm[i][0] = i, unit costs over Q and T, a base equals a letter iff it lies in the letter's set
    D(e) = min(E(e), d + 1)

(Dm[|Q|][j] is the least ed(Q, T[b:j]) over b <= j.)  e is a site iff D(e) <= d, D(e') > D(e) on [e - d, e) and D(e') >= D(e) on
(e, e + d], both inside the run.  The site's alignment is the canonical traceback of tests/tools/align_host.py from (|Q|, e - c) until
i == 0 -- rules `=`, `X`, `I`, `D` in that order, the first that holds wins --, the stop column is the start b, mismatch = #X,
gaps = #I + #D, dist = D(e).  Strand 1 is strand 0 on the reverse complement of the run with [b', e') mapped to [n - e', n - b').
Per (oligo, assembly): n_sites and the site least in (dist, record, pos, strand), then end.  The list is ordered by
(oligo, assembly, record, pos, end, strand).

    sites_matrix    NumPy: the whole matrix per (pattern, run), filled row by row, the walk on it
    sites_literal   plain Python: D a memoised recursion, every rule asked of it literally
    search          either of them as the arrays Batch.oligo_hits(max_edits=) returns
"""
import sys

import numpy as np

import oligo_host as H

NO_HIT = 0xFFFFFFFF
SITE_FIELDS = ("oligo", "assembly", "record", "pos", "end", "strand", "dist", "mismatch", "gaps")
BEST_FIELDS = ("best_dist", "best_record", "best_pos", "best_strand", "best_end", "best_mismatch", "best_gaps")


def sets_of(oligo):
    return H.strands(oligo)[0]


def runs_of(rec):
    """[(start, text over ACGT)] of a record's valid runs"""
    t = H._text(rec).upper().replace("U", "T")
    out, i = [], 0
    while i < len(t):
        if t[i] not in "ACGT":
            i += 1
            continue
        j = i
        while j < len(t) and t[j] in "ACGT":
            j += 1
        out.append((i, t[i:j]))
        i = j
    return out


def _rc(t):
    return t.translate(str.maketrans("ACGT", "TGCA"))[::-1]


# ---- the NumPy form --------------------------------------------------------------------------------------------------------------

def run_sites_matrix(P, T, d, c):
    """[(b, e, dist, mismatch, gaps)] of the sets P on the text T, strand 0"""
    L, n = len(P), len(T)
    m = L - c
    codes = np.frombuffer(T.encode(), np.uint8)
    codes = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), codes)
    member = np.array([[b in s for b in "ACGT"] for s in P], bool)
    eq = member[:, codes] if n else np.zeros((L, 0), bool)          # eq[i, j]: T[j] lies in P[i]
    Dm = np.zeros((m + 1, n + 1), np.int32)
    ar = np.arange(n + 1, dtype=np.int32)
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int32)
        t[0] = i
        t[1:] = np.minimum(Dm[i - 1, 1:] + 1, Dm[i - 1, :-1] + ~eq[i - 1])
        Dm[i] = np.minimum.accumulate(t - ar) + ar
    Dv = np.full(n + 1, d + 1, np.int32)                             # Dv[e], e = 0 is no end
    if n >= c:
        ok = np.ones(n - c + 1, bool)                                # ok[j]: the clamp holds at T[j : j + c]
        for i in range(c):
            ok &= eq[m + i, i:n - c + 1 + i]
        Dv[c:] = np.where(ok, np.minimum(Dm[m, :n - c + 1], d + 1), d + 1)
    Dv[0] = d + 1
    out = []
    for e in np.nonzero(Dv <= d)[0].tolist():
        v = Dv[e]
        if (Dv[max(1, e - d):e] <= v).any() or (Dv[e + 1:min(n, e + d) + 1] < v).any():
            continue
        i, j, nx, ng = m, e - c, 0, 0
        while i > 0:
            if j > 0 and eq[i - 1, j - 1]:
                i, j = i - 1, j - 1
            elif j > 0 and Dm[i - 1, j - 1] + 1 == Dm[i, j]:
                i, j, nx = i - 1, j - 1, nx + 1
            elif Dm[i - 1, j] + 1 == Dm[i, j]:
                i, ng = i - 1, ng + 1
            else:
                assert j > 0 and Dm[i, j - 1] + 1 == Dm[i, j]
                j, ng = j - 1, ng + 1
        assert nx + ng == v
        out.append((j, e, int(v), nx, ng))
    return out


# ---- the literal form ------------------------------------------------------------------------------------------------------------

def run_sites_literal(P, T, d, c):
    L, n = len(P), len(T)
    Q = P[:L - c]
    m = len(Q)
    memo = {}

    def same(i, j):
        return T[j - 1] in Q[i - 1]

    def dist(i, j):
        if i == 0:
            return 0
        if j == 0:
            return i
        if (i, j) not in memo:
            memo[(i, j)] = min(dist(i - 1, j) + 1, dist(i, j - 1) + 1, dist(i - 1, j - 1) + (0 if same(i, j) else 1))
        return memo[(i, j)]

    def D(e):
        if e < c or any(T[e - c + i] not in P[L - c + i] for i in range(c)):
            return d + 1
        return min(dist(m, e - c), d + 1)

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10 * (m + 10) + 1000))
    try:
        for j in range(n + 1):                                       # (ascending: the recursion stays as deep as the pattern is long)
            dist(m, j)
        out = []
        for e in range(1, n + 1):
            v = D(e)
            if v > d:
                continue
            if not all(D(x) > v for x in range(e - d, e) if 1 <= x <= n):
                continue
            if not all(D(x) >= v for x in range(e + 1, e + d + 1) if 1 <= x <= n):
                continue
            i, j, ops = m, e - c, []
            while i > 0:
                here = dist(i, j)
                if j > 0 and same(i, j):
                    ops.append("="); i, j = i - 1, j - 1
                elif j > 0 and dist(i - 1, j - 1) + 1 == here:
                    ops.append("X"); i, j = i - 1, j - 1
                elif dist(i - 1, j) + 1 == here:
                    ops.append("I"); i = i - 1
                else:
                    assert j > 0 and dist(i, j - 1) + 1 == here
                    ops.append("D"); j = j - 1
            out.append((j, e, v, ops.count("X"), ops.count("I") + ops.count("D")))
    finally:
        sys.setrecursionlimit(limit)
    return out


# ---- both strands, all records -----------------------------------------------------------------------------------------------------

def _sites(oligos, assemblies, d, c, run_sites):
    out = []
    rec0 = 0
    for a, recs in enumerate(assemblies):
        for ri, rec in enumerate(recs):
            for start, T in runs_of(rec):
                n = len(T)
                texts = (T, _rc(T))
                for q, o in enumerate(oligos):
                    P = sets_of(o)
                    for s in (0, 1):
                        for b, e, v, nx, ng in run_sites(P, texts[s], d, c):
                            pos, end = (b, e) if s == 0 else (n - e, n - b)
                            out.append((q, a, rec0 + ri, start + pos, start + end, s, v, nx, ng))
        rec0 += len(recs)
    return sorted(out)


def sites_matrix(oligos, assemblies, d, c=0):
    """sorted list of (oligo, assembly, record, pos, end, strand, dist, mismatch, gaps); record is global"""
    return _sites(oligos, assemblies, d, c, run_sites_matrix)


def sites_literal(oligos, assemblies, d, c=0):
    return _sites(oligos, assemblies, d, c, run_sites_literal)


def search(oligos, assemblies, d, c=0, form=sites_matrix):
    """dict: n_sites and the seven best_* fields [nq, na] uint32, and sites (the nine columns + cell_offsets)"""
    S = form(oligos, assemblies, d, c)
    nq, na = len(oligos), len(assemblies)
    n_sites = np.zeros((nq, na), np.uint32)
    best = {f: np.full((nq, na), NO_HIT, np.uint32) for f in BEST_FIELDS}
    key = {}
    for q, a, r, p, e, s, v, nx, ng in S:
        n_sites[q, a] += 1
        k = (v, r, p, s, e, nx, ng)
        if (q, a) not in key or k < key[q, a]:
            key[q, a] = k
    for (q, a), (v, r, p, s, e, nx, ng) in key.items():
        for f, x in zip(BEST_FIELDS, (v, r, p, s, e, nx, ng)):
            best[f][q, a] = x
    cols = np.array(S, np.uint32).reshape(-1, 9)
    sites = {f: cols[:, i].copy() for i, f in enumerate(SITE_FIELDS)}
    sites["cell_offsets"] = np.concatenate([[0], np.cumsum(n_sites.reshape(-1), dtype=np.uint64)]).astype(np.uint64)
    return dict(n_sites=n_sites, sites=sites, **best)
