"""Host restatement of the canonical alignment behind the infix edit distance (the device side is
seqwin_amd/csrc/align.hip).  Nothing in the reference computes this quantity; this file is its yardstick.

* A pair (query, strand, record, start, stop) is Layer A's (tests/tools/hits_host.py): P the query or its reverse complement, m = |P|,
  T = record[start:stop], n = |T|; D[0][j] = 0, D[i][0] = i, unit costs, an invalid base equals nothing.  dist = D[m][j*] with j* the
  smallest column of the minimum, end = start + j*.
* The canonical traceback starts at (i, j) = (m, j*) and repeats, first match wins, until i == 0:
    1. j > 0 and P[i-1] == T[j-1], both valid           op `=`, to (i-1, j-1)
    2. j > 0 and D[i-1][j-1] + 1 == D[i][j]             op `X`, to (i-1, j-1)
    3. D[i-1][j] + 1 == D[i][j]                          op `I` (a pattern base faces a gap), to (i-1, j)
    4. otherwise (j > 0 and D[i][j-1] + 1 == D[i][j])    op `D` (a text base faces a gap), to (i, j-1)
* a_start = start + j at the stop; nident = #`=`, mismatch = #`X`, gaps = #`I` + #`D`.  The script is the ops in pattern order from
  a_start to end, one byte each: `=` 0, `X` 1, `I` 2, `D` 3; it has m + #D entries.

Two forms that share nothing but this text: :func:`align_one` / :func:`alignments` keep the whole matrix as a NumPy array filled row
by row and walk it on code arrays; :func:`align_literal_one` / :func:`alignments_literal` are plain Python on strings, the distance a
memoised top-down recursion, the walk asking it for the sub-problems each rule names.  :func:`replay` applies a script to P.
"""
from __future__ import annotations

import sys

import numpy as np

import hits_host as H

OPS = "=XID"
FIELDS = ("dist", "end", "start", "nident", "mismatch", "gaps")


# ---- the NumPy form --------------------------------------------------------------------------------------------------------------

def matrix(pattern_codes: np.ndarray, text_codes: np.ndarray) -> np.ndarray:
    """The infix matrix D[(m + 1), (n + 1)] of a pattern and a text given as codes 0..3, 4 = invalid."""
    m, n = len(pattern_codes), len(text_codes)
    text = np.where(text_codes > 3, 5, text_codes)          # 5 never equals the pattern's 4
    D = np.zeros((m + 1, n + 1), np.int32)
    ar = np.arange(n + 1, dtype=np.int32)
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int32)
        t[0] = i
        t[1:] = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (text != pattern_codes[i - 1]))
        D[i] = np.minimum.accumulate(t - ar) + ar           # D[i][j] = min over j' <= j of t[j'] + (j - j')
    return D


def align_one(pattern_codes: np.ndarray, text_codes: np.ndarray):
    """(dist, j*, j at the stop, nident, mismatch, gaps, ops uint8[] in pattern order)."""
    m = len(pattern_codes)
    D = matrix(pattern_codes, text_codes)
    js = int(np.argmin(D[m]))
    i, j, ops = m, js, []
    while i > 0:
        if j > 0 and pattern_codes[i - 1] < 4 and pattern_codes[i - 1] == text_codes[j - 1]:
            ops.append(0); i -= 1; j -= 1
        elif j > 0 and D[i - 1, j - 1] + 1 == D[i, j]:
            ops.append(1); i -= 1; j -= 1
        elif D[i - 1, j] + 1 == D[i, j]:
            ops.append(2); i -= 1
        else:
            assert j > 0 and D[i, j - 1] + 1 == D[i, j]
            ops.append(3); j -= 1
    ops = np.array(ops[::-1], np.uint8)
    return int(D[m, js]), js, j, int((ops == 0).sum()), int((ops == 1).sum()), int((ops >= 2).sum()), ops


def _collect(rows, starts):
    out = {f: np.zeros(len(rows), np.uint32) for f in FIELDS}
    offsets = np.zeros(len(rows) + 1, np.uint64)
    scripts = []
    for x, ((d, js, j0, ni, nx, ng, ops), start) in enumerate(zip(rows, starts)):
        out["dist"][x], out["end"][x], out["start"][x] = d, start + js, start + j0
        out["nident"][x], out["mismatch"][x], out["gaps"][x] = ni, nx, ng
        offsets[x + 1] = offsets[x] + np.uint64(len(ops))
        scripts.append(ops)
    out["offsets"] = offsets
    out["ops"] = np.concatenate(scripts).astype(np.uint8) if scripts else np.zeros(0, np.uint8)
    return out


def alignments(queries, records, pairs) -> dict:
    """dist, end, start, nident, mismatch, gaps (uint32[n]) and the scripts (offsets uint64[n + 1], ops uint8[]) of pairs
    (query, strand, record, start, stop)."""
    rows, starts = [], []
    for p in pairs:
        q, strand, rec, start, stop = H._check_pair(p, len(queries), records)
        rows.append(align_one(H._strand_codes(queries[q], strand), H._codes(records[rec])[start:stop]))
        starts.append(start)
    return _collect(rows, starts)


# ---- the literal form ------------------------------------------------------------------------------------------------------------

def align_literal_one(pattern: str, text: str):
    """The same for a pattern and a text over ACGT and '#', which equals nothing; ops as a string over =XID."""
    m, n = len(pattern), len(text)
    memo = {}

    def same(i, j):
        return pattern[i - 1] == text[j - 1] and pattern[i - 1] != "#"

    def dist(i, j):                                         # D[i][j]: the cheapest way to write pattern[:i] as a suffix of text[:j]
        if i == 0:
            return 0
        if j == 0:
            return i
        if (i, j) not in memo:
            memo[(i, j)] = min(dist(i - 1, j) + 1, dist(i, j - 1) + 1, dist(i - 1, j - 1) + (0 if same(i, j) else 1))
        return memo[(i, j)]

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * (m + n) + 200))
    try:
        best, js = m, 0
        for j in range(1, n + 1):
            if dist(m, j) < best:
                best, js = dist(m, j), j
        i, j, rev = m, js, []
        while i > 0:
            here = dist(i, j)
            if j > 0 and same(i, j):
                rev.append("="); i, j = i - 1, j - 1
            elif j > 0 and dist(i - 1, j - 1) + 1 == here:
                rev.append("X"); i, j = i - 1, j - 1
            elif dist(i - 1, j) + 1 == here:
                rev.append("I"); i = i - 1
            else:
                assert j > 0 and dist(i, j - 1) + 1 == here
                rev.append("D"); j = j - 1
    finally:
        sys.setrecursionlimit(limit)
    ops = "".join(reversed(rev))
    return best, js, j, ops.count("="), ops.count("X"), ops.count("I") + ops.count("D"), ops


def alignments_literal(queries, records, pairs) -> dict:
    rows, starts = [], []
    for p in pairs:
        q, strand, rec, start, stop = H._check_pair(p, len(queries), records)
        pat = H._text(queries[q])
        d, js, j0, ni, nx, ng, ops = align_literal_one(H._rc(pat) if strand else pat, H._text(records[rec])[start:stop])
        rows.append((d, js, j0, ni, nx, ng, np.array([OPS.index(c) for c in ops], np.uint8)))
        starts.append(start)
    return _collect(rows, starts)


# ---- replay ----------------------------------------------------------------------------------------------------------------------

def replay(pattern: str, ops) -> str:
    """The text a script implies for a pattern over ACGT and '#': the pattern's base under `=`, '?' under `X` (a base that does not
    equal the pattern's), nothing under `I`, '*' under `D` (any base).  ValueError unless the script consumes the pattern whole."""
    out, i = [], 0
    for op in ops:
        op = OPS[int(op)] if not isinstance(op, str) else op
        if op == "D":
            out.append("*")
            continue
        if i >= len(pattern):
            raise ValueError("the script is longer than the pattern")
        out.append({"=": pattern[i], "X": "?", "I": ""}[op])
        i += 1
    if i != len(pattern):
        raise ValueError(f"the script consumes {i} of the pattern's {len(pattern)} bases")
    return "".join(out)


def replay_matches(pattern: str, ops, segment: str) -> bool:
    """Whether `segment` (over ACGT and '#') is a text the script implies: equal and valid under `=`, not so under `X`."""
    implied = replay(pattern, ops)
    if len(implied) != len(segment):
        return False
    i = x = 0
    for op in ops:
        op = OPS[int(op)] if not isinstance(op, str) else op
        if op == "I":
            i += 1
        elif op == "D":
            x += 1
        else:
            eq = pattern[i] == segment[x] and pattern[i] != "#"
            if eq != (op == "="):
                return False
            i += 1
            x += 1
    return True


# ---- best hits -------------------------------------------------------------------------------------------------------------------

def best_hits_aligned(queries, assemblies, k: int) -> dict:
    """hits_host.best_hits plus, per (query, assembly) with a hit, the alignment on the window of section 3.2e: `start`, `nident`,
    `mismatch`, `gaps` (0xFFFFFFFF without a hit), the window itself as `lo` / `hi`, and `scripts[(q, a)]` (uint8 ops).  The windows
    are taken from the restatement as it computes them: its Layer A calls are listened to, in its order (assemblies ascending,
    queries ascending inside one), and lo = end - j."""
    calls = []
    orig = H.infix_one

    def listen(pattern_codes, text_codes):
        r = orig(pattern_codes, text_codes)
        calls.append((pattern_codes, text_codes, r))
        return r

    H.infix_one = listen
    try:
        out = H.best_hits(queries, assemblies, k)
    finally:
        H.infix_one = orig
    nq, na = out["seeds"].shape
    for f in ("start", "nident", "mismatch", "gaps", "lo", "hi"):
        out[f] = np.full((nq, na), H.NONE, np.uint32)
    out["scripts"] = {}
    at = 0
    for a in range(na):
        for q in range(nq):
            if not out["seeds"][q, a]:
                continue
            pc, tc, (d, j) = calls[at]
            at += 1
            lo = int(out["end"][q, a]) - j
            d2, js, j0, ni, nx, ng, ops = align_one(pc, tc)
            assert (d2, js) == (d, j) == (int(out["dist"][q, a]), js)
            out["lo"][q, a], out["hi"][q, a] = lo, lo + len(tc)
            out["start"][q, a], out["nident"][q, a], out["mismatch"][q, a], out["gaps"][q, a] = lo + j0, ni, nx, ng
            out["scripts"][(q, a)] = ops
    assert at == len(calls)
    return out
