"""Host restatement of the local alignment with affine gap scores (the device side is
seqwin_amd/csrc/local.hip).  Nothing in the reference computes this quantity -- it is NOT BLAST: no seeds of BLAST's, no X-drop, no
e-values -- so this file is its yardstick.

* A pair (query, strand, record, start, stop) is Layer A's (tests/tools/hits_host.py): P the query or its reverse complement, m = |P|,
  T = record[start:stop], n = |T|; an invalid base equals nothing.
* Scoring (r, p, go, ge): s(i, j) = r if P[i-1] == T[j-1], both valid, else p; a gap of L columns costs go + L ge.
    E[i][j] = max(E[i][j-1], H[i][j-1] - go) - ge, E[i][0] = -inf        (a text base faces a gap)
    F[i][j] = max(F[i-1][j], H[i-1][j] - go) - ge, F[0][j] = -inf        (a pattern base faces a gap)
    H[i][j] = max(0, H[i-1][j-1] + s(i, j), E[i][j], F[i][j]), H[0][j] = H[i][0] = 0
* Every value carries a record (i0, j0, mismatch, gapopen, gaps): H = 0 carries (i, j, 0, 0, 0); E takes E[i][j-1]'s with gaps + 1 if
  E[i][j-1] >= H[i][j-1] - go (extension wins a tie), else H[i][j-1]'s with gapopen + 1, gaps + 1; F likewise from row i - 1; a positive
  H takes the record of the first of diagonal, E, F that attains the maximum, the diagonal adding mismatch + 1 when s = p.
* score = max H; the end cell (i*, j*) is the maximal cell with the smallest j, then the smallest i; qstart = i0, qend = i*, sstart =
  start + j0, send = start + j*; ins = (gaps + (i* - i0) - (j* - j0)) / 2, nident = (i* - i0) - mismatch - ins.  score == 0: all 0,
  sstart = send = start.

Two forms that share nothing but this text.  :func:`local_one` / :func:`alignments` work a row at a time on NumPy arrays with the
records packed into two integers: F and the diagonal come from the row above whole; E is a running maximum, because a gap is never
opened from a cell whose H came out of E itself (go >= 0), so E[i][j] = max over j' < j of G[j'] - go - (j - j') ge with G = max(0,
diagonal, F), and "extension wins a tie" makes the smallest such j' the one whose record is carried.  :func:`local_literal_one` /
:func:`alignments_literal` are plain Python: a loop over rows, columns and candidates on tuples.  :func:`check` rebuilds the score
from the counts.
"""
from __future__ import annotations

import numpy as np

import hits_host as H

FIELDS = ("score", "qstart", "qend", "sstart", "send", "nident", "mismatch", "gapopen", "gaps")
BLASTN = (2, -3, 5, 2)
SCORINGS = [(2, -3, 5, 2), (1, -2, 0, 1), (1, -1, 1, 1), (1, -3, 5, 2), (5, -4, 10, 6)]
NEG = -(1 << 40)


def check_scoring(scoring):
    r, p, go, ge = (int(x) for x in scoring)
    if not (1 <= r <= 255 and -255 <= p <= -1 and 0 <= go <= 255 and 1 <= ge <= 255):
        raise ValueError(f"scoring {tuple(scoring)} lies outside 1..255, -255..-1, 0..255, 1..255")
    return r, p, go, ge


def _finish(score, i1, j1, i0, j0, mm, op, gp):
    if score <= 0:
        return (0,) * 9
    rows, cols = i1 - i0, j1 - j0
    ins = (gp + rows - cols) // 2
    return (score, i0, i1, j0, j1, rows - mm - ins, mm, op, gp)


# ---- the NumPy form --------------------------------------------------------------------------------------------------------------
# a record as two integers: org = i0 << 20 | j0; cnt = mismatch | gapopen << 20 | gaps << 40
_OPEN, _EXT = (1 << 20) | (1 << 40), 1 << 40


def local_one(pattern_codes: np.ndarray, text_codes: np.ndarray, scoring=BLASTN):
    """(score, qstart, qend, j0, j*, nident, mismatch, gapopen, gaps) of a pattern and a text given as codes 0..3, 4 = invalid."""
    r, p, go, ge = check_scoring(scoring)
    m, n = len(pattern_codes), len(text_codes)
    if m >= 1 << 16 or n >= 1 << 16:
        raise ValueError("a side of a local alignment stays below 2^16")
    if m == 0 or n == 0:
        return (0,) * 9
    text = np.where(text_codes > 3, 5, text_codes).astype(np.int64)
    js = np.arange(n + 1, dtype=np.int64)
    h = np.zeros(n + 1, np.int64)
    h_org, h_cnt = js.copy(), np.zeros(n + 1, np.int64)              # row 0: (0, j, 0, 0, 0)
    f = np.full(n + 1, NEG, np.int64)
    f_org, f_cnt = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    best = (0, 0, 0, 0, 0)                                           # score, i, j, org, cnt
    for i in range(1, m + 1):
        zero_org = (i << 20) | js
        # F from the row above
        ext = f >= h - go
        nf = np.where(ext, f, h - go) - ge
        nf_org, nf_cnt = np.where(ext, f_org, h_org), np.where(ext, f_cnt + _EXT, h_cnt + _OPEN)
        nf[0] = NEG
        # the diagonal
        hit = text == int(pattern_codes[i - 1])
        d = np.full(n + 1, NEG, np.int64)
        d[1:] = h[:-1] + np.where(hit, r, p)
        d_org, d_cnt = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        d_org[1:], d_cnt[1:] = h_org[:-1], h_cnt[:-1] + np.where(hit, 0, 1)
        # G = max(0, diagonal, F) with its record: what a gap along the row is opened from
        g = np.maximum(d, nf)
        g_org, g_cnt = np.where(d >= nf, d_org, nf_org), np.where(d >= nf, d_cnt, nf_cnt)
        dead = g <= 0
        g, g_org, g_cnt = np.where(dead, 0, g), np.where(dead, zero_org, g_org), np.where(dead, 0, g_cnt)
        # E[j] = max over j' < j of g[j'] - go - (j - j') ge, the smallest j' of the maximum
        key = ((g - go + js * ge) << 20) | ((1 << 20) - 1 - js)
        run = np.maximum.accumulate(key)[:-1]                        # run[j - 1]: over j' <= j - 1
        src = (1 << 20) - 1 - (run & ((1 << 20) - 1))
        e = np.full(n + 1, NEG, np.int64)
        e[1:] = (run >> 20) - js[1:] * ge
        e_org, e_cnt = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        e_org[1:] = g_org[src]
        e_cnt[1:] = g_cnt[src] + _OPEN + (js[1:] - src - 1) * _EXT
        # H: the first of diagonal, E, F that attains the maximum
        use_d, use_e = (d >= e) & (d >= nf), e >= nf
        nh = np.where(use_d, d, np.where(use_e, e, nf))
        nh_org = np.where(use_d, d_org, np.where(use_e, e_org, nf_org))
        nh_cnt = np.where(use_d, d_cnt, np.where(use_e, e_cnt, nf_cnt))
        dead = nh <= 0
        h, h_org, h_cnt = np.where(dead, 0, nh), np.where(dead, zero_org, nh_org), np.where(dead, 0, nh_cnt)
        f, f_org, f_cnt = nf, nf_org, nf_cnt
        j = int(np.argmax(h))                                        # (the first column of the row's maximum)
        if h[j] > best[0] or (h[j] == best[0] and j < best[2]):
            best = (int(h[j]), i, j, int(h_org[j]), int(h_cnt[j]))
    score, i1, j1, org, cnt = best
    mask = (1 << 20) - 1
    return _finish(score, i1, j1, org >> 20, org & mask, cnt & mask, (cnt >> 20) & mask, cnt >> 40)


def _collect(rows, starts):
    out = {f: np.zeros(len(rows), np.uint32) for f in FIELDS}
    for x, (row, start) in enumerate(zip(rows, starts)):
        for f, v in zip(FIELDS, row):
            out[f][x] = v + start if f in ("sstart", "send") else v
    return out


def alignments(queries, records, pairs, scoring=BLASTN) -> dict:
    """The nine figures (uint32[n] each) of pairs (query, strand, record, start, stop)."""
    rows, starts = [], []
    for pr in pairs:
        q, strand, rec, start, stop = H._check_pair(pr, len(queries), records)
        rows.append(local_one(H._strand_codes(queries[q], strand), H._codes(records[rec])[start:stop], scoring))
        starts.append(start)
    return _collect(rows, starts)


# ---- the literal form ------------------------------------------------------------------------------------------------------------

def local_literal_one(pattern: str, text: str, scoring=BLASTN):
    """The same for a pattern and a text over ACGT and '#', which equals nothing."""
    r, p, go, ge = check_scoring(scoring)
    m, n = len(pattern), len(text)
    if m >= 1 << 16 or n >= 1 << 16:
        raise ValueError("a side of a local alignment stays below 2^16")
    inf = float("inf")
    # a cell: (value, (i0, j0, mismatch, gapopen, gaps))
    h_prev = [(0, (0, j, 0, 0, 0)) for j in range(n + 1)]
    f_prev = [(-inf, None)] * (n + 1)
    top = (0, 0, 0, None)
    for i in range(1, m + 1):
        h_row = [(0, (i, 0, 0, 0, 0))]
        f_row = [(-inf, None)]
        e_left = (-inf, None)
        for j in range(1, n + 1):
            hl, rl = h_row[j - 1]
            if e_left[0] >= hl - go:
                a, b, c, d, g = e_left[1]
                e = (e_left[0] - ge, (a, b, c, d, g + 1))
            else:
                a, b, c, d, g = rl
                e = (hl - go - ge, (a, b, c, d + 1, g + 1))
            hu, ru = h_prev[j]
            if f_prev[j][0] >= hu - go:
                a, b, c, d, g = f_prev[j][1]
                f = (f_prev[j][0] - ge, (a, b, c, d, g + 1))
            else:
                a, b, c, d, g = ru
                f = (hu - go - ge, (a, b, c, d + 1, g + 1))
            same = pattern[i - 1] == text[j - 1] and pattern[i - 1] != "#"
            a, b, c, d, g = h_prev[j - 1][1]
            diag = (h_prev[j - 1][0] + (r if same else p), (a, b, c + (0 if same else 1), d, g))
            cell = (0, (i, j, 0, 0, 0))
            for cand in (diag, e, f):
                if cand[0] > cell[0]:
                    cell = cand
            h_row.append(cell)
            f_row.append(f)
            e_left = e
            if cell[0] > top[0] or (cell[0] == top[0] and (j, i) < (top[2], top[1])):
                top = (cell[0], i, j, cell[1])
        h_prev, f_prev = h_row, f_row
    if top[0] == 0:
        return (0,) * 9
    return _finish(top[0], top[1], top[2], *top[3])


def alignments_literal(queries, records, pairs, scoring=BLASTN) -> dict:
    rows, starts = [], []
    for pr in pairs:
        q, strand, rec, start, stop = H._check_pair(pr, len(queries), records)
        pat = H._text(queries[q])
        rows.append(local_literal_one(H._rc(pat) if strand else pat, H._text(records[rec])[start:stop], scoring))
        starts.append(start)
    return _collect(rows, starts)


# ---- the checker -----------------------------------------------------------------------------------------------------------------

def check(out: dict, scoring, queries=None, records=None, pairs=None) -> None:
    """The identities of section 3.2i on every entry of the nine arrays (any shape; entries of 0xFFFFFFFF in `score` are skipped):
    the score rebuilt from the counts, rows and columns consumed, gapopen <= gaps; with the sequences, also that the first and the
    last column of the alignment are matches and that the interval lies in its window."""
    r, p, go, ge = check_scoring(scoring)
    a = {f: np.asarray(out[f]).astype(np.int64).ravel() for f in FIELDS}
    live = a["score"] != H.NONE
    rows, cols = a["qend"] - a["qstart"], a["send"] - a["sstart"]
    twice_ins = a["gaps"] + rows - cols
    assert (twice_ins[live] % 2 == 0).all() and (twice_ins[live] >= 0).all()
    ins = twice_ins // 2
    assert (a["score"] == r * a["nident"] + p * a["mismatch"] - go * a["gapopen"] - ge * a["gaps"])[live].all()
    assert (a["nident"] + a["mismatch"] + ins == rows)[live].all()
    assert (a["nident"] + a["mismatch"] + (a["gaps"] - ins) == cols)[live].all()
    assert (a["gapopen"] <= a["gaps"])[live].all() and ((a["gapopen"] == 0) == (a["gaps"] == 0))[live].all()
    zero = live & (a["score"] == 0)
    for f in ("qstart", "qend", "nident", "mismatch", "gapopen", "gaps"):
        assert (a[f][zero] == 0).all(), f
    assert (a["nident"][live & ~zero] >= 1).all()
    if pairs is None:
        return
    for x, pr in enumerate(pairs):
        q, strand, rec, start, stop = (int(v) for v in pr)
        if a["score"][x] == 0:
            assert a["sstart"][x] == a["send"][x] == start
            continue
        pat, text = H._strand_codes(queries[q], strand), H._codes(records[rec])
        assert 0 <= a["qstart"][x] < a["qend"][x] <= len(pat) and start <= a["sstart"][x] < a["send"][x] <= stop
        for i, j in ((a["qstart"][x], a["sstart"][x]), (a["qend"][x] - 1, a["send"][x] - 1)):
            assert pat[i] < 4 and pat[i] == text[j], (x, "an end column is no match")


def rescore(nident: int, ops, scoring) -> int:
    """The score of an edit script of align_host (ops 0 `=`, 1 `X`, 2 `I`, 3 `D`) under a scoring system: runs of I and of D are
    gaps of their own."""
    r, p, go, ge = check_scoring(scoring)
    total, last = 0, None
    for op in (int(o) for o in ops):
        if op == 0:
            total += r
        elif op == 1:
            total += p
        else:
            total -= ge + (go if op != last else 0)
        last = op
    return total
