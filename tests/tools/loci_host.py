"""Host restatement of all seeded loci of every query in every assembly (the device side is the loci mode
of seqwin_amd/csrc/hits.hip).  Nothing in the reference computes this quantity; this file is its yardstick.

Everything up to the candidates is section 3.2e (tests/tools/hits_host.py): seeds, hits, e, the band b = e >> 6, the counts
c[r, o, b] of one (query, assembly), the candidates c > 0 and the score s(r, o, b) = c[r, o, b] + c[r, o, b + 1].

* Locus.  A candidate x = (r, o, b) of query q is a locus iff s(x) >= min_seeds (min_seeds >= 1) and, for every candidate
  y = (r, o, b') of the same q with 1 <= |b' - b| <= 2: s(y) < s(x), or s(y) == s(x) and b' > b.
* Per locus: seeds = s(x), record = r, strand = o; the window of section 3.2e (s0 = 64 b - (m - k), lo = max(0, s0 - 64),
  hi = min(len(record), s0 + 192 + m)); Layer A on (q, o, r, lo, hi) gives dist and end, the canonical traceback of section 3.2f
  start, nident, mismatch and gaps.
* The list ascends by (q, r, o, b) -- records ascend with assemblies, so that is (q, assembly, r, o, b).
* Locus j is a duplicate (dup = 1) iff locus j - 1 has the same query, record, strand, start and end.
* Per cell (q, a): n_loci = its loci that are no duplicates, sum_nident = the sum of their nident; 0 where there is none.

Two forms that share nothing but this text and the two files they build on: :func:`best_hits_loci` uses NumPy (sorted key arrays,
shifted comparisons, hits_host.infix_one / align_host.align_one), :func:`best_hits_loci_literal` plain Python (dicts of votes, a
look at every band b - 2 .. b + 2, hits_host.infix_literal_one / align_host.align_literal_one).  Both return a dict of the list as
parallel arrays (LIST_FIELDS, and the windows as `lo` / `hi`), `cell_offsets` uint64[nq * na + 1], `n_loci` / `sum_nident`
uint32[nq, na], and `n_candidates`, the candidates of all cells (at min_seeds = 1 those that are no locus were suppressed).
"""
from __future__ import annotations

import numpy as np

import align_host as A
import hits_host as H

LIST_FIELDS = ("query", "assembly", "record", "strand", "band", "seeds", "dist", "end", "start", "nident", "mismatch", "gaps", "dup")
_BYTE_FIELDS = ("strand", "dup")


def _check_min_seeds(min_seeds: int) -> None:
    if int(min_seeds) < 1:
        raise ValueError(f"min_seeds must be at least 1 (got {min_seeds})")


def _arrays(rows) -> dict:
    """rows: tuples (q, a, r, o, b, seeds, dist, end, start, nident, mismatch, gaps, lo, hi) in the list's order, as arrays."""
    cols = list(zip(*rows)) if rows else [[] for _ in range(14)]
    return {name: np.array(col, np.uint8 if name in _BYTE_FIELDS else np.uint32) for name, col in zip(LIST_FIELDS[:12] + ("lo", "hi"), cols)}


def _finish_literal(rows, nq: int, na: int) -> dict:
    out = _arrays(rows)
    dup = np.zeros(len(rows), np.uint8)
    for j in range(1, len(rows)):
        dup[j] = all(rows[j][f] == rows[j - 1][f] for f in (0, 2, 3, 7, 8))
    out["dup"] = dup
    per_cell = [0] * (nq * na)
    n_loci = np.zeros((nq, na), np.uint32)
    sum_nident = np.zeros((nq, na), np.uint32)
    for j, row in enumerate(rows):
        per_cell[row[0] * na + row[1]] += 1
        if not dup[j]:
            n_loci[row[0], row[1]] += 1
            sum_nident[row[0], row[1]] += row[9]
    offs = np.zeros(nq * na + 1, np.uint64)
    for c, n in enumerate(per_cell):
        offs[c + 1] = offs[c] + np.uint64(n)
    out["cell_offsets"], out["n_loci"], out["sum_nident"] = offs, n_loci, sum_nident
    return out


def _finish_numpy(rows, nq: int, na: int) -> dict:
    out = _arrays(rows)
    same = np.ones(max(len(rows) - 1, 0), bool)
    for f in ("query", "record", "strand", "start", "end"):
        same &= out[f][1:] == out[f][:-1]
    out["dup"] = np.concatenate([np.zeros(min(len(rows), 1), bool), same]).astype(np.uint8)
    cell = out["query"].astype(np.int64) * na + out["assembly"].astype(np.int64)
    out["cell_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=nq * na))]).astype(np.uint64)
    first = out["dup"] == 0
    out["n_loci"] = np.bincount(cell[first], minlength=nq * na).astype(np.uint32).reshape(nq, na)
    out["sum_nident"] = np.bincount(cell[first], weights=out["nident"][first], minlength=nq * na).astype(np.uint32).reshape(nq, na)
    return out


# ---- the NumPy form --------------------------------------------------------------------------------------------------------------

_BAND_BITS, _REC_BITS = 30, 24


def best_hits_loci(queries, assemblies, k: int, min_seeds: int = 1) -> dict:
    H._check_k(k)
    _check_min_seeds(min_seeds)
    nq, na = len(queries), len(assemblies)
    records = [r for recs in assemblies for r in recs]
    ws = [H._windows(text, k) for text in queries]
    rows = []
    n_candidates = 0
    if ws and sum(len(w[0]) for w in ws):
        w = np.concatenate([x[0] for x in ws])
        q_of = np.concatenate([np.full(len(x[0]), q, np.int64) for q, x in enumerate(ws)])
        i_of = np.concatenate([x[1] for x in ws])
        f_of = np.concatenate([x[2] for x in ws])
        uniq, first, count = np.unique(w, return_index=True, return_counts=True)
        s_word, s_q, s_i, s_f = uniq[count == 1], q_of[first][count == 1], i_of[first][count == 1], f_of[first][count == 1]
        pal = np.concatenate([x[3] for x in ws])[first][count == 1]
        s_word, s_q, s_i, s_f = s_word[~pal], s_q[~pal], s_i[~pal], s_f[~pal]
        m_of = np.array([len(H._bytes(t)) for t in queries], np.int64)
        r0 = 0
        for a, recs in enumerate(assemblies):
            keys = [np.zeros(0, np.int64)]
            for r, rec in enumerate(recs, start=r0):
                if not len(s_word):
                    break
                bw, bp, bf, _ = H._windows(rec, k)
                at = np.searchsorted(s_word, bw)
                at[at == len(s_word)] = 0
                hit = s_word[at] == bw
                at, bp, bf = at[hit], bp[hit], bf[hit]
                o = (bf != s_f[at]).astype(np.int64)
                m = m_of[s_q[at]]
                e = bp - np.where(o == 1, m - k - s_i[at], s_i[at]) + (m - k)
                keys.append(((s_q[at] << _REC_BITS | r) << 1 | o) << _BAND_BITS | (e >> 6))
            r0 += len(recs)
            uk, cnt = np.unique(np.concatenate(keys), return_counts=True)
            if not len(uk):
                continue
            n_candidates += len(uk)
            band, grp = uk & ((1 << _BAND_BITS) - 1), uk >> _BAND_BITS
            score = cnt.astype(np.int64)
            nxt = np.flatnonzero((grp[1:] == grp[:-1]) & (band[1:] == band[:-1] + 1))
            score[nxt] += cnt[nxt + 1]
            keep = score >= min_seeds
            for s in (1, 2):                                     # distinct ascending keys: a band within 2 lies within 2 places
                near = (grp[s:] == grp[:-s]) & (band[s:] - band[:-s] <= 2)
                keep[:-s] &= ~(near & (score[s:] > score[:-s]))  # the smaller band loses to a strictly larger score only
                keep[s:] &= ~(near & (score[:-s] >= score[s:]))  # the larger band loses a tie as well
            for x in np.flatnonzero(keep):
                b, g = int(band[x]), int(grp[x])
                o, r, q = g & 1, (g >> 1) & ((1 << _REC_BITS) - 1), g >> (1 + _REC_BITS)
                m = int(m_of[q])
                s0 = 64 * b - (m - k)
                lo, hi = max(0, s0 - 64), min(len(records[r]), s0 + 192 + m)
                pc, tc = H._strand_codes(queries[q], o), H._codes(records[r])[lo:hi]
                d, js, j0, ni, nx, ng, _ = A.align_one(pc, tc)
                assert (d, js) == H.infix_one(pc, tc)
                rows.append((q, a, r, o, b, int(score[x]), d, lo + js, lo + j0, ni, nx, ng, lo, hi))
    order = np.lexsort([[row[f] for row in rows] for f in (4, 3, 2, 0)]) if rows else []
    out = _finish_numpy([rows[x] for x in order], nq, na)
    out["n_candidates"] = np.uint64(n_candidates)
    return out


# ---- the literal form ------------------------------------------------------------------------------------------------------------

def best_hits_loci_literal(queries, assemblies, k: int, min_seeds: int = 1) -> dict:
    H._check_k(k)
    _check_min_seeds(min_seeds)
    nq, na = len(queries), len(assemblies)
    texts = [H._text(t) for t in queries]
    seen = {}                                                # canonical k-mer -> list of (q, i, window-is-canonical, palindrome)
    for q, t in enumerate(texts):
        for i in range(len(t) - k + 1):
            w = t[i:i + k]
            if "#" in w:
                continue
            rc = H._rc(w)
            seen.setdefault(min(w, rc), []).append((q, i, w < rc, w == rc))
    seeds = {w: v[0] for w, v in seen.items() if len(v) == 1 and not v[0][3]}
    rows = []
    n_candidates = 0
    r0 = 0
    for a, recs in enumerate(assemblies):
        votes = {}                                           # (q, r, o, b) -> hits
        rec_text = {}
        for r, rec in enumerate(recs, start=r0):
            t = rec_text[r] = H._text(rec)
            for p in range(len(t) - k + 1):
                w = t[p:p + k]
                if "#" in w:
                    continue
                rc = H._rc(w)
                s = seeds.get(min(w, rc))
                if s is None:
                    continue
                q, i, q_canon, _ = s
                o = 0 if (w < rc) == q_canon else 1
                m = len(texts[q])
                e = p - (i if o == 0 else m - k - i) + (m - k)
                votes[(q, r, o, e >> 6)] = votes.get((q, r, o, e >> 6), 0) + 1
        r0 += len(recs)

        def score(q, r, o, b):
            return votes[(q, r, o, b)] + votes.get((q, r, o, b + 1), 0)

        n_candidates += len(votes)
        for (q, r, o, b) in votes:
            s = score(q, r, o, b)
            if s < min_seeds:
                continue
            beaten = False
            for b2 in (b - 2, b - 1, b + 1, b + 2):
                if (q, r, o, b2) not in votes:
                    continue
                s2 = score(q, r, o, b2)
                if not (s2 < s or (s2 == s and b2 > b)):
                    beaten = True
            if beaten:
                continue
            m = len(texts[q])
            s0 = 64 * b - (m - k)
            lo, hi = max(0, s0 - 64), min(len(rec_text[r]), s0 + 192 + m)
            pat = H._rc(texts[q]) if o else texts[q]
            d, js, j0, ni, nx, ng, _ = A.align_literal_one(pat, rec_text[r][lo:hi])
            assert (d, js) == H.infix_literal_one(pat, rec_text[r][lo:hi])
            rows.append((q, a, r, o, b, s, d, lo + js, lo + j0, ni, nx, ng, lo, hi))
    rows.sort(key=lambda row: (row[0], row[2], row[3], row[4]))
    out = _finish_literal(rows, nq, na)
    out["n_candidates"] = np.uint64(n_candidates)
    return out
