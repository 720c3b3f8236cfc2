"""Host restatement of the best hits with seeds shared between queries (the device side is
k_hit_probe_shared and the owner lists of seqwin_amd/csrc/hits.hip).

Words, windows, canonical form, orientation, bands, vote, window and Layer A are section 3.2e's (tests/tools/hits_host.py, whose
Layer A and window helpers are imported here, not restated).  What differs is the seed rule, with the cap c in 1..256:

* mult(word) = the valid windows of ALL query text whose canonical word it is.
* A word is a seed iff 1 <= mult <= c and it is not its own reverse complement; every one of its windows (q, i, window-is-canonical)
  owns it.  A word with mult > c is dropped whole.
* n_seeds[q] = the windows of q that own a seed.
* A window of the batch whose canonical word is a seed is one hit PER OWNER, each with that owner's q, i, orientation, e and band by
  section 3.2e's formulas.  From the hits on nothing differs.

Two forms that share nothing but this text and hits_host's helpers: :func:`best_hits_shared` uses NumPy (sorted key arrays),
:func:`best_hits_shared_literal` plain Python (dicts, string slices).  Both return ``n_seeds`` and the five matrix fields of
``hits_host.FIELDS``; :func:`seed_stats` counts what the cap keeps and drops.
"""
from __future__ import annotations

import numpy as np

from hits_host import (NONE, FIELDS, _bytes, _check_k, _codes, _empty, _rc, _strand_codes, _text, _windows,  # noqa: F401
                       infix_literal_one, infix_one)


def _check_c(c: int) -> None:
    if not 1 <= c <= 256:
        raise ValueError(f"seed_copies must lie in 1..256 (got {c})")


# ---- the NumPy form --------------------------------------------------------------------------------------------------------------

def _owners(queries, k: int, c: int):
    """(seed words ascending, offsets into the owners, owners' q, i, window-is-canonical) and the counts of :func:`seed_stats`."""
    ws, qs, ps, fs, pal = [], [], [], [], []
    for q, text in enumerate(queries):
        w = _windows(text, k)
        ws.append(w[0]); qs.append(np.full(len(w[0]), q, np.int64)); ps.append(w[1]); fs.append(w[2]); pal.append(w[3])
    z = np.zeros(0, np.int64)
    stats = dict(seed_copies=c, seed_words=0, seed_windows=0, dropped_words=0, dropped_windows=0, palindromic_words=0, longest_owner_list=0)
    if not ws:
        return np.zeros(0, np.uint64), np.zeros(1, np.int64), z, z, np.zeros(0, bool), stats
    w, q_of, i_of, f_of, pal = (np.concatenate(x) for x in (ws, qs, ps, fs, pal))
    order = np.argsort(w, kind="stable")
    w, q_of, i_of, f_of, pal = w[order], q_of[order], i_of[order], f_of[order], pal[order]
    uniq, first, count = np.unique(w, return_index=True, return_counts=True)
    is_pal = pal[first] if len(first) else np.zeros(0, bool)
    keep = (count <= c) & ~is_pal
    drop = (count > c) & ~is_pal
    own = np.repeat(keep, count)                             # per sorted window: its word is a seed
    off = np.concatenate([[0], np.cumsum(count[keep])]).astype(np.int64)
    stats.update(seed_words=int(keep.sum()), seed_windows=int(count[keep].sum()), dropped_words=int(drop.sum()), dropped_windows=int(count[drop].sum()),
                 palindromic_words=int(is_pal.sum()), longest_owner_list=int(count[keep].max()) if keep.any() else 0)
    return uniq[keep], off, q_of[own], i_of[own], f_of[own], stats


def seed_stats(queries, k: int, c: int) -> dict:
    _check_k(k)
    _check_c(c)
    return _owners(queries, k, c)[5]


def best_hits_shared(queries, assemblies, k: int, c: int) -> dict:
    _check_k(k)
    _check_c(c)
    nq, na = len(queries), len(assemblies)
    out = _empty(nq, na)
    records = [r for recs in assemblies for r in recs]
    s_word, s_off, o_q, o_i, o_f, _ = _owners(queries, k, c)
    out["n_seeds"] = np.bincount(o_q, minlength=nq).astype(np.uint32)
    if not len(s_word):
        return out
    m_of = np.array([len(_bytes(t)) for t in queries], np.int64)
    r0 = 0
    for a, recs in enumerate(assemblies):
        keys = []                                            # (q, r, o, b) packed: q major, then r, o, b
        for r, rec in enumerate(recs, start=r0):
            bw, bp, bf, _ = _windows(rec, k)
            at = np.searchsorted(s_word, bw)
            at[at == len(s_word)] = 0
            hit = s_word[at] == bw
            at, bp, bf = at[hit], bp[hit], bf[hit]
            n_own = s_off[at + 1] - s_off[at]                # every hit window once per owner of its word
            rep = np.repeat(np.arange(len(at)), n_own)
            rank = np.arange(len(rep)) - np.repeat(np.cumsum(n_own) - n_own, n_own)
            ow = s_off[at][rep] + rank
            bp, bf = bp[rep], bf[rep]
            o = (bf != o_f[ow]).astype(np.int64)
            m = m_of[o_q[ow]]
            io = np.where(o == 1, m - k - o_i[ow], o_i[ow])
            e = bp - io + (m - k)
            assert (e >= 0).all()
            keys.append(((o_q[ow] << 24 | r) << 1 | o) << 30 | (e >> 6))
        r0 += len(recs)
        if not keys:
            continue
        keys = np.sort(np.concatenate(keys))
        if not len(keys):
            continue
        uk, cnt = np.unique(keys, return_counts=True)
        nxt = np.zeros(len(uk), np.int64)
        adj = np.flatnonzero(uk[1:] == uk[:-1] + 1)
        nxt[adj] = cnt[adj + 1]
        score = cnt + nxt
        uq = uk >> 55
        for q in np.unique(uq):
            sel = np.flatnonzero(uq == q)
            best = sel[np.argmax(score[sel])]                # (argmax: the first of equal scores, the smallest key)
            key = int(uk[best])
            b, o, r = key & ((1 << 30) - 1), (key >> 30) & 1, (key >> 31) & ((1 << 24) - 1)
            m = int(m_of[q])
            s0 = 64 * b - (m - k)
            lo, hi = max(0, s0 - 64), min(len(records[r]), s0 + 192 + m)
            d, j = infix_one(_strand_codes(queries[q], o), _codes(records[r])[lo:hi])
            out["seeds"][q, a], out["record"][q, a], out["strand"][q, a] = score[best], r, o
            out["dist"][q, a], out["end"][q, a] = d, lo + j
    return out


# ---- the literal form ------------------------------------------------------------------------------------------------------------

def best_hits_shared_literal(queries, assemblies, k: int, c: int) -> dict:
    _check_k(k)
    _check_c(c)
    nq, na = len(queries), len(assemblies)
    out = _empty(nq, na)
    texts = [_text(t) for t in queries]
    seen = {}                                                # canonical k-mer -> list of (q, i, window-is-canonical)
    for q, t in enumerate(texts):
        for i in range(len(t) - k + 1):
            w = t[i:i + k]
            if "#" in w:
                continue
            rc = _rc(w)
            if w != rc:                                      # (its own reverse complement: never a seed)
                seen.setdefault(min(w, rc), []).append((q, i, w < rc))
    seeds = {w: v for w, v in seen.items() if len(v) <= c}   # a word above the cap goes whole
    for v in seeds.values():
        for q, _, _ in v:
            out["n_seeds"][q] += 1
    r0 = 0
    for a, recs in enumerate(assemblies):
        votes = {}                                           # (q, r, o, b) -> hits
        for r, rec in enumerate(recs, start=r0):
            t = _text(rec)
            for p in range(len(t) - k + 1):
                w = t[p:p + k]
                if "#" in w:
                    continue
                rc = _rc(w)
                for q, i, q_canon in seeds.get(min(w, rc), ()):
                    o = 0 if (w < rc) == q_canon else 1
                    m = len(texts[q])
                    e = p - (i if o == 0 else m - k - i) + (m - k)
                    votes[(q, r, o, e >> 6)] = votes.get((q, r, o, e >> 6), 0) + 1
        best = {}
        for (q, r, o, b), n in votes.items():
            cand = (-(n + votes.get((q, r, o, b + 1), 0)), r, o, b)
            if q not in best or cand < best[q]:
                best[q] = cand
        for q, (neg, r, o, b) in best.items():
            m = len(texts[q])
            s0 = 64 * b - (m - k)
            rt = _text(recs[r - r0])
            lo, hi = max(0, s0 - 64), min(len(rt), s0 + 192 + m)
            d, j = infix_literal_one(_rc(texts[q]) if o else texts[q], rt[lo:hi])
            out["seeds"][q, a], out["record"][q, a], out["strand"][q, a] = -neg, r, o
            out["dist"][q, a], out["end"][q, a] = d, lo + j
        r0 += len(recs)
    return out
