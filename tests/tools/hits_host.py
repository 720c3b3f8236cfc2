"""Host restatement of the best hit of every query in every assembly (the device side is
seqwin_amd/csrc/hits.hip).

* Alphabet: ACGTU in either case, U reads as T; every other byte is invalid.  An invalid base equals nothing, not even another
  invalid base, and its complement is invalid.
* Layer A, a pair (query, strand, record, start, stop): the pattern P is the query (strand 0) or its reverse complement (strand 1),
  the text T is record[start:stop].  D[0][j] = 0, D[i][0] = i, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (P[i-1] !=
  T[j-1])).  dist = min over j of D[m][j]; end = start + the smallest j that attains it.
* Layer B, k in 1..32.  A k-mer is a window of k valid bases inside one record or one query; its canonical word is the smaller of
  its 2k-bit word (A0 C1 G2 T3, first base most significant) and its reverse complement's.  A canonical word is a seed iff exactly
  one window of ALL query text has it and it is not its own reverse complement; it belongs to query q at offset i.  A window of the
  batch (global record r, position p) whose canonical word is a seed is a hit with orientation o = 0 if the batch window and the
  query window are both or neither their canonical form, else 1.  With m = |q|: i' = i (o = 0) or m - k - i (o = 1), e = p - i' +
  (m - k), band b = e >> 6.  For one (q, assembly): c[r, o, b] = hits; a candidate has c > 0 and scores c[r, o, b] + c[r, o, b + 1];
  the winner has the highest score, ties to the smallest (r, o, b).  seeds = the winner's score.  s0 = 64 b - (m - k), lo = max(0,
  s0 - 64), hi = min(len(record), s0 + 192 + m); Layer A on (q, o, r, lo, hi) gives dist and end.  A pair without a hit: seeds 0,
  strand 0, record = end = dist = 0xFFFFFFFF.

Two forms that share nothing but this text: :func:`infix` / :func:`best_hits` use NumPy (a row-wise DP with a running minimum,
sorted key arrays), :func:`infix_literal` / :func:`best_hits_literal` plain Python (a cell-by-cell DP, dicts, string slices).
Sequences are ``str`` or ``bytes``; ``records`` is the flat list of the batch's records, an assembly a list of records.
"""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF
FIELDS = ("seeds", "record", "strand", "end", "dist")


def _bytes(s) -> bytes:
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def _check_k(k: int) -> None:
    if not 1 <= k <= 32:
        raise ValueError(f"k-mer length must lie in 1..32 (got {k})")


def revcomp(s) -> bytes:
    """Reverse complement of an ACGT text (other bytes stay where the reversal puts them)."""
    return _bytes(s).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def _empty(nq: int, na: int) -> dict:
    out = {f: np.full((nq, na), NONE, np.uint32) for f in FIELDS}
    out["seeds"][:] = 0
    out["strand"] = np.zeros((nq, na), np.uint8)
    out["n_seeds"] = np.zeros(nq, np.uint32)
    return out


# ---- the NumPy form --------------------------------------------------------------------------------------------------------------

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def _codes(s) -> np.ndarray:
    return _CODE[np.frombuffer(_bytes(s), np.uint8)]


def infix_one(pattern_codes: np.ndarray, text_codes: np.ndarray):
    """(dist, j) for a pattern and a text given as codes 0..3, 4 = invalid."""
    m, n = len(pattern_codes), len(text_codes)
    text = np.where(text_codes > 3, 5, text_codes)          # 5 never equals the pattern's 4
    row = np.zeros(n + 1, np.int64)
    ar = np.arange(n + 1, dtype=np.int64)
    for i in range(1, m + 1):
        t = np.empty(n + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (text != pattern_codes[i - 1]))
        row = np.minimum.accumulate(t - ar) + ar            # D[i][j] = min over j' <= j of t[j'] + (j - j')
    return int(row.min()), int(np.argmin(row))


def _strand_codes(q, strand: int) -> np.ndarray:
    c = _codes(q)
    if strand:
        c = c[::-1]
        c = np.where(c > 3, 4, 3 - c).astype(np.uint8)
    return c


def _check_pair(p, nq, records):
    q, strand, rec, start, stop = (int(x) for x in p)
    if not (0 <= q < nq and strand in (0, 1) and 0 <= rec < len(records) and 0 <= start <= stop <= len(records[rec])):
        raise ValueError(f"pair {tuple(p)} names no query, no strand or no interval of a record")
    return q, strand, rec, start, stop


def infix(queries, records, pairs):
    """(dist uint32[n], end uint32[n]) of pairs (query, strand, record, start, stop)."""
    dist = np.zeros(len(pairs), np.uint32)
    end = np.zeros(len(pairs), np.uint32)
    for x, p in enumerate(pairs):
        q, strand, rec, start, stop = _check_pair(p, len(queries), records)
        d, j = infix_one(_strand_codes(queries[q], strand), _codes(records[rec])[start:stop])
        dist[x], end[x] = d, start + j
    return dist, end


def _windows(seq, k: int):
    """(canonical word, position, window-is-canonical, window-is-its-own-reverse-complement) of every window of k valid bases."""
    codes = _codes(seq)
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, bool), np.zeros(0, bool)
    fwd = np.zeros(n, np.uint64)
    rev = np.zeros(n, np.uint64)
    bad = np.zeros(n, bool)
    for i in range(k):
        c = codes[i:i + n]
        bad |= c > 3
        c = (c & 3).astype(np.uint64)
        fwd |= c << np.uint64(2 * (k - 1 - i))
        rev |= (np.uint64(3) - c) << np.uint64(2 * i)
    ok = ~bad
    return np.minimum(fwd, rev)[ok], np.flatnonzero(ok).astype(np.int64), (fwd < rev)[ok], (fwd == rev)[ok]


def best_hits(queries, assemblies, k: int) -> dict:
    _check_k(k)
    nq, na = len(queries), len(assemblies)
    out = _empty(nq, na)
    records = [r for recs in assemblies for r in recs]
    # seeds: words with one window in all query text, not palindromic; sorted by word
    ws, qs, ps, fs, pal = [], [], [], [], []
    for q, text in enumerate(queries):
        w = _windows(text, k)
        ws.append(w[0]); qs.append(np.full(len(w[0]), q, np.int64)); ps.append(w[1]); fs.append(w[2]); pal.append(w[3])
    if not ws:
        return out
    w, q_of, i_of, f_of, pal = (np.concatenate(x) for x in (ws, qs, ps, fs, pal))
    order = np.argsort(w, kind="stable")
    w, q_of, i_of, f_of, pal = w[order], q_of[order], i_of[order], f_of[order], pal[order]
    uniq, first, count = np.unique(w, return_index=True, return_counts=True)
    keep = (count == 1) & ~pal[first]
    s_word, s_q, s_i, s_f = uniq[keep], q_of[first][keep], i_of[first][keep], f_of[first][keep]
    out["n_seeds"] = np.bincount(s_q, minlength=nq).astype(np.uint32)
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
            o = (bf != s_f[at]).astype(np.int64)
            m = m_of[s_q[at]]
            io = np.where(o == 1, m - k - s_i[at], s_i[at])
            e = bp - io + (m - k)
            assert (e >= 0).all()
            keys.append(((s_q[at] << 24 | r) << 1 | o) << 30 | (e >> 6))
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

_UPPER = str.maketrans("acgtuU", "ACGTTT")
_COMP = str.maketrans("ACGT", "TGCA")


def _text(s) -> str:
    """Upper case, U as T, every invalid byte as '#'."""
    t = (s if isinstance(s, str) else bytes(s).decode("latin-1")).translate(_UPPER)
    return "".join(c if c in "ACGT" else "#" for c in t)


def _rc(t: str) -> str:
    return t.translate(_COMP)[::-1]


def infix_literal_one(pattern: str, text: str):
    """(dist, j): pattern and text over ACGT and '#', which equals nothing."""
    m, n = len(pattern), len(text)
    prev = [0] * (n + 1)
    for i in range(1, m + 1):
        cur = [i] * (n + 1)
        pc = pattern[i - 1]
        for j in range(1, n + 1):
            same = pc == text[j - 1] and pc != "#"
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if same else 1))
        prev = cur
    d = min(prev)
    return d, prev.index(d)


def infix_literal(queries, records, pairs):
    dist = np.zeros(len(pairs), np.uint32)
    end = np.zeros(len(pairs), np.uint32)
    for x, p in enumerate(pairs):
        q, strand, rec, start, stop = _check_pair(p, len(queries), records)
        pat = _text(queries[q])
        d, j = infix_literal_one(_rc(pat) if strand else pat, _text(records[rec])[start:stop])
        dist[x], end[x] = d, start + j
    return dist, end


def best_hits_literal(queries, assemblies, k: int) -> dict:
    _check_k(k)
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
            seen.setdefault(min(w, rc), []).append((q, i, w < rc, w == rc))
    seeds = {w: v[0] for w, v in seen.items() if len(v) == 1 and not v[0][3]}
    for q, _, _, _ in seeds.values():
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
                s = seeds.get(min(w, rc))
                if s is None:
                    continue
                q, i, q_canon, _ = s
                o = 0 if (w < rc) == q_canon else 1
                m = len(texts[q])
                e = p - (i if o == 0 else m - k - i) + (m - k)
                votes[(q, r, o, e >> 6)] = votes.get((q, r, o, e >> 6), 0) + 1
        r0 += len(recs)
        best = {}
        for (q, r, o, b), c in votes.items():
            cand = (-(c + votes.get((q, r, o, b + 1), 0)), r, o, b)
            if q not in best or cand < best[q]:
                best[q] = cand
        recs_text = None
        for q, (neg, r, o, b) in best.items():
            m = len(texts[q])
            s0 = 64 * b - (m - k)
            if recs_text is None:
                recs_text = {}
            if r not in recs_text:
                recs_text[r] = _text(recs[r - (r0 - len(recs))])
            lo, hi = max(0, s0 - 64), min(len(recs_text[r]), s0 + 192 + m)
            d, j = infix_literal_one(_rc(texts[q]) if o else texts[q], recs_text[r][lo:hi])
            out["seeds"][q, a], out["record"][q, a], out["strand"][q, a] = -neg, r, o
            out["dist"][q, a], out["end"][q, a] = d, lo + j
    return out
