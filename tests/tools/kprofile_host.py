"""Host restatement of the k-mer profile (the device side is seqwin_amd/csrc/screen.hip).

For every byte position p of the query text and every group g of assemblies:

* Alphabet, k (1..32), windows and canonical k-mers are the screen's (section 3.2d): ACGTU in either case, U reads as T, every other
  byte is invalid; a window is k valid bases inside one record or one query; the canonical k-mer is the smaller of the window and its
  reverse complement (A < C < G < T); a palindrome is its own partner.
* Groups: one label per assembly, 0 .. n_groups - 1 with n_groups in 1..8 (None: the largest label + 1), 255 leaves the assembly
  out, a label in n_groups..254 is a ValueError.
* present[p, g] (uint32) = the assemblies labelled g that hold the canonical k-mer of the window starting at p in at least one valid
  window of any record.
* copies[p, g] (uint64) = the valid windows of those assemblies whose canonical k-mer equals it: a window counts once, whatever its
  strand.
* A row where no query window starts (the last k - 1 bytes of a query, a window with an invalid byte, a query shorter than k) reads
  0xFFFFFFFF in present and 0xFFFFFFFFFFFFFFFF in copies, in every group.
* group_sizes[g] = the assemblies labelled g.

Two forms that share nothing but this text: :func:`profile_literal` slices Python strings, reverse-complements them with
str.translate and counts with sets and collections.Counter per assembly; :func:`profile_words` packs 2k-bit words with NumPy
(np.unique, np.searchsorted, np.add.at).  Sequences are ``str`` or ``bytes``; an assembly is a list of records.  Both return
``(offsets uint64[n + 1], present uint32[total, groups], copies uint64[total, groups], group_sizes uint32[groups])``.

The functions below the two forms restate seqwin_amd/kprofile.py with plain loops.
"""
from __future__ import annotations

import math
from collections import Counter

import numpy as np

NO_WINDOW = 0xFFFFFFFF
NO_WINDOW_COPIES = 0xFFFFFFFFFFFFFFFF
LEAVE_OUT = 255


def _check(k, labels, n_assemblies, n_groups):
    if not 1 <= k <= 32:
        raise ValueError(f"k-mer length must lie in 1..32 (got {k})")
    labels = [int(x) for x in labels]
    if len(labels) != n_assemblies:
        raise ValueError(f"one label per assembly: {n_assemblies} (got {len(labels)})")
    kept = [x for x in labels if x != LEAVE_OUT]
    if n_groups is None:
        n_groups = max(kept) + 1 if kept else 1
    if not 1 <= n_groups <= 8:
        raise ValueError(f"1..8 groups (got {n_groups})")
    if any(not 0 <= x < n_groups for x in kept):
        raise ValueError("a label is neither below n_groups nor 255")
    return labels, int(n_groups)


# ---- the literal form ------------------------------------------------------------------------------------------------------------

_UPPER = str.maketrans("acgtuU", "ACGTTT")
_COMP = str.maketrans("ACGT", "TGCA")


def _text(s) -> str:
    return (s if isinstance(s, str) else bytes(s).decode("latin-1")).translate(_UPPER)


def _canonical(window: str):
    """The canonical k-mer of a window, None if it holds a byte outside ACGT."""
    if any(c not in "ACGT" for c in window):
        return None
    rc = window.translate(_COMP)[::-1]
    return min(window, rc)


def profile_literal(queries, assemblies, k: int, labels, n_groups=None):
    labels, ng = _check(k, labels, len(assemblies), n_groups)
    counters = []
    for recs in assemblies:
        c = Counter()
        for rec in recs:
            t = _text(rec)
            for i in range(len(t) - k + 1):
                w = _canonical(t[i:i + k])
                if w is not None:
                    c[w] += 1
        counters.append(c)
    lens = [len(q) for q in queries]
    offsets = np.zeros(len(queries) + 1, np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64) if lens else 0
    total = int(offsets[-1])
    present = np.full((total, ng), NO_WINDOW, np.uint32)
    copies = np.full((total, ng), NO_WINDOW_COPIES, np.uint64)
    for q, text in enumerate(queries):
        t = _text(text)
        for u in range(len(t) - k + 1):
            w = _canonical(t[u:u + k])
            if w is None:
                continue
            row = int(offsets[q]) + u
            present[row] = 0
            copies[row] = 0
            for a, c in enumerate(counters):
                if labels[a] != LEAVE_OUT and w in c:
                    present[row, labels[a]] += 1
                    copies[row, labels[a]] += np.uint64(c[w])
    sizes = np.array([sum(1 for x in labels if x == g) for g in range(ng)], np.uint32).reshape(ng)
    return offsets, present, copies, sizes


# ---- the word form ---------------------------------------------------------------------------------------------------------------

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def _words(seq, k: int):
    """(canonical words uint64[n], valid bool[n]) of the n = len - k + 1 windows of one sequence (n <= 0: empty)."""
    raw = seq.encode("utf-8") if isinstance(seq, str) else bytes(seq)
    codes = _CODE[np.frombuffer(raw, np.uint8)]
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    fwd = np.zeros(n, np.uint64)
    rev = np.zeros(n, np.uint64)
    valid = np.ones(n, bool)
    for i in range(k):
        c = codes[i:i + n]
        valid &= c < 4
        c = (c & 3).astype(np.uint64)
        fwd = (fwd << np.uint64(2)) | c
        rev |= (np.uint64(3) - c) << np.uint64(2 * i)
    return np.where(fwd < rev, fwd, rev), valid


def profile_words(queries, assemblies, k: int, labels, n_groups=None):
    labels, ng = _check(k, labels, len(assemblies), n_groups)
    offsets = np.zeros(len(queries) + 1, np.uint64)
    q_words, q_rows = [], []
    for q, text in enumerate(queries):
        n = len(text.encode("utf-8") if isinstance(text, str) else bytes(text))
        offsets[q + 1] = offsets[q] + np.uint64(n)
        w, ok = _words(text, k)
        q_words.append(w[ok])
        q_rows.append(int(offsets[q]) + np.flatnonzero(ok))
    total = int(offsets[-1])
    present = np.full((total, ng), NO_WINDOW, np.uint32)
    copies = np.full((total, ng), NO_WINDOW_COPIES, np.uint64)
    sizes = np.bincount(np.array([x for x in labels if x != LEAVE_OUT], np.int64), minlength=ng).astype(np.uint32)
    words = np.concatenate(q_words) if q_words else np.zeros(0, np.uint64)
    rows = np.concatenate(q_rows).astype(np.int64) if q_rows else np.zeros(0, np.int64)
    distinct, inverse = np.unique(words, return_inverse=True)
    n_asm_with = np.zeros((len(distinct), ng), np.uint32)
    n_windows = np.zeros((len(distinct), ng), np.uint64)
    for a, recs in enumerate(assemblies):
        if labels[a] == LEAVE_OUT:
            continue
        tally = np.zeros(len(distinct), np.uint64)
        for rec in recs:
            w, ok = _words(rec, k)
            w = w[ok]
            at = np.searchsorted(distinct, w)
            hit = at < len(distinct)
            hit[hit] = distinct[at[hit]] == w[hit]
            np.add.at(tally, at[hit], np.uint64(1))
        n_asm_with[:, labels[a]] += (tally > 0).astype(np.uint32)
        n_windows[:, labels[a]] += tally
    present[rows] = n_asm_with[inverse.reshape(-1)]
    copies[rows] = n_windows[inverse.reshape(-1)]
    return offsets, present, copies, sizes


# ---- seqwin_amd/kprofile.py, restated with loops ---------------------------------------------------------------------------------

def fraction(present, group_sizes):
    present = np.asarray(present)
    out = np.full(present.shape, np.nan)
    for p in range(present.shape[0]):
        for g in range(present.shape[1]):
            if int(present[p, g]) != NO_WINDOW and int(group_sizes[g]) != 0:
                out[p, g] = int(present[p, g]) / int(group_sizes[g])
    return out


def window_bounds(offsets, present, k: int, length: int):
    present = np.asarray(present)
    out = np.full(present.shape, NO_WINDOW, np.uint32)
    for q in range(len(offsets) - 1):
        lo, hi = int(offsets[q]), int(offsets[q + 1])
        for p in range(lo, hi - length + 1):
            covered = present[p:p + length - k + 1]
            if (covered == NO_WINDOW).any():
                continue
            out[p] = covered.min(axis=0)
    return out


def specific_positions(present, group_sizes, tar=0, neg=1, min_tar=0.95, max_neg=0.05):
    f = fraction(present, group_sizes)
    rows = []
    for p in range(len(f)):
        if int(present[p, tar]) == NO_WINDOW or math.isnan(f[p, tar]):
            continue
        f_neg = 0.0 if math.isnan(f[p, neg]) else f[p, neg]
        if f[p, tar] >= min_tar and f_neg <= max_neg:
            rows.append(p)
    return np.array(rows, np.int64)


def repeat_positions(present, copies, group, min_mean_copies=2.0):
    rows = []
    for p in range(len(present)):
        n = int(present[p, group])
        if n == NO_WINDOW or n == 0:
            continue
        if int(copies[p, group]) / n >= min_mean_copies:
            rows.append(p)
    return np.array(rows, np.int64)


def count_exact(window, assemblies, labels, n_groups):
    """Per group: the assemblies that hold ``window`` (ACGT text) or its reverse complement as a substring of a record, by str.find."""
    w = _text(window)
    rc = w.translate(_COMP)[::-1]
    out = [0] * n_groups
    for a, recs in enumerate(assemblies):
        if labels[a] == LEAVE_OUT:
            continue
        if any(w in _text(r) or rc in _text(r) for r in recs):
            out[labels[a]] += 1
    return out
