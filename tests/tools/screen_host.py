"""Host restatement of the exact k-mer containment screen (the device side is seqwin_amd/csrc/screen.hip).

For every query and every assembly: how many of the query's distinct canonical k-mers occur anywhere in the assembly.

* Alphabet: ACGTU in either case, U reads as T; every other byte is invalid.
* A k-mer is a window of k valid bases inside one record (assembly side) or one query (query side); 1 <= k <= 32.
* Code A0 C1 G2 T3, first base most significant: a 2k-bit word.  The canonical k-mer is the smaller of the word and its reverse
  complement's word; a palindrome is its own partner.
* counts[q, a] = |K_q & K_a|, uint32; n_kmers[q] = |K_q|; containment = counts / n_kmers in float64, nan where n_kmers is 0.
  Multiplicity never counts.

Two forms that share nothing but this text: :func:`screen` rolls the words with NumPy (np.unique, np.isin), :func:`screen_literal`
slices Python strings, reverse-complements them with str.translate and intersects sets.  Sequences are ``str`` or ``bytes``; an
assembly is a list of records.
"""
from __future__ import annotations

import numpy as np

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def _bytes(s) -> bytes:
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def _check_k(k: int) -> None:
    if not 1 <= k <= 32:
        raise ValueError(f"k-mer length must lie in 1..32 (got {k})")


def canonical_words(seq, k: int) -> np.ndarray:
    """The canonical words of all windows of k valid bases of one sequence, in text order, repeats kept (uint64)."""
    _check_k(k)
    codes = _CODE[np.frombuffer(_bytes(seq), np.uint8)]
    n = len(codes) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    fwd = np.zeros(n, np.uint64)
    rev = np.zeros(n, np.uint64)
    bad = np.zeros(n, bool)
    for i in range(k):
        c = codes[i:i + n]
        bad |= c > 3
        c = (c & 3).astype(np.uint64)
        fwd |= c << np.uint64(2 * (k - 1 - i))              # first base most significant
        rev |= (np.uint64(3) - c) << np.uint64(2 * i)       # the complement of base i is base k - 1 - i of the other strand
    return np.minimum(fwd, rev)[~bad]


def kmer_set(seqs, k: int) -> np.ndarray:
    """Ascending distinct canonical words of a list of sequences (no window spans two of them)."""
    parts = [canonical_words(s, k) for s in seqs]
    return np.unique(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)


def screen(queries, assemblies, k: int):
    """(counts uint32[n_queries, n_assemblies], n_kmers uint32[n_queries])"""
    _check_k(k)
    k_q = [kmer_set([text], k) for text in queries]
    counts = np.zeros((len(queries), len(assemblies)), np.uint32)
    n_kmers = np.array([len(s) for s in k_q], np.uint32).reshape(len(queries))
    # one membership test per assembly, over the union of the queries' sets; a query's count is the sum over its own members
    union = np.unique(np.concatenate(k_q)) if k_q else np.zeros(0, np.uint64)
    where = [np.searchsorted(union, s) for s in k_q]
    for a, recs in enumerate(assemblies):
        present = np.isin(union, kmer_set(recs, k), assume_unique=True)
        for q, idx in enumerate(where):
            counts[q, a] = int(present[idx].sum())
    return counts, n_kmers


def containment(counts, n_kmers) -> np.ndarray:
    nk = np.asarray(n_kmers, np.float64).copy()
    nk[nk == 0] = np.nan
    return np.asarray(counts, np.float64) / nk[:, None]


# ---- the literal form ------------------------------------------------------------------------------------------------------------

_UPPER = str.maketrans("acgtuU", "ACGTTT")
_COMP = str.maketrans("ACGT", "TGCA")


def _text(s) -> str:
    return (s if isinstance(s, str) else bytes(s).decode("latin-1")).translate(_UPPER)


def kmer_set_literal(seqs, k: int) -> set:
    """The canonical k-mers of a list of sequences as strings: the smaller of a window and its reverse complement (A < C < G < T,
    which is the order of the words)."""
    _check_k(k)
    out = set()
    for s in seqs:
        t = _text(s)
        for i in range(len(t) - k + 1):
            w = t[i:i + k]
            if any(c not in "ACGT" for c in w):
                continue
            rc = w.translate(_COMP)[::-1]
            out.add(min(w, rc))
    return out


def screen_literal(queries, assemblies, k: int):
    k_a = [kmer_set_literal(recs, k) for recs in assemblies]
    counts = np.zeros((len(queries), len(assemblies)), np.uint32)
    n_kmers = np.zeros(len(queries), np.uint32)
    for q, text in enumerate(queries):
        k_q = kmer_set_literal([text], k)
        n_kmers[q] = len(k_q)
        for a, ka in enumerate(k_a):
            counts[q, a] = len(k_q & ka)
    return counts, n_kmers


def revcomp(s) -> bytes:
    """Reverse complement of an ACGT text (other bytes stay where the reversal puts them)."""
    return _bytes(s).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]
