"""Host restatement of csrc/seqs.hip: the interval fetch and the interval edit distance.

Fetch: the record's text in upper case (what utils.load_fasta keeps), sliced [start:stop], every letter that is not A, C, G or T
written as N; inexact iff such a letter lies inside.  (The library also takes U as T; the restatement is not asked about U.)

Distance: the plain O(|R| |S|) dynamic programme of the Levenshtein distance, one row of the table at a time in NumPy, over the
symbols A, C, G, T; every other letter is invalid: it equals nothing, not even itself, and so does its complement.
dist = min(d(R, S), d(R, revcomp(S))), strand = 0 if the forward one is not larger.
"""
from __future__ import annotations

import gzip
from pathlib import Path

import numpy as np

_VALID = np.zeros(256, bool)
_VALID[list(b"ACGT")] = True
_COMP = np.full(256, ord("N"), np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def read_records(path) -> list:
    """The records of a FASTA file (.gz: gzip) as upper-case str, in file order."""
    path = Path(path)
    text = gzip.decompress(path.read_bytes()).decode() if path.suffix == ".gz" else path.read_text()
    out = []
    for rec in text.split(">")[1:]:
        eol = rec.find("\n")
        out.append("" if eol < 0 else rec[eol:].replace("\n", "").replace("\r", "").upper())
    return out


def fetch(text: str, start: int, stop: int):
    """(the interval as the library writes it, inexact)"""
    raw = np.frombuffer(text[start:stop].upper().encode("latin-1"), np.uint8)
    ok = _VALID[raw]
    return np.where(ok, raw, ord("N")).astype(np.uint8).tobytes().decode("ascii"), bool((~ok).any())


def _codes(s) -> np.ndarray:
    if isinstance(s, str):
        s = s.encode("latin-1")
    return np.frombuffer(bytes(s), np.uint8)


def levenshtein(r, s) -> int:
    """d(R, S): substitution, insertion, deletion cost 1 each, both consumed whole; an invalid letter matches nothing."""
    r, s = _codes(r), _codes(s)
    if len(r) == 0 or len(s) == 0:
        return len(r) + len(s)
    valid_s = _VALID[s]
    idx = np.arange(len(s) + 1, dtype=np.int64)
    prev = idx.copy()                                    # row 0: D[0][j] = j
    for i in range(1, len(r) + 1):
        neq = np.ones(len(s), np.int64)
        if _VALID[r[i - 1]]:
            neq[(s == r[i - 1]) & valid_s] = 0
        cur = np.empty(len(s) + 1, np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + neq, prev[1:] + 1)   # diagonal, from above
        # from the left: cur[j] = min over j' <= j of cur[j'] + (j - j')
        cur = np.minimum.accumulate(cur - idx) + idx
        prev = cur
    return int(prev[-1])


def revcomp(s) -> bytes:
    return _COMP[_codes(s)][::-1].tobytes()


def distance(r, s):
    """(dist, strand) of the specification."""
    r, s = _codes(r), _codes(s)
    if len(r) == 0 or len(s) == 0:
        return len(r) + len(s), 0
    f, v = levenshtein(r, s), levenshtein(r, revcomp(s))
    return (f, 0) if f <= v else (v, 1)


def save_block(cks_rows, record_ids) -> tuple:
    """The two files of markers.get_markers' saving block (markers.py:777-802) as text, restated: cks_rows = one tuple
    (assembly_idx, record_idx, start, stop, seq, length, rep_ratio, n_kmers) per candidate; the metric fields are empty."""
    fasta, lines = [], ["fasta_header,length,conservation,f_tar_hits,divergence,f_neg_hits,avg_repeats_tar,avg_pident_tar,"
                        "avg_repeats_neg,avg_pident_neg,rep_ratio,n_nodes"]
    for a, r, start, stop, seq, length, ratio, n_kmers in cks_rows:
        header = f"{a}-{record_ids[a][r]}-{start}:{stop}"
        fasta.append(f">{header}\n{seq}\n")
        lines.append(f"{header},{length},,,,,,,,,{ratio!r},{n_kmers}")
    return "".join(fasta), "\n".join(lines) + "\n"
