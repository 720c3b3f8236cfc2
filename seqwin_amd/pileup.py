"""Reading a pileup (:class:`seqwin_amd.device.Pileup`): consensus, match fraction and the positions that
tell targets from non-targets.  Pure NumPy on the exported table; nothing here touches a device.

The names are deliberately not those of the reference's ``MarkerMetrics``: these are counts over the canonical alignment of every
assembly's best hit to the query alone -- no BLAST, no multiple alignment, no conservation or divergence score of Seqwin's.
"""
from __future__ import annotations

import numpy as np

A, C, G, T, N, DEL, INS, INS_BASES = range(8)
_COLUMN = "ACGTN-"                                  # the six classes of a column; their sum is the depth
_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def consensus(counts_g) -> str:
    """One character per position of ``counts_g`` (``[m, 8]``, one query and one group): the largest of the six column classes, a
    tie going to the smaller class; ``-`` for DEL, ``N`` for N, ``.`` where the depth is 0.  Insertions are not rendered."""
    c = np.asarray(counts_g)
    if c.ndim != 2 or c.shape[1] != 8:
        raise ValueError(f"consensus takes the [m, 8] counts of one query and one group (got shape {c.shape})")
    col = c[:, :6]
    best = np.argmax(col, axis=1)                   # (the first of equal maxima: the smaller class)
    chars = np.frombuffer(_COLUMN.encode(), np.uint8)[best]
    chars = np.where(col.sum(axis=1) == 0, ord("."), chars).astype(np.uint8)
    return chars.tobytes().decode()


def _table_of(pile):
    """(offsets int64, table) of a Pileup or of its ``table()``."""
    offs, tab = pile.table() if hasattr(pile, "table") else pile
    return np.asarray(offs).astype(np.int64), np.asarray(tab)


def _query_codes(queries, offs) -> np.ndarray:
    qs = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
    if len(qs) != len(offs) - 1 or any(len(q) != offs[i + 1] - offs[i] for i, q in enumerate(qs)):
        raise ValueError("the queries are not those of the pileup's call")
    return _CODE[np.frombuffer(b"".join(qs), np.uint8)]


def match_fraction(pile, queries) -> np.ndarray:
    """float64[total, groups]: per position and group, the share of the depth whose text base is the query's own --
    ``T[u][g][code(query[u])] / depth``; nan where the depth is 0 or the query's base is none of ACGTU."""
    offs, tab = _table_of(pile)
    codes = _query_codes(queries, offs)
    depth = tab[:, :, :6].sum(axis=2, dtype=np.int64)
    valid = codes < 4
    own = np.take_along_axis(tab[:, :, :4], np.where(valid, codes, 0)[:, None, None].astype(np.int64), axis=2)[:, :, 0]
    out = np.full(depth.shape, np.nan)
    ok = (depth > 0) & valid[:, None]
    out[ok] = own[ok] / depth[ok]
    return out


def diagnostic_positions(pile, queries, tar: int = 0, neg: int = 1, min_tar: float = 0.95, max_neg: float = 0.05) -> np.ndarray:
    """Rows of the table (``offsets[q] + u``) whose query base is matched by at least ``min_tar`` of group ``tar``'s hits and by at
    most ``max_neg`` of group ``neg``'s: where a primer's 3' end or a probe tells the two apart.  A position without depth in
    either group, or with an invalid query base, is none."""
    f = match_fraction(pile, queries)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((f[:, tar] >= min_tar) & (f[:, neg] <= max_neg))
