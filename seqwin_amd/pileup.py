"""Reading a pileup (:class:`seqwin_amd.device.Pileup`): consensus, match fraction and the positions that
tell targets from non-targets; and reading the oligo windows (:class:`seqwin_amd.device.Windows`, section 3.2l): the share of a class
and the windows that serve as oligos.  Pure NumPy on the exported tables; nothing here touches a device.

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


# ---- oligo windows (:class:`seqwin_amd.device.Windows`) ----------------------------------------------------

MM0, MM1, MM2, MM3, MM4P, GAPPED, FWD_OK, REV_OK = range(8)
CANDIDATE_DTYPE = np.dtype([("query", np.uint32), ("start", np.uint32), ("length", np.uint32), ("orientation", "U1"), ("f_tar", np.float64),
                            ("f_neg", np.float64)])
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def _windows_of(w):
    """(offsets int64, lengths, table [total, lengths, groups, 8]) of a Windows or of ``(offsets, lengths, table)``."""
    if hasattr(w, "table"):
        offs, tab = w.table()
        lengths = w.lengths
    else:
        offs, lengths, tab = w
    tab = np.asarray(tab)
    if tab.ndim != 4 or tab.shape[1] != len(lengths) or tab.shape[3] != 8:
        raise ValueError(f"a window table is [total, lengths, groups, 8] (got shape {tab.shape} for {len(lengths)} lengths)")
    return np.asarray(offs).astype(np.int64), tuple(int(x) for x in lengths), tab


def _depth_rows(pile, offs, n_groups) -> np.ndarray:
    """int64[total, groups]: the depth of its query at every row -- from a Pileup, its ``table()`` (the six column classes add up to
    it at every position) or a ``[queries, groups]`` array of depths."""
    if hasattr(pile, "depth"):
        depth = np.asarray(pile.depth())
    elif isinstance(pile, tuple):
        return _table_of(pile)[1][:, :, :6].sum(axis=2, dtype=np.int64)
    else:
        depth = np.asarray(pile)
    if depth.shape != (len(offs) - 1, n_groups):
        raise ValueError(f"the depths are not those of the windows' call: shape {depth.shape}, not {(len(offs) - 1, n_groups)}")
    return np.repeat(depth.astype(np.int64), np.diff(offs), axis=0)


def window_fraction(w, pile, cls: int) -> np.ndarray:
    """float64[total, lengths, groups]: per window start, window length and group, the share of the depth that is of class ``cls`` --
    ``W[u][l][g][cls] / depth``; nan where the depth is 0.  A row behind the last window of its query (u > m - L) reads 0."""
    offs, _, tab = _windows_of(w)
    depth = _depth_rows(pile, offs, tab.shape[2])[:, None, :]
    out = np.full(tab.shape[:3], np.nan)
    ok = np.broadcast_to(depth > 0, out.shape)
    out[ok] = (tab[..., int(cls)] / np.where(depth > 0, depth, 1))[ok]
    return out


def candidate_oligos(w, pile, queries, tar: int = 0, neg: int = 1, min_tar: float = 0.95, max_neg: float = 0.05, orientation: str = "both"):
    """``(candidates, oligos)``: the windows that at least ``min_tar`` of group ``tar``'s piled hits and at most ``max_neg`` of group
    ``neg``'s serve as an oligo -- ``FWD_OK`` for the window itself (orientation ``"F"``), ``REV_OK`` for its reverse complement
    (``"R"``); ``orientation`` is ``"forward"``, ``"reverse"`` or ``"both"``.  ``candidates`` is a structured array of (query, start,
    length, orientation, f_tar, f_neg) in the table's order, ``oligos`` the list of their strings, a reverse oligo reverse-complemented:
    ready for ``Batch.oligo_hits``.  A window whose query text has a letter outside ACGT is dropped, and so is one without depth in
    group ``tar``.  Without depth in group ``neg`` -- in ``best_hits`` a non-target that shares no seed with the query is no pair at
    all, so a signature that no non-target holds has depth 0 there -- ``f_neg`` is 0 and the window stays: no non-target serves it.
    (``window_fraction`` reads nan there, and ``diagnostic_positions`` drops such a position.)

    What this is NOT: a non-target is seen here only at its best locus for the whole query, aligned to the query alone.  Whether an
    oligo binds anywhere else in a non-target (or a target) -- off-locus binding -- this table cannot say; that is what the
    exhaustive ``oligo_hits`` confirmation of the candidates is for.  No Tm, no dG, no dimers: not a thermodynamic model."""
    if orientation not in ("forward", "reverse", "both"):
        raise ValueError(f"orientation is 'forward', 'reverse' or 'both' (got {orientation!r})")
    offs, lengths, tab = _windows_of(w)
    if not (0 <= int(tar) < tab.shape[2] and 0 <= int(neg) < tab.shape[2]):
        raise ValueError(f"groups {tar} and {neg} are not both among the table's {tab.shape[2]}")
    qs = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
    if len(qs) != len(offs) - 1 or any(len(q) != offs[i + 1] - offs[i] for i, q in enumerate(qs)):
        raise ValueError("the queries are not those of the windows' call")
    text = b"".join(qs)
    acgt = np.isin(np.frombuffer(text, np.uint8), np.frombuffer(b"ACGT", np.uint8))
    bad_before = np.concatenate(([0], np.cumsum(~acgt)))
    q_of_row = np.repeat(np.arange(len(qs)), np.diff(offs))
    rows = np.arange(len(text))
    found = []
    for o, cls in (("F", FWD_OK), ("R", REV_OK)):
        if orientation != "both" and orientation[0].upper() != o:
            continue
        f = window_fraction((offs, lengths, tab), pile, cls)
        f_neg = np.nan_to_num(f[:, :, neg], nan=0.0)            # no depth among the non-targets: none of them serves
        for l, L in enumerate(lengths):
            fits = rows + L <= offs[q_of_row + 1]
            clean = np.zeros(len(rows), bool)
            clean[fits] = bad_before[rows[fits] + L] == bad_before[rows[fits]]
            with np.errstate(invalid="ignore"):
                keep = np.flatnonzero(fits & clean & (f[:, l, tar] >= min_tar) & (f_neg[:, l] <= max_neg))
            for r in keep:
                found.append((int(r), l, o, float(f[r, l, tar]), float(f_neg[r, l])))
    found.sort(key=lambda x: (x[0], x[1], x[2]))
    cand = np.zeros(len(found), CANDIDATE_DTYPE)
    oligos = []
    for i, (r, l, o, ft, fn) in enumerate(found):
        q = int(q_of_row[r])
        cand[i] = (q, r - offs[q], lengths[l], o, ft, fn)
        s = text[r:r + lengths[l]]
        oligos.append((s.translate(_COMPLEMENT)[::-1] if o == "R" else s).decode())
    return cand, oligos
