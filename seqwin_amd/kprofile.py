"""Reading a k-mer profile (:class:`seqwin_amd.device.KmerProfile`): the share of a group that holds the k-mer
at a position, upper bounds for longer windows, the positions that tell targets from non-targets and the positions that repeat.  Pure
NumPy on the exported tables; nothing here touches a device.

The names are deliberately not those of the reference's ``MarkerMetrics``: these are exact counts of one k-mer per position over every
locus of every assembly -- no alignment, no mismatches, no BLAST, no Tm or dG, no conservation or divergence score of Seqwin's.  The
profile proposes; ``Batch.oligo_hits`` confirms.

Every function takes a ``KmerProfile`` or a :class:`Table` of host arrays.
"""
from __future__ import annotations

import numpy as np

NO_WINDOW = 0xFFFFFFFF
NO_WINDOW_COPIES = 0xFFFFFFFFFFFFFFFF


class Table:
    """A profile as host arrays, with the interface of ``KmerProfile`` that this module reads: ``offsets`` uint64[queries + 1],
    ``present`` uint32[total, groups], ``copies`` uint64[total, groups] or None, ``group_sizes`` uint32[groups], ``k``."""

    def __init__(self, offsets, present, copies, group_sizes, k: int):
        self._offs = np.asarray(offsets, np.uint64)
        self._present = np.asarray(present, np.uint32)
        self._copies = None if copies is None else np.asarray(copies, np.uint64)
        self._sizes = np.asarray(group_sizes, np.uint32)
        self.k = int(k)
        if self._present.ndim != 2 or self._present.shape != (int(self._offs[-1]), len(self._sizes)):
            raise ValueError(f"present is [total, groups] = {(int(self._offs[-1]), len(self._sizes))} (got shape {self._present.shape})")
        if self._copies is not None and self._copies.shape != self._present.shape:
            raise ValueError(f"copies has the shape of present (got {self._copies.shape})")

    def table(self):
        return self._offs, self._present, self._copies

    def group_sizes(self):
        return self._sizes


def _read(profile):
    """(offsets int64, present, copies or None, group_sizes, k)"""
    offs, present, copies = profile.table()
    return np.asarray(offs).astype(np.int64), np.asarray(present), copies, np.asarray(profile.group_sizes()), int(profile.k)


def _group(g, n_groups: int) -> int:
    if not 0 <= int(g) < n_groups:
        raise ValueError(f"group {g} is none of the table's {n_groups}")
    return int(g)


def fraction(profile) -> np.ndarray:
    """float64[total, groups]: ``present / group_sizes``, the share of the group's assemblies that hold the position's k-mer; nan at a
    ``NO_WINDOW`` row and for an empty group."""
    _, present, _, sizes, _ = _read(profile)
    out = np.full(present.shape, np.nan)
    ok = (present != NO_WINDOW) & (sizes != 0)[None, :]
    out[ok] = (present / np.where(sizes != 0, sizes, 1)[None, :].astype(np.float64))[ok]
    return out


def window_bounds(profile, length: int) -> np.ndarray:
    """uint32[total, groups]: per window start of ``length >= k`` bases inside one query, the minimum of ``present`` over the
    ``length - k + 1`` k-mers the window covers -- an upper bound of the assemblies of the group that hold the whole window exactly
    (an assembly that holds the window holds each of its k-mers), and that number itself at ``length == k``.  ``NO_WINDOW`` where a
    covered k-mer has no window or the window leaves its query."""
    offs, present, _, _, k = _read(profile)
    length = int(length)
    if length < k:
        raise ValueError(f"a window is at least the profile's k = {k} bases (got {length})")
    n = length - k + 1
    out = np.full(present.shape, NO_WINDOW, np.uint32)
    for q in range(len(offs) - 1):
        lo, hi = offs[q], offs[q + 1]
        m = hi - lo - length + 1          # window starts of this query
        if m <= 0:
            continue
        rows = present[lo:hi]
        low = rows[0:m].copy()
        high = rows[0:m].copy()
        for i in range(1, n):
            np.minimum(low, rows[i:i + m], out=low)
            np.maximum(high, rows[i:i + m], out=high)
        out[lo:lo + m] = np.where(high == NO_WINDOW, NO_WINDOW, low)   # (a sentinel in any group is one in every group)
    return out


def specific_positions(profile, tar: int = 0, neg: int = 1, min_tar: float = 0.95, max_neg: float = 0.05) -> np.ndarray:
    """Rows of the table (``offsets[q] + u``) whose k-mer at least ``min_tar`` of group ``tar``'s assemblies hold and at most
    ``max_neg`` of group ``neg``'s: where an exact k-mer tells the two apart.  A ``NO_WINDOW`` row is none, and neither is any row
    when group ``tar`` is empty; an empty group ``neg`` reads ``f_neg = 0`` (no non-target holds anything), as
    ``pileup.candidate_oligos`` reads a window without depth there."""
    _, present, _, sizes, _ = _read(profile)
    tar, neg = _group(tar, len(sizes)), _group(neg, len(sizes))
    f = fraction(profile)
    window = present[:, tar] != NO_WINDOW
    f_neg = np.where(window & np.isnan(f[:, neg]), 0.0, f[:, neg])
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(window & (f[:, tar] >= min_tar) & (f_neg <= max_neg))


def repeat_positions(profile, group: int, min_mean_copies: float = 2.0) -> np.ndarray:
    """Rows whose k-mer the assemblies of ``group`` that hold it hold at least ``min_mean_copies`` times on average --
    ``copies / present >= min_mean_copies``: rRNA operons, IS elements and other repeats.  A ``NO_WINDOW`` row and a k-mer that no
    assembly of the group holds are none.  ValueError for a profile made without copies."""
    _, present, copies, sizes, _ = _read(profile)
    if copies is None:
        raise ValueError("the profile was made without copies (screen(..., profile=groups, copies=True) counts them)")
    g = _group(group, len(sizes))
    p, c = present[:, g], np.asarray(copies)[:, g]
    ok = (p != NO_WINDOW) & (p != 0)
    mean = np.zeros(len(p))
    mean[ok] = c[ok].astype(np.float64) / p[ok]
    return np.flatnonzero(ok & (mean >= float(min_mean_copies)))
