"""Helpers of tests/test_gpu_wide_index.py: references for a batch whose batch-wide base index passes 2^32, neither of which is the
code under test at such an index.

* Pair lists (query, strand, record, start, stop).  :func:`excerpt_model` replaces every pair's record by the text of its window --
  fetched by the caller from a SHARD of the same synthetic job, where every base index is small -- and moves the pair to the
  excerpt's start; the host restatements (hits_host, align_host, local_host, pileup_host) run on that model, and :func:`shift_back`
  puts the record positions they return (`end`, `start`, `sstart`, `send`) back where the window lies in its record.  `qstart` and
  `qend` are positions in the query: an excerpt does not move them.
* Whole-batch walks.  The columns of a result on the wide batch that belong to a shard's assemblies must equal the shard's own
  result: :func:`assert_columns` for matrices (record indices moved by the shard's first record), :func:`assert_list` for site and
  locus lists restricted to those assemblies.
"""
from __future__ import annotations

import numpy as np

NO_HIT = 0xFFFFFFFF
RECORD_POSITIONS = ("end", "start", "sstart", "send")


def excerpt_model(pairs, texts):
    """(records, model pairs, starts): ``texts[i]`` is the text of pair i's window ``[start, stop)``; record i of the model is that
    excerpt and pair i of the model is ``(query, strand, i, 0, stop - start)``."""
    assert len(pairs) == len(texts)
    records, model, starts = [], [], []
    for i, ((q, s, _, a, z), t) in enumerate(zip(pairs, texts)):
        assert len(t) == z - a
        records.append(bytes(t))
        model.append((q, s, i, 0, z - a))
        starts.append(a)
    return records, model, np.asarray(starts, np.int64)


def shift_back(out: dict, starts) -> dict:
    """A copy of a restatement's arrays with every record position moved by its pair's excerpt start."""
    res = dict(out)
    for f in RECORD_POSITIONS:
        if f in res:
            res[f] = (np.asarray(res[f]).astype(np.int64) + starts).astype(np.uint32)
    return res


def moved_records(rec, by: int) -> np.ndarray:
    """Record indices of a shard as the whole batch numbers them; NO_HIT stays."""
    r = np.asarray(rec).astype(np.int64)
    return np.where(r == NO_HIT, NO_HIT, r + by).astype(np.uint32)


def assert_columns(wide: dict, shard: dict, fields, c0: int, r0: int, what) -> None:
    """Columns [c0, c0 + the shard's) of every matrix of ``wide`` equal the shard's matrix; the field ``record`` / ``best_record``
    holds record indices, which the shard counts from its own first record r0."""
    for f in fields:
        w, s = np.asarray(wide[f]), np.asarray(shard[f])
        assert w.dtype == s.dtype and w.shape[0] == s.shape[0], (what, f)
        want = moved_records(s, r0) if f in ("record", "best_record") else s
        got = w[:, c0:c0 + s.shape[1]]
        assert np.array_equal(got, want), (what, f, got.tolist(), want.tolist())


def assert_list(wide: dict, shard: dict, fields, n_rows: int, n_cols: int, c0: int, r0: int, what) -> None:
    """The entries of a list (parallel arrays with ``assembly`` and ``record`` among them, ``cell_offsets`` over n_rows x n_cols cells)
    that lie in the shard's assemblies, in the list's order, equal the shard's whole list; so do the cells' counts."""
    s_cols =(len(shard["cell_offsets"]) - 1) // n_rows if n_rows else 0
    asm = np.asarray(wide["assembly"]).astype(np.int64)
    keep = (asm >= c0) & (asm < c0 + s_cols)
    assert int(keep.sum()) == len(shard["assembly"]), (what, int(keep.sum()), len(shard["assembly"]))
    for f in fields:
        got = np.asarray(wide[f])[keep]
        if f == "assembly":
            got = (got.astype(np.int64) - c0).astype(got.dtype)
        elif f == "record":
            got = (got.astype(np.int64) - r0).astype(got.dtype)
        assert np.array_equal(got, shard[f]), (what, f, got.tolist(), np.asarray(shard[f]).tolist())
    w_cnt = np.diff(np.asarray(wide["cell_offsets"]).astype(np.int64)).reshape(n_rows, n_cols)
    s_cnt = np.diff(np.asarray(shard["cell_offsets"]).astype(np.int64)).reshape(n_rows, s_cols)
    assert np.array_equal(w_cnt[:, c0:c0 + s_cols], s_cnt), (what, "cell_offsets")


def rows_of(lst: dict, fields, keep=None) -> list:
    """The entries of a list as tuples over ``fields``, in the list's order; ``keep``: a mask over the entries."""
    cols = [np.asarray(lst[f]).astype(np.int64) for f in fields]
    if keep is not None:
        cols = [c[keep] for c in cols]
    return list(zip(*(c.tolist() for c in cols)))


# ---- the oligo search with indels on excerpts ----------------------------------------------------------------------------------------
# How far a site must lie from an excerpt's edge for the excerpt to decide it as the record does.  By tests/tools/oligo_edit_host.py
# an end e is a site by the values D(e') of the ends e - d <= e' <= e + d, and D(e') <= d is decided by the text an alignment of the
# oligo with at most d edits can face: the L + d bases before e'.  So the site [pos, e) on strand 0 is decided by the bases
# [e - d - (L + d), e + d) -- and e > pos, so an edge L + 2 d bases or more before pos and d or more behind e changes nothing: a cut
# text only takes alignments away (row 0 is free at every column, so the boundary column Dm[i][0] = i offers nothing the record does
# not), every value <= d keeps its alignment and with it its value, every other value stays above d, and the traceback compares only
# values <= d.  Strand 1 is the same on the reverse complement, with the sides exchanged.  L <= 32 and d <= 4 (OLE_MAX_EDITS): 32 +
# 2 * 4, and 4 to spare.  An edge of the excerpt that is the record's own edge needs no margin: the run ends there on the device too.
EDIT_MARGIN = 32 + 2 * 4 + 4


def interior(lo: int, hi: int, rec_len: int, margin: int = EDIT_MARGIN):
    """[a, z) of the excerpt [lo, hi) of a record: the sites inside it are decided by the excerpt alone."""
    assert 0 <= lo < hi <= rec_len
    return (lo if lo == 0 else lo + margin), (hi if hi == rec_len else hi - margin)


def bulge_at(text: bytes, lo: int = 4) -> int:
    """The index nearest the middle of ``text`` (at least ``lo`` + 1 letters from either end) whose base differs from both of its
    neighbours: deleting it, or inserting a fourth base in front of it, is one gap column in every optimal alignment's count."""
    n = len(text)
    for i in sorted(range(lo + 1, n - lo - 1), key=lambda i: (abs(i - n // 2), i)):
        if text[i] != text[i - 1] and text[i] != text[i + 1]:
            return i
    raise AssertionError("no base that differs from both neighbours")


def deleted(text: bytes) -> bytes:
    """``text`` without the base at :func:`bulge_at`"""
    i = bulge_at(text)
    return bytes(text[:i] + text[i + 1:])


def inserted(text: bytes) -> bytes:
    """``text`` with a base that neither neighbour is in front of :func:`bulge_at`"""
    i = bulge_at(text)
    new = next(c for c in b"ACGT" if c not in (text[i - 1], text[i]))
    return bytes(text[:i]) + bytes([new]) + bytes(text[i:])


def has_entry(lst: dict, **want) -> bool:
    """Whether a list holds an entry with these values."""
    m = None
    for f, v in want.items():
        eq = np.asarray(lst[f]).astype(np.int64) == int(v)
        m = eq if m is None else m & eq
    return bool(m is not None and m.any())
