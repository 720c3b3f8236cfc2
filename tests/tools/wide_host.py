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


def has_entry(lst: dict, **want) -> bool:
    """Whether a list holds an entry with these values."""
    m = None
    for f, v in want.items():
        eq = np.asarray(lst[f]).astype(np.int64) == int(v)
        m = eq if m is None else m & eq
    return bool(m is not None and m.any())
