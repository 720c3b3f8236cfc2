"""Drop-in for the per-subgraph step of Seqwin's markers._get_cks (src/seqwin/markers.py:474-528), on the device.

``get_cks`` takes the kept index and the subgraphs as they are resident after ``Index.filter_kmers(f, subgraphs)`` and returns the
candidate markers as plain objects carrying the attributes that ``get_markers`` and ``_fetch_cks_seq`` read.  Not done here
(DESIGN.md section 7): the graph ordering ``path`` (left ``None``), the sequence text (``rep['seq']`` is ``None``) and BLAST.

The attribute and field names are an interface, kept as data below and pinned by tests/test_gpu_markers.py.
"""
from __future__ import annotations

import numpy as np

from .device import MARKER_DUP, MARKER_SINGLE, Index, Markers, Subgraphs  # noqa: F401

# fields of ``rep`` (a row of the reference's ``loc`` table), in the reference's column order
REP_FIELDS = "assembly_idx record_idx start stop n_kmers kmers is_target n_repeats len seq".split()
# attributes a candidate carries
CK_ATTRS = "graph kmers loc path rep len n_rep blast metrics rep_ratio warnings is_bad".split()
WARNING_OF_FLAG = {MARKER_SINGLE: "single", MARKER_DUP: "dup"}   # both make a candidate bad


class NoMetrics:
    """The metrics of a marker before any BLAST check: every metric reads as None."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None

    def __repr__(self):
        return "NoMetrics()"


class Candidate:
    """A candidate marker: an attribute holder with the names of ``CK_ATTRS``."""

    def __init__(self, **values):
        for name in CK_ATTRS:
            setattr(self, name, values.get(name))

    def __repr__(self):
        return f"Candidate(len={self.len}, n_rep={self.n_rep}, warnings={sorted(self.warnings)})"


def all_cks(markers: Markers, n_tar: int) -> list:
    """One candidate per subgraph of ``markers``, in the final subgraph order."""
    import pandas as pd
    reps, offs, hashes = markers.reps()
    bounds = offs.astype(np.int64).tolist()
    hashes = list(hashes)   # np.uint64 elements, as the reference's tuples hold them
    out = []
    for i, r in enumerate(reps):
        flags = int(r["flags"])
        warnings = {w for bit, w in WARNING_OF_FLAG.items() if flags & bit}
        values = dict(assembly_idx=int(r["assembly_idx"]), record_idx=r["record_idx"], start=r["start"], stop=r["stop"],
                      n_kmers=int(r["n_kmers"]), kmers=tuple(hashes[bounds[i]:bounds[i + 1]]), is_target=bool(r["assembly_idx"] < n_tar),
                      n_repeats=int(r["n_repeats"]), len=np.uint32(r["stop"] - r["start"]), seq=None)
        rep = pd.Series([values[f] for f in REP_FIELDS], index=REP_FIELDS, dtype=object, name=0)
        out.append(Candidate(rep=rep, len=values["len"], n_rep=int(r["n_rep"]), metrics=NoMetrics(), warnings=warnings,
                             is_bad=bool(warnings)))
    return out


def get_cks(kept: Index, subgraphs: Subgraphs, record_offsets, n_tar: int, kmerlen: int, windowsize: int, min_len: int) -> list:
    """markers._get_cks up to the sequence fetch: the candidates with ``len >= min_len`` that are not bad, ``rep_ratio`` set."""
    m = kept.marker_locs(subgraphs, record_offsets, n_tar, kmerlen, windowsize)
    try:
        cks = [ck for ck in all_cks(m, n_tar) if ck.len >= min_len and not ck.is_bad]
    finally:
        m.close()
    for ck in cks:
        ck.rep_ratio = ck.n_rep / n_tar
    return cks
