"""Drop-in for the per-subgraph step of Seqwin's markers._get_cks (src/seqwin/markers.py:474-528), on the device.

``get_cks`` takes the kept index and the subgraphs as they are resident after ``Index.filter_kmers(f, subgraphs)`` and returns the
candidate markers as plain objects carrying the attributes that ``get_markers`` and ``_fetch_cks_seq`` read.  Given the resident
batch it also fills ``rep['seq']`` (``_fetch_cks_seq``, markers.py:428-471, without reading a file again), and ``save_markers``
writes the two files ``get_markers`` ends with (markers.py:777-802).  ``row_summary`` condenses ``Markers.row_distances``.  Not
done here: the graph ordering ``path`` (left ``None``) and BLAST.

The attribute and field names are an interface, kept as data below and pinned by tests/test_gpu_markers.py.
"""
from __future__ import annotations

import gzip
from pathlib import Path

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


def _load_records(path) -> list:
    """The records of a FASTA file (``.gz``: gzip) the way utils.load_fasta (utils.py:492-530) yields them: the lines behind each
    header joined, in upper case.  A file that does not start with '>' is a ValueError, as there."""
    path = Path(path)
    text = gzip.decompress(path.read_bytes()).decode() if path.suffix == ".gz" else path.read_text()
    if text[:1] != ">":
        raise ValueError(f"FASTA file must start with '>', in: {path}")
    out = []
    for record in text.split(">")[1:]:
        eol = record.find("\n")
        out.append("" if eol < 0 else record[eol:].replace("\n", "").upper())
    return out


def get_cks(kept: Index, subgraphs: Subgraphs, record_offsets, n_tar: int, kmerlen: int, windowsize: int, min_len: int,
            batch=None, paths=None) -> list:
    """markers._get_cks: the candidates with ``len >= min_len`` that are not bad, ``rep_ratio`` set.  With ``batch`` (the resident
    batch the index was built from) ``rep['seq']`` is filled as ``str`` from the packed bases; a representative that holds a base
    the batch does not keep (lower case aside: an N, an IUPAC letter) is read from ``paths[assembly_idx]`` the reference's way
    instead, and is a ValueError naming the candidate when ``paths`` is not given.  Without a batch ``rep['seq']`` stays None."""
    m = kept.marker_locs(subgraphs, record_offsets, n_tar, kmerlen, windowsize)
    try:
        keep = [(i, ck) for i, ck in enumerate(all_cks(m, n_tar)) if ck.len >= min_len and not ck.is_bad]
        cks = [ck for _, ck in keep]
        if batch is not None and cks:
            offs, blob, inexact = m.sequences(batch, "reps", select=[i for i, _ in keep])
            bounds = offs.astype(np.int64).tolist()
            loaded = {}   # assembly_idx -> its records: a file is read once however many flagged representatives lie in it
            for j, ck in enumerate(cks):
                rep = ck.rep
                if not inexact[j]:
                    rep["seq"] = blob[bounds[j]:bounds[j + 1]].decode("ascii")
                elif paths is not None:
                    a = rep["assembly_idx"]
                    if a not in loaded:
                        loaded[a] = _load_records(paths[a])
                    rep["seq"] = loaded[a][int(rep["record_idx"])][int(rep["start"]):int(rep["stop"])]
                else:
                    raise ValueError(f"candidate {rep['assembly_idx']}-{int(rep['record_idx'])}-{int(rep['start'])}:{int(rep['stop'])} "
                                     "holds a base that is not A, C, G or T: pass `paths` to read it from its file")
    finally:
        m.close()
    for ck in cks:
        ck.rep_ratio = ck.n_rep / n_tar
    return cks


# WORKINGDIR.markers_fasta / .markers_csv (src/seqwin/config.py:276-277) and the fields of MarkerMetrics (markers.py:80-87)
MARKERS_FASTA = "signatures.fasta"
MARKERS_CSV = "signatures.csv"
METRIC_NAMES = ("conservation f_tar_hits divergence f_neg_hits avg_repeats_tar avg_pident_tar avg_repeats_neg avg_pident_neg").split()


def _file_to_write(path: Path, overwrite: bool) -> None:
    if path.is_file():
        if not overwrite:
            raise FileExistsError(f"{path} exists (overwrite is off)")
        path.unlink()
    elif path.is_dir():
        raise IsADirectoryError(f"Expected a file, but a directory is found: {path}")


def save_markers(cks, record_ids, working_dir, overwrite: bool = False):
    """The file-saving block of markers.get_markers (markers.py:777-802): ``signatures.fasta`` with one record per candidate under
    the header ``{assembly_idx}-{record_id}-{start}:{stop}``, and ``signatures.csv`` with the header, the length, the metrics
    (empty before any BLAST check), ``rep_ratio`` and the number of k-mers.  ``record_ids``: ids by assembly, as
    ``Batch.records()`` returns them.  Returns the two paths."""
    import pandas as pd
    working_dir = Path(working_dir)
    fasta_path, csv_path = working_dir / MARKERS_FASTA, working_dir / MARKERS_CSV
    _file_to_write(fasta_path, overwrite)
    fasta, rows = [], []
    for ck in cks:
        rep = ck.rep
        header = f"{rep['assembly_idx']}-{record_ids[rep['assembly_idx']][rep['record_idx']]}-{rep['start']}:{rep['stop']}"
        fasta.append(f">{header}\n{rep['seq']}\n")
        rows.append((header, ck.len, *(getattr(ck.metrics, name) for name in METRIC_NAMES), ck.rep_ratio, rep["n_kmers"]))
    fasta_path.write_text("".join(fasta), encoding="utf-8", newline="\n")
    _file_to_write(csv_path, overwrite)
    pd.DataFrame(rows, columns=("fasta_header", "length", *METRIC_NAMES, "rep_ratio", "n_nodes")).to_csv(
        csv_path, index=False, encoding="utf-8", lineterminator="\n")
    return fasta_path, csv_path


ROW_SUMMARY_DTYPE = np.dtype([("identity_tar", "<f8"), ("f_tar_rows", "<f8"), ("distance_neg", "<f8"), ("f_neg_rows", "<f8")])


def row_summary(markers: Markers, dist, n_tar: int, n_neg: int) -> np.ndarray:
    """Per subgraph, from ``dist`` of ``markers.row_distances(batch)``: ``identity_tar`` = the sum over its target rows of
    ``max(0, 1 - dist / len(R))`` divided by ``n_tar``, ``distance_neg`` = the sum over its other rows of ``min(1, dist / len(R))``
    divided by ``n_neg``, and the rows of either kind over ``n_tar`` / ``n_neg`` (``f_tar_rows``, ``f_neg_rows``); R is the
    subgraph's representative.  These are NOT BLAST's ``conservation`` / ``divergence``: only located copies count, by edit distance."""
    reps = markers.reps()[0]
    per = markers.rows()
    out = np.zeros(len(per), ROW_SUMMARY_DTYPE)
    dist = np.asarray(dist, np.float64)
    if len(dist) != sum(len(r) for r, _, _ in per):
        raise ValueError(f"{len(dist)} distances for {sum(len(r) for r, _, _ in per)} rows")
    at = 0
    for i, (rows, _, _) in enumerate(per):
        d = dist[at:at + len(rows)]
        at += len(rows)
        length = np.float64(np.uint32(reps["stop"][i] - reps["start"][i]))
        tar = rows["assembly_idx"] < n_tar
        frac = d / length if length else np.ones(len(d))
        out["identity_tar"][i] = np.maximum(0.0, 1.0 - frac[tar]).sum() / n_tar if n_tar else 0.0
        out["f_tar_rows"][i] = tar.sum() / n_tar if n_tar else 0.0
        out["distance_neg"][i] = np.minimum(1.0, frac[~tar]).sum() / n_neg if n_neg else 0.0
        out["f_neg_rows"][i] = (~tar).sum() / n_neg if n_neg else 0.0
    return out


SCREEN_SUMMARY_DTYPE = np.dtype([("n_kmers", "<u4"), ("containment_tar", "<f8"), ("f_tar", "<f8"), ("containment_neg", "<f8"), ("f_neg", "<f8")])


def screen_summary(screen, n_tar: int, min_containment: float = 0.9) -> np.ndarray:
    """Per query of a :class:`Screen` (or of a pair ``(counts, n_kmers)`` of host arrays), with the targets the first ``n_tar``
    columns and the non-targets the rest: ``containment_tar`` / ``containment_neg`` = the mean over the group's assemblies of
    ``counts / n_kmers``, ``f_tar`` / ``f_neg`` = the fraction of the group's assemblies with ``counts / n_kmers >= min_containment``,
    all in float64.  A query without a k-mer, and an empty group, read ``nan``.  These are NOT BLAST's ``conservation`` /
    ``divergence`` and none of ``MarkerMetrics``: shared exact k-mers say nothing about an alignment."""
    counts, n_kmers = (screen.counts(), screen.n_kmers()) if hasattr(screen, "counts") else screen
    counts = np.asarray(counts, np.uint32)
    n_kmers = np.asarray(n_kmers, np.uint32)
    if counts.ndim != 2 or n_kmers.shape != (counts.shape[0],):
        raise ValueError(f"counts of shape {counts.shape} against {n_kmers.shape} k-mer counts")
    n_tar = int(n_tar)
    if not 0 <= n_tar <= counts.shape[1]:
        raise ValueError(f"n_tar = {n_tar} lies outside the {counts.shape[1]} assemblies")
    out = np.zeros(len(n_kmers), SCREEN_SUMMARY_DTYPE)
    out["n_kmers"] = n_kmers
    nk = n_kmers.astype(np.float64)
    nk[nk == 0] = np.nan
    c = counts.astype(np.float64) / nk[:, None]
    for name, f_name, block in (("containment_tar", "f_tar", c[:, :n_tar]), ("containment_neg", "f_neg", c[:, n_tar:])):
        if block.shape[1] == 0:
            out[name] = out[f_name] = np.nan
            continue
        out[name] = block.sum(axis=1) / block.shape[1]
        out[f_name] = np.where(np.isnan(nk), np.nan, (block >= np.float64(min_containment)).sum(axis=1) / block.shape[1])
    return out


HIT_SUMMARY_DTYPE = np.dtype([("similarity_tar", "<f8"), ("f_tar", "<f8"), ("distance_neg", "<f8"), ("f_neg", "<f8")])


def hit_summary(h, lengths, n_tar: int, min_identity: float = 0.9) -> np.ndarray:
    """Per query of a :class:`BestHits` (or of a uint32 ``dist`` matrix of host memory, 0xFFFFFFFF = no hit), with ``lengths`` the
    queries' lengths, the targets the first ``n_tar`` columns and the non-targets the rest: ``similarity_tar`` = the mean over the
    targets of ``max(0, 1 - dist / len)`` with 0 where there is no hit, ``distance_neg`` = the mean over the non-targets of
    ``min(1, dist / len)`` with 1 where there is no hit, ``f_tar`` / ``f_neg`` = the share of the group's assemblies with a hit and
    ``dist <= (1 - min_identity) * len``, all in float64.  A query of length 0, and an empty group, read ``nan``.  The names are
    deliberately not those of ``MarkerMetrics``: an infix edit distance at one seeded locus is not BLAST's best hit, and nothing
    of this is written into ``signatures.csv``."""
    dist = np.asarray(h.dist() if hasattr(h, "dist") else h, np.uint32)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if dist.ndim != 2 or lengths.shape != (dist.shape[0],) or (lengths < 0).any():
        raise ValueError(f"dist of shape {dist.shape} against {lengths.shape} query lengths")
    n_tar = int(n_tar)
    if not 0 <= n_tar <= dist.shape[1]:
        raise ValueError(f"n_tar = {n_tar} lies outside the {dist.shape[1]} assemblies")
    out = np.zeros(len(lengths), HIT_SUMMARY_DTYPE)
    ln = lengths.astype(np.float64)
    ln[ln == 0] = np.nan
    hit = dist != np.uint32(0xFFFFFFFF)
    frac = np.where(hit, dist.astype(np.float64), np.inf) / ln[:, None]          # dist / len; inf without a hit, nan for an empty query
    near = hit & (dist.astype(np.float64) <= (1.0 - np.float64(min_identity)) * ln[:, None])
    for name, f_name, cols, val in (("similarity_tar", "f_tar", slice(0, n_tar), np.maximum(0.0, 1.0 - frac)),
                                    ("distance_neg", "f_neg", slice(n_tar, None), np.minimum(1.0, frac))):
        block = val[:, cols]
        if block.shape[1] == 0:
            out[name] = out[f_name] = np.nan
            continue
        out[name] = block.sum(axis=1) / block.shape[1]
        out[f_name] = np.where(np.isnan(ln), np.nan, near[:, cols].sum(axis=1) / block.shape[1])
    return out


ALIGNMENT_SUMMARY_DTYPE = np.dtype([("identity_tar", "<f8"), ("f_tar", "<f8"), ("distance_neg", "<f8"), ("f_neg", "<f8")])


def alignment_summary(h, lengths, n_tar: int) -> np.ndarray:
    """Per query of a :class:`BestHits` made with ``align=True``, with ``lengths`` the queries' lengths, the targets the first
    ``n_tar`` columns and the non-targets the rest: ``identity_tar`` = the sum of ``nident`` over the targets' hits / len / n_tar,
    ``distance_neg`` = the sum of ``mismatch + gaps`` over the non-targets' hits / len / n_neg -- the formulas of ``_get_avg_ident``
    and ``_get_avg_dist`` (src/seqwin/markers.py:531-604) applied to the canonical alignment at one seeded locus --, ``f_tar`` /
    ``f_neg`` = the share of the group's assemblies with a hit, all in float64.  A query of length 0, and an empty group, read
    ``nan``.  The names are deliberately not those of ``MarkerMetrics``: this is not BLAST's best hit, and nothing of it is written
    into ``signatures.csv``."""
    nident = np.asarray(h.nident(), np.uint32)
    edits = np.asarray(h.mismatch(), np.uint32).astype(np.float64) + np.asarray(h.gaps(), np.uint32).astype(np.float64)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if nident.ndim != 2 or lengths.shape != (nident.shape[0],) or (lengths < 0).any():
        raise ValueError(f"hits of shape {nident.shape} against {lengths.shape} query lengths")
    n_tar = int(n_tar)
    if not 0 <= n_tar <= nident.shape[1]:
        raise ValueError(f"n_tar = {n_tar} lies outside the {nident.shape[1]} assemblies")
    out = np.zeros(len(lengths), ALIGNMENT_SUMMARY_DTYPE)
    ln = lengths.astype(np.float64)
    ln[ln == 0] = np.nan
    hit = nident != np.uint32(0xFFFFFFFF)
    for name, f_name, cols, val in (("identity_tar", "f_tar", slice(0, n_tar), np.where(hit, nident.astype(np.float64), 0.0)),
                                    ("distance_neg", "f_neg", slice(n_tar, None), np.where(hit, edits, 0.0))):
        block = val[:, cols]
        if block.shape[1] == 0:
            out[name] = out[f_name] = np.nan
            continue
        out[name] = block.sum(axis=1) / ln / block.shape[1]
        out[f_name] = np.where(np.isnan(ln), np.nan, hit[:, cols].sum(axis=1) / block.shape[1])
    return out


REPEAT_SUMMARY_DTYPE = np.dtype([("loci_tar", "<f8"), ("identity_all_tar", "<f8"), ("loci_neg", "<f8"), ("identity_all_neg", "<f8")])


def repeat_summary(h, lengths, n_tar: int) -> np.ndarray:
    """Per query of a :class:`BestHits` made with ``loci=True``, with ``lengths`` the queries' lengths, the targets the first
    ``n_tar`` columns and the non-targets the rest; a cell with ``n_loci > 0`` has a hit.  ``loci_tar`` = the mean of ``n_loci`` over
    the query's target cells with a hit, ``identity_all_tar`` = the mean of ``sum_nident / n_loci`` over those cells / len;
    ``loci_neg`` / ``identity_all_neg`` the same over the non-target cells -- the arithmetic ``_get_metrics``
    (src/seqwin/markers.py:566-604) applies to its ``n_hits`` and ``avg_nident`` columns, here on the seeded loci of DESIGN.md section
    3.2g.  ``0.0`` where no cell of the group has a hit, as ``_BASELINE_METRICS`` reads.  The names are deliberately not those of
    ``MarkerMetrics``: a locus is not a BLAST hit, this is not BLAST, and nothing of it is written into ``signatures.csv``."""
    n_loci = np.asarray(h.n_loci(), np.uint32)
    sum_nident = np.asarray(h.sum_nident(), np.uint32)
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if n_loci.ndim != 2 or lengths.shape != (n_loci.shape[0],) or (lengths < 0).any():
        raise ValueError(f"hits of shape {n_loci.shape} against {lengths.shape} query lengths")
    n_tar = int(n_tar)
    if not 0 <= n_tar <= n_loci.shape[1]:
        raise ValueError(f"n_tar = {n_tar} lies outside the {n_loci.shape[1]} assemblies")
    out = np.zeros(len(lengths), REPEAT_SUMMARY_DTYPE)
    hit = n_loci > 0
    avg = np.where(hit, sum_nident / np.maximum(n_loci, 1), 0.0)      # (a cell with a hit has a query of at least k bases)
    ln = np.maximum(lengths, 1).astype(np.float64)
    for loci_name, ident_name, cols in (("loci_tar", "identity_all_tar", slice(0, n_tar)), ("loci_neg", "identity_all_neg", slice(n_tar, None))):
        cells = hit[:, cols].sum(axis=1)
        some = cells > 0
        den = np.maximum(cells, 1)
        out[loci_name] = np.where(some, np.where(hit, n_loci, 0)[:, cols].sum(axis=1) / den, 0.0)
        out[ident_name] = np.where(some, avg[:, cols].sum(axis=1) / den / ln, 0.0)
    return out


LOCAL_SUMMARY_DTYPE = np.dtype([("coverage_tar", "<f8"), ("identity_local_tar", "<f8"), ("f_tar", "<f8"), ("distance_local_neg", "<f8"),
                                ("f_neg", "<f8")])


def _best_locus_cells(h, shape):
    """Per cell the figures (qstart, qend, nident, mismatch, gaps, hit) of its non-duplicate locus with the highest local score, ties
    going to the first in list order; computed on the host from ``cell_offsets``."""
    L = h.loci()
    offs = L["cell_offsets"].astype(np.int64)
    keep = np.flatnonzero(L["dup"] == 0)
    cell = np.searchsorted(offs, keep, side="right") - 1                       # the cell of every kept locus (ascending)
    order = np.lexsort((keep, -L["local_score"][keep].astype(np.int64), cell))  # by cell, score descending, list order
    first = order[np.concatenate(([True], cell[order][1:] != cell[order][:-1]))] if len(order) else order
    out = {f: np.zeros(shape, np.float64).reshape(-1) for f in ("qstart", "qend", "nident", "mismatch", "gaps")}
    hit = np.zeros(shape, bool).reshape(-1)
    hit[cell[first]] = True
    for f in out:
        out[f][cell[first]] = L["local_" + f][keep[first]]
    return {f: a.reshape(shape) for f, a in out.items()}, hit.reshape(shape)


def local_summary(h, lengths, n_tar: int, best_locus: bool = False) -> np.ndarray:
    """Per query of a :class:`BestHits` made with ``local=True``, with ``lengths`` the queries' lengths, the targets the first
    ``n_tar`` columns and the non-targets the rest: ``coverage_tar`` = the mean over ALL targets of ``(qend - qstart) / len`` with 0
    where there is no hit, ``identity_local_tar`` = the sum of the local ``nident`` over the targets' hits / len / n_tar,
    ``distance_local_neg`` = the sum of the local ``mismatch + gaps`` over the non-targets' hits / len / n_neg, ``f_tar`` / ``f_neg`` =
    the share of the group's assemblies with a hit, all in float64.  A query of length 0, and an empty group, read ``nan``.
    ``best_locus=True`` (hits made with ``loci=True`` too): a cell's figures are those of its non-duplicate locus with the highest
    local score, ties going to the first in list order, not those of the vote's winner.  A copy of which a non-target holds half
    reads here as half the coverage at distance 0, where ``alignment_summary`` reads half a query of edits.  The names are
    deliberately not those of ``MarkerMetrics``: the window is a seeded one, there is no X-drop and no e-value, this is not BLAST,
    and nothing of it is written into ``signatures.csv``."""
    lengths = np.asarray(lengths, np.int64).reshape(-1)
    if best_locus:
        nq, na = h.sizes()[:2]
        cells, hit = _best_locus_cells(h, (nq, na))
        span, nident, edits = cells["qend"] - cells["qstart"], cells["nident"], cells["mismatch"] + cells["gaps"]
    else:
        score = np.asarray(h.score(), np.uint32)
        hit = score != np.uint32(0xFFFFFFFF)
        f64 = lambda a: np.where(hit, np.asarray(a, np.uint32).astype(np.float64), 0.0)   # noqa: E731
        span, nident, edits = f64(h.qend()) - f64(h.qstart()), f64(h.local_nident()), f64(h.local_mismatch()) + f64(h.local_gaps())
    if hit.ndim != 2 or lengths.shape != (hit.shape[0],) or (lengths < 0).any():
        raise ValueError(f"hits of shape {hit.shape} against {lengths.shape} query lengths")
    n_tar = int(n_tar)
    if not 0 <= n_tar <= hit.shape[1]:
        raise ValueError(f"n_tar = {n_tar} lies outside the {hit.shape[1]} assemblies")
    out = np.zeros(len(lengths), LOCAL_SUMMARY_DTYPE)
    ln = lengths.astype(np.float64)
    ln[ln == 0] = np.nan
    tar, neg = slice(0, n_tar), slice(n_tar, None)
    n_neg = hit.shape[1] - n_tar
    if n_tar:
        out["coverage_tar"] = span[:, tar].sum(axis=1) / ln / n_tar
        out["identity_local_tar"] = nident[:, tar].sum(axis=1) / ln / n_tar
        out["f_tar"] = np.where(np.isnan(ln), np.nan, hit[:, tar].sum(axis=1) / n_tar)
    else:
        out["coverage_tar"] = out["identity_local_tar"] = out["f_tar"] = np.nan
    if n_neg:
        out["distance_local_neg"] = edits[:, neg].sum(axis=1) / ln / n_neg
        out["f_neg"] = np.where(np.isnan(ln), np.nan, hit[:, neg].sum(axis=1) / n_neg)
    else:
        out["distance_local_neg"] = out["f_neg"] = np.nan
    return out


def cigar(offsets, ops) -> list:
    """The edit scripts of :meth:`Batch.infix_alignments` (``ops=True``) as run-length strings such as ``12=1X3=2I``: ``=`` match,
    ``X`` mismatch, ``I`` a query base facing a gap, ``D`` a text base facing a gap; an empty script is the empty string."""
    offsets = np.asarray(offsets, np.uint64).astype(np.int64)
    ops = np.asarray(ops, np.uint8)
    if offsets.ndim != 1 or len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != len(ops) or (ops > 3).any():
        raise ValueError("offsets and ops are no edit scripts in CSR form")
    out = []
    for a, b in zip(offsets[:-1], offsets[1:]):
        s = ops[a:b]
        if not len(s):
            out.append("")
            continue
        heads = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))
        runs = np.diff(np.concatenate((heads, [len(s)])))
        out.append("".join(f"{int(n)}{'=XID'[int(s[i])]}" for i, n in zip(heads, runs)))
    return out
