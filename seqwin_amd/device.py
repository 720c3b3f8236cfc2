"""Device-resident pipeline: batches of 2-bit packed assemblies in HBM and indexes built from them.

Thin object wrappers over the ``sw_batch_*`` / ``sw_index_*`` / ``sw_sketch`` entry points of
include/seqwin_hip.h.  This is what ``sw_build`` is made of; bench.py and the multi-GPU driver use it
directly so that the timed region starts with inputs already resident in HBM.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._core import EDGE_DTYPE, KMER_DTYPE, NODE_DTYPE, _ptr, _split_ids
from ._lib import Timings, c_u64, c_vp, check, lib


def device_count() -> int:
    return int(lib.sw_device_count())


def set_device(device: int) -> None:
    check(lib.sw_set_device(ctypes.c_int(device)))


def pool_trim() -> None:
    """Hand the library's cached, unused device blocks back to the driver (for a process that shares HBM with torch)."""
    lib.sw_pool_trim()


class Batch:
    """A set of assemblies, 2-bit packed and resident on the current device."""

    def __init__(self, handle: c_vp):
        self._h = handle

    @classmethod
    def from_fasta(cls, assembly_paths, n_cpu: int = 1) -> "Batch":
        paths = [os.fsencode(str(p)) for p in assembly_paths]
        arr = (ctypes.c_char_p * max(len(paths), 1))(*paths)
        h = c_vp()
        check(lib.sw_batch_from_fasta(arr, ctypes.c_size_t(len(paths)), c_u64(n_cpu), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def synthetic(cls, n_genomes: int, records_per_genome: int, record_len: int, n_ancestors: int = 1,
                  snp_ppm: int = 10000, seed: int = 1, first_genome: int = 0) -> "Batch":
        """Genomes [first_genome, first_genome + n_genomes) of the synthetic job ``seed``: a shard holds exactly the
        bases and record ids the unsharded batch holds for these genomes."""
        h = c_vp()
        check(lib.sw_batch_synthetic_shard(c_u64(n_genomes), c_u64(records_per_genome), c_u64(record_len),
                                           c_u64(n_ancestors), c_u64(snp_ppm), c_u64(seed), c_u64(first_genome),
                                           ctypes.byref(h)))
        return cls(h)

    @classmethod
    def synthetic_ragged(cls, n_genomes: int, genome_bp: int, n_ancestors: int = 1, snp_ppm: int = 10000, seed: int = 1,
                         first_genome: int = 0) -> "Batch":
        """Ragged draft assemblies (sw_batch_synthetic_ragged): 20-300 contigs of 200 bp ... 1.5 Mbp per genome, scaffold gaps of
        10-1000 N in one contig of ten."""
        h = c_vp()
        check(lib.sw_batch_synthetic_ragged(c_u64(n_genomes), c_u64(genome_bp), c_u64(n_ancestors), c_u64(snp_ppm), c_u64(seed),
                                            c_u64(first_genome), ctypes.byref(h)))
        return cls(h)

    def info(self) -> dict:
        v = [c_u64() for _ in range(4)]
        check(lib.sw_batch_info(self._h, *[ctypes.byref(x) for x in v]))
        return dict(n_assemblies=v[0].value, n_records=v[1].value, total_bp=v[2].value, device_bytes=v[3].value)

    def record_offsets(self) -> np.ndarray:
        offs = np.empty(self.info()["n_assemblies"] + 1, np.uint32)
        nb = c_u64()
        check(lib.sw_batch_records(self._h, _ptr(offs), None, c_u64(0), ctypes.byref(nb)))
        return offs

    def records(self):
        """(record_offsets, ids_by_assembly)"""
        na = self.info()["n_assemblies"]
        offs = np.empty(na + 1, np.uint32)
        nb = c_u64()
        check(lib.sw_batch_records(self._h, _ptr(offs), None, c_u64(0), ctypes.byref(nb)))
        blob = ctypes.create_string_buffer(max(nb.value, 1))
        check(lib.sw_batch_records(self._h, _ptr(offs), blob, c_u64(nb.value), ctypes.byref(nb)))
        return offs, _split_ids(blob.raw[:nb.value], offs)

    def record(self, record_idx: int) -> bytes:
        n = c_u64()
        check(lib.sw_batch_record(self._h, c_u64(record_idx), None, c_u64(0), ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        check(lib.sw_batch_record(self._h, c_u64(record_idx), buf, c_u64(n.value), ctypes.byref(n)))
        return buf.raw[:n.value]

    def sketch(self, kmerlen: int, windowsize: int, stream: int = 0):
        """All minimizers in (record_idx, pos) order: (out_hash[u64], kmers[KMER_DTYPE])."""
        n = c_u64()
        check(lib.sw_sketch(self._h, c_u64(kmerlen), c_u64(windowsize), c_vp(stream), None, None, c_u64(0),
                            ctypes.byref(n)))
        oh = np.empty(n.value, np.uint64)
        km = np.empty(n.value, KMER_DTYPE)
        check(lib.sw_sketch(self._h, c_u64(kmerlen), c_u64(windowsize), c_vp(stream), _ptr(oh), _ptr(km),
                            c_u64(n.value), ctypes.byref(n)))
        return oh[:n.value], km[:n.value]

    def build_index(self, kmerlen: int, windowsize: int, is_targets=None, stream: int = 0) -> "Index":
        h = c_vp()
        if is_targets is None:
            tar, n = None, 0
        else:
            t = np.ascontiguousarray(np.asarray(is_targets, np.bool_)).view(np.uint8)
            tar, n = _ptr(t), len(t)
        check(lib.sw_index_build(self._h, c_u64(kmerlen), c_u64(windowsize), tar, c_u64(n), c_vp(stream),
                                 ctypes.byref(h)))
        return Index(h)

    def minhash(self, kmerlen: int, sketchsize: int = 1000, seed: int = 42, stream: int = 0) -> "MinHash":
        """One MinHash sketch per assembly as ``mash sketch -k kmerlen -s sketchsize`` makes it (csrc/minhash.hip), from the
        resident packed bases.  ValueError for a k-mer length outside 1..32, as Mash refuses it."""
        h = c_vp()
        check(lib.sw_batch_minhash(self._h, c_u64(int(kmerlen)), c_u64(int(sketchsize)), c_u64(int(seed)), c_vp(stream),
                                   ctypes.byref(h)))
        return MinHash(h)

    def screen(self, queries, kmerlen: int, profile=None, n_groups=None, copies: bool = False, stream: int = 0) -> "Screen":
        """For every query (a list of ``str`` or ``bytes``) and every assembly: how many of the query's distinct canonical
        ``kmerlen``-mers occur anywhere in the assembly, exactly (csrc/screen.hip).  ACGTU in either case, U
        reads as T, every other byte ends a window.  Not BLAST.  ValueError for a k-mer length outside 1..32.
        ``profile=groups`` (it changes nothing the call answers without it) also counts, for every position
        of every query and every group, the assemblies of the group that hold the k-mer starting there anywhere, on either strand --
        one label per assembly, 0 .. ``n_groups - 1`` or 255 to leave the assembly out, ``n_groups`` (1..8) as the pileup takes it:
        the result then answers ``profile()``, a :class:`KmerProfile`.  ``copies=True`` (it needs ``profile``, else ValueError) also
        counts the copies every group holds.  With ``kmerlen`` an oligo's length this is the exact-match inclusivity and exclusivity
        of every window at once; it proposes, :meth:`oligo_hits` confirms.  No mismatches, no Tm, no dG."""
        if copies and profile is None:
            raise ValueError("copies=True needs profile=groups: the copies are counted per group")
        qs = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
        offs = np.zeros(len(qs) + 1, np.uint64)
        np.cumsum([len(q) for q in qs], out=offs[1:])
        h = c_vp()
        if profile is None:
            check(lib.sw_batch_screen(self._h, _ptr(offs), b"".join(qs), c_u64(len(qs)), c_u64(int(kmerlen)), c_vp(stream), ctypes.byref(h)))
            return Screen(h)
        lab, ng = _pile_groups(profile, self.info()["n_assemblies"], n_groups, "assembly")
        check(lib.sw_batch_screen_profile(self._h, _ptr(offs), b"".join(qs), c_u64(len(qs)), c_u64(int(kmerlen)), _ptr(lab), c_u64(ng),
                                          ctypes.c_int(1 if copies else 0), c_vp(stream), ctypes.byref(h)))
        return Screen(h, offsets=offs, copies=bool(copies))

    def infix_distances(self, queries, pairs, stats: bool = False):
        """``(dist, end)`` of the infix edit distance of queries against intervals of the batch (csrc/hits.hip, DESIGN.md section
        3.2e).  ``pairs`` is INFIX_PAIR_DTYPE or an (n, 5) array of ``(query, strand, record, start, stop)``: the pattern is the
        query (strand 0) or its reverse complement (strand 1), the text bases ``[start, stop)`` of the global record.  ``dist`` is
        the smallest unit-cost edit distance of the whole pattern to any substring of the text, ``end`` the record position behind
        the first text prefix that attains it.  An empty query gives ``(0, start)``, an empty text ``(len(query), start)``.  Not
        BLAST.  ValueError for a pair that names no query, no strand or no interval of its record."""
        offs, blob, nq = _query_csr(queries)
        pr = _infix_pairs(pairs)
        dist = np.empty(len(pr), np.uint32)
        end = np.empty(len(pr), np.uint32)
        c = (c_u64 * 6)()
        ms = (ctypes.c_double * 1)()
        check(lib.sw_batch_infix_distances(self._h, _ptr(offs), blob, c_u64(nq), _ptr(pr), c_u64(len(pr)), _ptr(dist), _ptr(end), c, ms))
        if not stats:
            return dist, end
        d = dict(zip(("pairs", "cells", "striped_pairs", "longest", "launches", "block_cap"), (int(x) for x in c)))
        d.update(distance_ms=ms[0])
        return dist, end, d

    def infix_alignments(self, queries, pairs, ops: bool = False, stats: bool = False):
        """:meth:`infix_distances` plus the canonical optimal alignment behind each distance (csrc/align.hip, DESIGN.md section
        3.2f): ``(dist, end, start, nident, mismatch, gaps)``, all uint32 -- the located copy is ``[start, end)`` of the record,
        ``nident`` / ``mismatch`` count the ``=`` / ``X`` columns and ``gaps`` both kinds of gap column, so that ``mismatch + gaps ==
        dist``.  ``ops=True`` adds ``(offsets, ops)``: the edit scripts in CSR form, pair i's ops in pattern order from ``start`` to
        ``end``, one uint8 each (OP_MATCH 0, OP_MISMATCH 1, OP_INSERT 2 -- a query base faces a gap --, OP_DELETE 3 -- a text base
        faces a gap); :func:`seqwin_amd.markers.cigar` renders them.  Not BLAST.  ``stats=True`` adds the call's counters last."""
        offs, blob, nq = _query_csr(queries)
        pr = _infix_pairs(pairs)
        out = [np.empty(len(pr), np.uint32) for _ in range(6)]
        c = (c_u64 * 8)()
        ms = (ctypes.c_double * 3)()
        h = c_vp()
        check(lib.sw_batch_infix_alignments(self._h, _ptr(offs), blob, c_u64(nq), _ptr(pr), c_u64(len(pr)), *[_ptr(a) for a in out],
                                            ctypes.byref(h) if ops else None, c, ms))
        res = tuple(out)
        if ops:
            try:
                n, nb = c_u64(), c_u64()
                check(lib.sw_ops_sizes(h, ctypes.byref(n), ctypes.byref(nb)))
                o_off = np.empty(n.value + 1, np.uint64)
                o_ops = np.empty(nb.value, np.uint8)
                check(lib.sw_ops_export(h, _ptr(o_off), _ptr(o_ops) if nb.value else None))
            finally:
                lib.sw_ops_free(h)
            res += (o_off, o_ops)
        if stats:
            d = dict(zip(_ALIGN_COUNTERS, (int(x) for x in c)))
            d.update(distance_ms=ms[0], store_ms=ms[1], walk_ms=ms[2])
            res += (d,)
        return res

    def infix_pileup(self, queries, pairs, groups, n_groups=None, max_dist_permille: int = 1000):
        """``(Pileup, (dist, end, start, nident, mismatch, gaps))``: :meth:`infix_alignments` whose walk also counts, per query
        position and group, what the pairs' canonical alignments put there (csrc/align.hip).  ``groups`` is
        one label per pair: 0 .. ``n_groups - 1`` (``n_groups`` in 1..8; None: the largest label + 1), or 255 to leave the pair out.
        A pair is piled iff ``dist * 1000 <= max_dist_permille * len(query)``; the default piles every labelled pair.  The counts
        are exact and do not depend on the order of the pairs.  Not BLAST, and not a multiple alignment: every pair is aligned to
        its query alone.  ValueError for a label in ``n_groups..254``, ``n_groups`` outside 1..8 or a bound outside 0..1000."""
        offs, blob, nq = _query_csr(queries)
        pr = _infix_pairs(pairs)
        lab, ng = _pile_groups(groups, len(pr), n_groups, "pair")
        out = [np.empty(len(pr), np.uint32) for _ in range(6)]
        h = c_vp()
        check(lib.sw_batch_infix_pileup(self._h, _ptr(offs), blob, c_u64(nq), _ptr(pr), c_u64(len(pr)), _ptr(lab), c_u64(ng), c_u64(int(max_dist_permille)),
                                        *[_ptr(a) for a in out], ctypes.byref(h), None, None))
        return Pileup(h, offs), tuple(out)

    def infix_windows(self, queries, pairs, groups, lengths, n_groups=None, max_dist_permille: int = 1000, max_mismatch: int = 2, three_prime: int = 3,
                      stats: bool = False):
        """``(Windows, Pileup, (dist, end, start, nident, mismatch, gaps))``: :meth:`infix_pileup` -- the same pileup and arrays, bit
        for bit -- whose walk also classes, per window start of every query, window length and group, how the piled pairs' copies
        match the window JOINTLY (csrc/align.hip).  ``lengths``: 1..8 distinct window lengths, each in 8..32;
        ``max_mismatch`` in 0..8 and below the shortest length; ``three_prime`` in 0..8: the bases at an oligo's 3' end that must not
        face a mismatch.  Anything else is a ValueError before a device is touched.  Exact counts that do not depend on the order
        of the pairs.  Not BLAST and no thermodynamic model: no Tm, no dG.  ``stats=True`` adds the counters and times of the
        alignment behind the tables last, as :meth:`infix_alignments` names them; ``walk_ms`` is the one walk that fills both tables."""
        offs, blob, nq = _query_csr(queries)
        pr = _infix_pairs(pairs)
        lab, ng = _pile_groups(groups, len(pr), n_groups, "pair")
        lens, mm, c3 = _window_args(lengths, max_mismatch, three_prime)
        out = [np.empty(len(pr), np.uint32) for _ in range(6)]
        c = (c_u64 * 8)()
        ms = (ctypes.c_double * 3)()
        h, wh = c_vp(), c_vp()
        check(lib.sw_batch_infix_windows(self._h, _ptr(offs), blob, c_u64(nq), _ptr(pr), c_u64(len(pr)), _ptr(lab), c_u64(ng), c_u64(int(max_dist_permille)),
                                         _ptr(lens), c_u64(len(lens)), c_u64(mm), c_u64(c3), *[_ptr(a) for a in out], ctypes.byref(h), ctypes.byref(wh), c, ms))
        res = (Windows(wh, offs), Pileup(h, offs), tuple(out))
        if stats:
            d = dict(zip(_ALIGN_COUNTERS, (int(x) for x in c)))
            d.update(distance_ms=ms[0], store_ms=ms[1], walk_ms=ms[2])
            res += (d,)
        return res

    def local_alignments(self, queries, pairs, scoring=(2, -3, 5, 2), stats: bool = False) -> dict:
        """The optimal LOCAL alignment of every pair of :meth:`infix_distances` under the scoring system ``(reward, penalty, gapopen,
        gapextend)`` -- a gap of L columns costs ``gapopen + L * gapextend``; the default is blastn's (csrc/local.hip, DESIGN.md section
        3.2i).  A dict of uint32 arrays: ``score``, ``qstart`` / ``qend`` (half-open, in the pattern's orientation), ``sstart`` /
        ``send`` (half-open record positions), ``nident``, ``mismatch``, ``gapopen`` and ``gaps``; of equal maxima the one that ends in
        the smallest column, then the smallest row.  ``score == 0`` (an empty side, no match): every count 0 and ``sstart == send ==
        start``.  Not BLAST: the window is the caller's, the dynamic programme is exhaustive inside it (no X-drop), no e-values, no
        bit scores.  ValueError for a scoring value outside 1..255, -255..-1, 0..255, 1..255, for a side of 2^16 bases or more, and
        for what :meth:`infix_distances` refuses.  ``stats=True`` adds the call's counters under ``"stats"``."""
        offs, blob, nq = _query_csr(queries)
        pr = _infix_pairs(pairs)
        out = [np.empty(len(pr), np.uint32) for _ in LOCAL_FIELDS]
        c = (c_u64 * 6)()
        ms = (ctypes.c_double * 1)()
        check(lib.sw_batch_local_alignments(self._h, _ptr(offs), blob, c_u64(nq), _ptr(pr), c_u64(len(pr)), _scoring(scoring), *[_ptr(a) for a in out], c, ms))
        res = dict(zip(LOCAL_FIELDS, out))
        if stats:
            res["stats"] = dict(zip(_LOCAL_COUNTERS, (int(x) for x in c)), local_ms=ms[0])
        return res

    def best_hits(self, queries, kmerlen: int, align: bool = False, loci: bool = False, min_seeds: int = 1, seed_copies=None, local: bool = False,
                  scoring=(2, -3, 5, 2), pileup=None, n_groups=None, max_dist_permille: int = 1000, window_lengths=None, window_mismatch: int = 2,
                  window_three_prime: int = 3) -> "BestHits":
        """For every query (a list of ``str`` or ``bytes``) and every assembly: the best seeded locus and the exact infix edit
        distance of the query to the best substring there (csrc/hits.hip).  A seed is a canonical
        ``kmerlen``-mer that exactly one window of ALL the query text has and that is not its own reverse complement: a query whose
        k-mers are shared with another query, or repeat inside it, loses them as seeds -- deliberately, one hit means one diagonal.
        Not BLAST: no scores, no e-values, no local alignment, one locus per pair.  ValueError for a k-mer length outside 1..32.
        ``align=True`` also traces every winner's alignment (:meth:`infix_alignments` on its window): the result then answers
        ``start()``, ``nident()``, ``mismatch()``, ``gaps()`` and ``intervals()``.
        ``loci=True`` (it implies ``align=True``) also lists EVERY seeded locus of every pair with ``min_seeds`` or more seeds (DESIGN.md
        section 3.2g: a local maximum of the vote over two bands to either side), each measured and traced like a winner: the result
        then answers ``n_loci()``, ``sum_nident()``, ``loci()``, ``loci_intervals()`` and ``loci_stats()``.  The matrix fields do not
        depend on ``min_seeds``.  ValueError for ``min_seeds < 1``.  Still not BLAST.
        ``seed_copies=c`` (1..256, else ValueError) shares seeds between windows of the query text: a
        canonical k-mer that 1..c windows of ALL the query text have, and that is not its own reverse complement, is a seed owned by
        every one of those windows, so two alleles in one call, a sequence given twice or a repeat inside a query keep their k-mers;
        a k-mer with more than c windows is dropped whole (the repeat mask, not truncated to c).  ``n_seeds()[q]`` counts the windows
        of q that own a seed, a window of the batch with a seed is one hit per owner, and vote, winner, distance, ``align`` and
        ``loci`` follow from the hits as above.  ``seed_copies=1`` gives the default's results bit for bit; ``None`` (the default) runs
        the unique-seed route itself.  ``seed_stats()`` says what the cap kept and dropped; the summaries of
        :mod:`seqwin_amd.markers` (``hit_summary``, ``alignment_summary``, ``repeat_summary``) take such a result unchanged.
        ``local=True`` (it combines with everything above and changes none of it) adds the optimal local
        alignment of every winner on its window under ``scoring`` (:meth:`local_alignments`): the result then answers ``score()``,
        ``qstart()``, ``qend()``, ``sstart()``, ``send()``, ``local_nident()``, ``local_mismatch()``, ``local_gapopen()``,
        ``local_gaps()`` and ``local_stats()``, and with ``loci=True`` its ``loci()`` has nine ``local_*`` columns.  A copy of which
        an assembly holds only a part reads as a large ``dist`` and as a clean local hit over that part.  Still not BLAST: our seeds and
        windows, no X-drop, no e-values.  ValueError for a query above 65279 bases.
        ``pileup=groups`` (it implies ``align=True``, combines with everything above and changes none of it)
        piles every winner's canonical alignment into the group of its assembly -- one label per assembly, 0 .. ``n_groups - 1`` or 255
        to leave the assembly out, ``n_groups`` and ``max_dist_permille`` as :meth:`infix_pileup` takes them: the result then answers
        ``pileup()``, a :class:`Pileup` of base counts per query position and group.  The loci of ``loci=True`` are not piled.
        ``window_lengths=(18, 20, 22, 25)`` (it needs ``pileup=groups``, else ValueError, and changes nothing the
        call answers without it) also classes every window of those lengths of every query by how the piled winners match it jointly
        -- 0, 1, 2, 3 or more mismatches, or a gap, and whether it serves as a forward or a reverse oligo with at most
        ``window_mismatch`` mismatches and none in the ``window_three_prime`` bases at the 3' end: the result then answers ``windows()``,
        a :class:`Windows`.  The arguments are :meth:`infix_windows`'.  Not BLAST and no thermodynamic model."""
        if window_lengths is not None and pileup is None:
            raise ValueError("window_lengths needs pileup=groups: the windows count the pairs the pileup piles")
        offs, blob, nq = _query_csr(queries)
        h = c_vp()
        if loci and int(min_seeds) < 1:
            raise ValueError(f"min_seeds must be at least 1 (got {min_seeds})")
        if pileup is not None:
            if seed_copies is not None and not 1 <= int(seed_copies) <= 256:
                raise ValueError(f"seed_copies must lie in 1..256 (got {seed_copies})")
            lab, ng = _pile_groups(pileup, self.info()["n_assemblies"], n_groups, "assembly")
            ph = c_vp()
            if window_lengths is not None:
                lens, mm, c3 = _window_args(window_lengths, window_mismatch, window_three_prime)
                wh = c_vp()
                check(lib.sw_batch_best_hits_windows(self._h, _ptr(offs), blob, c_u64(nq), c_u64(int(kmerlen)), c_u64(int(seed_copies or 0)),
                                                     c_u64(2 if loci else 1), c_u64(int(min_seeds) if loci else 0), _scoring(scoring) if local else None,
                                                     _ptr(lab), c_u64(ng), c_u64(int(max_dist_permille)), _ptr(lens), c_u64(len(lens)), c_u64(mm), c_u64(c3),
                                                     ctypes.byref(h), ctypes.byref(ph), ctypes.byref(wh)))
                return BestHits(h, aligned=True, loci=bool(loci), local=bool(local), pileup=Pileup(ph, offs), windows=Windows(wh, offs))
            check(lib.sw_batch_best_hits_pileup(self._h, _ptr(offs), blob, c_u64(nq), c_u64(int(kmerlen)), c_u64(int(seed_copies or 0)), c_u64(2 if loci else 1),
                                                c_u64(int(min_seeds) if loci else 0), _scoring(scoring) if local else None, _ptr(lab), c_u64(ng),
                                                c_u64(int(max_dist_permille)), ctypes.byref(h), ctypes.byref(ph)))
            return BestHits(h, aligned=True, loci=bool(loci), local=bool(local), pileup=Pileup(ph, offs))
        if local:
            if seed_copies is not None and not 1 <= int(seed_copies) <= 256:
                raise ValueError(f"seed_copies must lie in 1..256 (got {seed_copies})")
            mode = 2 if loci else 1 if align else 0
            check(lib.sw_batch_best_hits_local(self._h, _ptr(offs), blob, c_u64(nq), c_u64(int(kmerlen)), c_u64(int(seed_copies or 0)), c_u64(mode),
                                               c_u64(int(min_seeds) if loci else 0), _scoring(scoring), ctypes.byref(h)))
            return BestHits(h, aligned=mode >= 1, loci=mode == 2, local=True)
        if seed_copies is not None:
            if not 1 <= int(seed_copies) <= 256:
                raise ValueError(f"seed_copies must lie in 1..256 (got {seed_copies})")
            mode = 2 if loci else 1 if align else 0
            check(lib.sw_batch_best_hits_shared(self._h, _ptr(offs), blob, c_u64(nq), c_u64(int(kmerlen)), c_u64(int(seed_copies)), c_u64(mode),
                                                c_u64(int(min_seeds) if loci else 0), ctypes.byref(h)))
            return BestHits(h, aligned=mode >= 1, loci=mode == 2)
        if loci:
            check(lib.sw_batch_best_hits_loci(self._h, _ptr(offs), blob, c_u64(nq), c_u64(int(kmerlen)), c_u64(int(min_seeds)), ctypes.byref(h)))
            return BestHits(h, aligned=True, loci=True)
        fn = lib.sw_batch_best_hits_aligned if align else lib.sw_batch_best_hits
        check(fn(self._h, _ptr(offs), blob, c_u64(nq), c_u64(int(kmerlen)), ctypes.byref(h)))
        return BestHits(h, aligned=bool(align))

    def oligo_hits(self, oligos, max_mismatch: int = 0, three_prime: int = 0, sites: bool = False, stream: int = 0, max_edits=None, thermo=None,
                   max_dg=None) -> "OligoHits":
        """Every place in every assembly where an oligo (a list of ``str`` or ``bytes``: primers, probes) binds with at most
        ``max_mismatch`` mismatches, on either strand -- exhaustively, every window of the batch against every oligo, no seed
        (csrc/oligo.hip).  An oligo is 8..32 letters in either case: ``ACGT``, ``U`` (= T) or an IUPAC code
        ``RYSWKMBDHVN``; every position is a set of bases.  Strand 0 is the oligo, strand 1 its reverse complement.  A site is a window
        inside one valid run of a record, ``mm`` the number of its bases outside the set they face; a hit has ``mm <= max_mismatch``
        (0..8, below the shortest oligo) and no mismatch among the ``three_prime`` (0..8) bases at the oligo's 3' end.  An oligo that
        equals its reverse complement hits twice at one place.  ``sites=True`` also keeps the list of all hits.  Not BLAST: no
        e-values.  ValueError for anything else, before a device is touched.

        ``thermo`` (a :class:`seqwin_amd.oligos.ThermoModel`, e.g. ``oligos.santalucia98()``) also sums the
        model's integer tables over every hit: ``dh``, ``ds``, ``dg`` of the duplex the oligo forms there.  Per (oligo, assembly)
        ``n_stable`` counts the hits with ``dg <= max_dg`` (cal/mol; ``None``: every hit) and the ``stable_*`` fields describe the
        hit that is least in (dg, record, pos, strand) among ALL hits; with ``sites=True`` every entry of the list gets ``dh``,
        ``ds``, ``dg``.  The hits themselves are those of the call without it.  Not together with ``max_edits`` (ValueError): a
        bulge needs loop parameters.  No Tm on the device: :func:`seqwin_amd.oligos.melting_temperature`.

        ``max_edits`` (0..4, ``max_edits + three_prime`` below the shortest oligo, ``max_mismatch`` left at 0) searches by unit-cost
        edit distance instead, so that a site with a bulge of a base or two is found: an end ``e`` of a
        valid run is a site iff the oligo without its ``three_prime`` last letters aligns to some text that ends ``three_prime``
        bases before ``e`` within ``max_edits`` edits, those last bases match exactly, and no end within ``max_edits`` before it is
        as good nor one within ``max_edits`` after it better.  A site then has ``pos``, ``end``, ``dist``, ``mismatch`` and
        ``gaps`` from the canonical alignment.  ``max_edits=0`` gives the sites of ``max_mismatch=0``."""
        from .oligos import check_oligos
        qs = check_oligos(oligos, max_mismatch, three_prime, max_edits)
        offs = np.zeros(len(qs) + 1, np.uint64)
        np.cumsum([len(q) for q in qs], out=offs[1:])
        h = c_vp()
        if thermo is not None or max_dg is not None:
            from .oligos import ThermoModel
            if max_edits is not None:
                raise ValueError("thermo and max_edits exclude each other: a site with a bulge needs loop parameters")
            if not isinstance(thermo, ThermoModel):
                raise ValueError("thermo must be a seqwin_amd.oligos.ThermoModel (max_dg needs one)")
            if max_dg is not None:
                try:
                    whole = int(max_dg) == max_dg and -2 ** 31 <= int(max_dg) < 2 ** 31
                except (TypeError, ValueError, OverflowError):
                    whole = False
                if not whole:
                    raise ValueError(f"max_dg must be an integer of cal/mol that fits int32 (got {max_dg!r})")
            check(lib.sw_batch_oligo_hits_thermo(self._h, _ptr(offs), b"".join(qs), c_u64(len(qs)), c_u64(int(max_mismatch)), c_u64(int(three_prime)),
                                                 ctypes.c_int(1 if sites else 0), c_vp(stream), _ptr(thermo.stack), _ptr(thermo.end), _ptr(thermo.init),
                                                 ctypes.c_int64(0 if max_dg is None else int(max_dg)), ctypes.c_int(1 if max_dg is None else 0),
                                                 ctypes.byref(h)))
            return OligoHits(h, [len(q) for q in qs], bool(sites), thermo=True)
        if max_edits is None:
            check(lib.sw_batch_oligo_hits(self._h, _ptr(offs), b"".join(qs), c_u64(len(qs)), c_u64(int(max_mismatch)), c_u64(int(three_prime)),
                                          ctypes.c_int(1 if sites else 0), c_vp(stream), ctypes.byref(h)))
        else:
            check(lib.sw_batch_oligo_hits_edit(self._h, _ptr(offs), b"".join(qs), c_u64(len(qs)), c_u64(int(max_edits)), c_u64(int(three_prime)),
                                               ctypes.c_int(1 if sites else 0), c_vp(stream), ctypes.byref(h)))
        return OligoHits(h, [len(q) for q in qs], bool(sites))

    def fetch(self, intervals, stats: bool = False):
        """The text of ``intervals`` (INTERVAL_DTYPE or an (n, 3) array of record, start, stop; ``record`` is the batch's global
        record index), decoded from the resident packed bases (csrc/seqs.hip): ``(offsets, blob, inexact)`` -- interval i is
        ``blob[offsets[i]:offsets[i + 1]]`` in A, C, G, T and N for every invalid base; ``inexact[i]`` says that it is not
        contained in one valid run.  ValueError for an interval that does not lie inside its record."""
        iv = _intervals(intervals)
        h = c_vp()
        check(lib.sw_batch_fetch(self._h, _ptr(iv), c_u64(len(iv)), ctypes.byref(h)))
        return _export_seqs(h, stats)

    def edit_distances(self, r, s, stats: bool = False):
        """``(dist, strand)`` of the pairs of intervals ``(r[i], s[i])``: the smaller of the Levenshtein distances of R to S and to
        the reverse complement of S, and which of the two it was (0 on a tie), by DESIGN.md section 3.2c (csrc/seqs.hip).  Not BLAST.
        ``stats=True`` adds the call's counters and times as a third element."""
        r, s = _intervals(r), _intervals(s)
        if len(r) != len(s):
            raise ValueError(f"{len(r)} intervals against {len(s)}")
        dist = np.empty(len(r), np.uint32)
        strand = np.empty(len(r), np.uint8)
        c = (c_u64 * 6)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_batch_edit_distances(self._h, _ptr(r), _ptr(s), c_u64(len(r)), _ptr(dist), _ptr(strand), c, ms))
        return (dist, strand, _distance_stats(c, ms)) if stats else (dist, strand)

    def close(self) -> None:
        if self._h:
            lib.sw_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


INTERVAL_DTYPE = np.dtype([("record", "<u4"), ("start", "<u4"), ("stop", "<u4")])
SEQ_INEXACT = 1
INFIX_PAIR_DTYPE = np.dtype([("query", "<u4"), ("strand", "<u4"), ("record", "<u4"), ("start", "<u4"), ("stop", "<u4")])
NO_HIT = 0xFFFFFFFF   # record, end and dist of a (query, assembly) without a hit
OP_MATCH, OP_MISMATCH, OP_INSERT, OP_DELETE = 0, 1, 2, 3   # the bytes of an edit script: = X I D
_ALIGN_COUNTERS = ("pairs", "rounds", "striped_pairs", "own_scratch_pairs", "scratch_peak_bytes", "ops", "largest_pair_bytes", "store_launches")


def _query_csr(queries):
    """(offsets uint64[n + 1], blob, n) of a list of ``str`` or ``bytes``."""
    qs = [q.encode("utf-8") if isinstance(q, str) else bytes(q) for q in queries]
    offs = np.zeros(len(qs) + 1, np.uint64)
    np.cumsum([len(q) for q in qs], out=offs[1:])
    return offs, b"".join(qs), len(qs)


PILE_CLASSES = ("A", "C", "G", "T", "N", "DEL", "INS", "INS_BASES")   # the last axis of a pileup's table
PILE_LEAVE_OUT = 0xFF   # the group label that keeps a pair or an assembly out of the pileup


def _pile_groups(groups, n: int, n_groups, what: str):
    """(labels uint8[n], n_groups) of a pileup call; the library checks the labels against ``n_groups``."""
    a = np.asarray(groups)
    if a.ndim != 1 or len(a) != n:
        raise ValueError(f"the pileup takes one group label per {what}: {n} (got an array of shape {a.shape})")
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or not len(a)):
        raise ValueError(f"group labels are integers 0..7 or {PILE_LEAVE_OUT} (got {a.dtype})")
    a = a.astype(np.int64)
    if len(a) and (a.min() < 0 or a.max() > 0xFF):
        raise ValueError(f"group labels are integers 0..7 or {PILE_LEAVE_OUT}")
    if n_groups is None:
        kept = a[a != PILE_LEAVE_OUT]
        n_groups = int(kept.max()) + 1 if len(kept) else 1
    return np.ascontiguousarray(a.astype(np.uint8)), int(n_groups)


WINDOW_CLASSES = ("MM0", "MM1", "MM2", "MM3", "MM4P", "GAPPED", "FWD_OK", "REV_OK")   # the last axis of a window table


def _window_args(lengths, max_mismatch, three_prime):
    """(lengths uint32[n], max_mismatch, three_prime) of a windows call, checked as the library checks them."""
    try:
        lens = [int(x) for x in lengths]
    except TypeError:
        raise ValueError(f"window lengths are 1..8 distinct integers in 8..32 (got {lengths!r})") from None
    if not 1 <= len(lens) <= 8:
        raise ValueError(f"the windows take 1..8 lengths (got {len(lens)})")
    if any(not 8 <= x <= 32 for x in lens):
        raise ValueError(f"a window length lies outside 8..32 (got {lens})")
    if len(set(lens)) != len(lens):
        raise ValueError(f"a window length is given twice (got {lens})")
    mm, c3 = int(max_mismatch), int(three_prime)
    if not 0 <= mm <= 8 or mm >= min(lens):
        raise ValueError(f"max_mismatch must lie in 0..8 and below the shortest window length {min(lens)} (got {max_mismatch})")
    if not 0 <= c3 <= 8:
        raise ValueError(f"three_prime must lie in 0..8 (got {three_prime})")
    return np.array(lens, np.uint32), mm, c3


LOCAL_FIELDS = ("score", "qstart", "qend", "sstart", "send", "nident", "mismatch", "gapopen", "gaps")
_LOCAL_COUNTERS = ("pairs", "cells", "striped_pairs", "hbm_carry_pairs", "launches", "pass_rows")


def _scoring(scoring):
    """``(reward, penalty, gapopen, gapextend)`` as the int32[4] a ``sw_scoring`` is; the library checks the ranges."""
    v = [int(x) for x in scoring]
    if len(v) != 4 or any(abs(x) >= 1 << 31 for x in v):
        raise ValueError(f"scoring must be (reward, penalty, gapopen, gapextend) (got {scoring!r})")
    return (ctypes.c_int32 * 4)(*v)


def _infix_pairs(pairs) -> np.ndarray:
    a = np.asarray(pairs)
    if a.dtype != INFIX_PAIR_DTYPE:
        a = np.asarray(a, np.int64).reshape(-1, 5)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError("query, strand, record, start and stop of a pair are 32-bit values")
        out = np.empty(len(a), INFIX_PAIR_DTYPE)
        for i, f in enumerate(INFIX_PAIR_DTYPE.names):
            out[f] = a[:, i]
        a = out
    return np.ascontiguousarray(a)


def _intervals(iv) -> np.ndarray:
    a = np.asarray(iv)
    if a.dtype != INTERVAL_DTYPE:
        a = np.asarray(a, np.int64).reshape(-1, 3)
        if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
            raise ValueError("record, start and stop of an interval are 32-bit values")
        out = np.empty(len(a), INTERVAL_DTYPE)
        out["record"], out["start"], out["stop"] = a[:, 0], a[:, 1], a[:, 2]
        a = out
    return np.ascontiguousarray(a)


def _export_seqs(h: c_vp, stats: bool = False):
    """(offsets, blob, inexact) of a sw_seqs handle, which is freed; with ``stats`` the call's counters and time as a fourth."""
    try:
        n, nb = c_u64(), c_u64()
        check(lib.sw_seqs_sizes(h, ctypes.byref(n), ctypes.byref(nb)))
        offs = np.empty(n.value + 1, np.uint64)
        blob = ctypes.create_string_buffer(max(nb.value, 1))
        flags = np.empty(n.value, np.uint8)
        check(lib.sw_seqs_export(h, _ptr(offs), blob, _ptr(flags)))
        c = (c_u64 * 2)()
        ms = (ctypes.c_double * 1)()
        check(lib.sw_seqs_stats(h, c, ms))
        out = (offs, blob.raw[:nb.value], (flags & SEQ_INEXACT).astype(bool))
        return out + (dict(launches=int(c[0]), bytes=int(c[1]), ms=ms[0]),) if stats else out
    finally:
        lib.sw_seqs_free(h)


def _distance_stats(c, ms) -> dict:
    d = dict(zip(("pairs", "cells", "striped_pairs", "longest", "launches", "block_cap"), (int(x) for x in c)))
    d.update(classify_ms=ms[0], distance_ms=ms[1])
    return d


class Index:
    """kmers / nodes / edges of a batch, resident on the device."""

    def __init__(self, handle: c_vp):
        self._h = handle

    def sizes(self):
        v = [c_u64() for _ in range(3)]
        check(lib.sw_index_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def timings(self) -> dict:
        t = Timings()
        check(lib.sw_index_timings(self._h, ctypes.byref(t)))
        return {name: getattr(t, name) for name, _ in Timings._fields_}

    def export(self):
        nk, nn, ne = self.sizes()
        kmers = np.empty(nk, KMER_DTYPE)
        nodes = np.empty(nn, NODE_DTYPE)
        edges = np.empty(ne, EDGE_DTYPE)
        check(lib.sw_index_export(self._h, _ptr(kmers), _ptr(nodes), _ptr(edges)))
        return kmers, nodes, edges

    def threshold_sums(self):
        """(sum n_tar, sum n_tar^2, sum n_tar*n_neg) over the nodes, computed on device (kmers.py:426-429)."""
        v = (c_u64 * 3)()
        check(lib.sw_index_threshold_sums(self._h, v))
        return tuple(int(x) for x in v)

    def filter_graph(self, edge_weight_th: float) -> "Index":
        """kmers._filter_edges_and_nodes on device: edges with weight > th and their endpoint nodes (no kmers)."""
        h = c_vp()
        check(lib.sw_index_filter_graph(self._h, c_u64(int(np.uintp(edge_weight_th))), ctypes.byref(h)))
        return Index(h)

    def filter_kmers(self, nodes_from: "Index", used_hashes) -> "Index":
        """filter_kmers on device: nodes of ``nodes_from`` whose hash is in ``used_hashes`` + their kmers from self.
        ``used_hashes`` may be a :class:`Subgraphs`: its device-resident ``used`` is taken then, with no host set."""
        h = c_vp()
        if isinstance(used_hashes, Subgraphs):
            check(lib.sw_index_filter_kmers_sg(self._h, nodes_from._h, used_hashes._h, ctypes.byref(h)))
            return Index(h)
        used = np.fromiter((int(x) for x in used_hashes), dtype=np.uint64)
        check(lib.sw_index_filter_kmers(self._h, nodes_from._h, _ptr(used), c_u64(len(used)), ctypes.byref(h)))
        return Index(h)

    @classmethod
    def from_arrays(cls, nodes, edges) -> "Index":
        """Upload a filtered graph given as host arrays (what kmers._filter_edges_and_nodes returns): nodes strictly ascending by
        hash, edges whose endpoints are among them.  An index without kmers, for :meth:`subgraphs`."""
        nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
        edges = np.ascontiguousarray(edges, EDGE_DTYPE)
        h = c_vp()
        check(lib.sw_index_from_arrays(_ptr(nodes), c_u64(len(nodes)), _ptr(edges), c_u64(len(edges)), ctypes.byref(h)))
        return cls(h)

    def subgraph_seeds(self, penalty_th: float) -> int:
        """Number of seeds of the subgraph walk: nodes of the graph with penalty <= penalty_th (kmers.py:243-245)."""
        n = c_u64()
        check(lib.sw_index_subgraph_seeds(self._h, ctypes.c_double(float(penalty_th)), ctypes.byref(n)))
        return n.value

    def subgraphs(self, penalty_th: float, min_nodes: int, max_nodes, rng) -> "Subgraphs":
        """kmers._get_subgraphs (src/seqwin/kmers.py:176-312) on a filtered index (:meth:`filter_graph`), on the device.

        ``rng`` (random.Random) is used exactly as the reference uses it -- one shuffle of the seeds, one of the subgraphs --
        and left in the same state: both shuffles are done on index lists of the same lengths.  Raises the reference's
        RuntimeError when no subgraph is kept."""
        th = float(penalty_th)
        n_seeds = self.subgraph_seeds(th)
        perm = list(range(n_seeds))
        rng.shuffle(perm)
        perm = np.asarray(perm, np.uint64)
        mx = _U64_MAX if max_nodes is None else max(int(max_nodes), 0)
        h = c_vp()
        check(lib.sw_index_subgraphs(self._h, ctypes.c_double(th), c_u64(max(int(min_nodes), 0)), c_u64(mx), _ptr(perm),
                                     c_u64(n_seeds), ctypes.byref(h)))
        sg = Subgraphs(h)
        n_sg = sg.sizes()[0]
        if n_sg == 0:
            sg.close()
            raise RuntimeError(NO_SUBGRAPH_MSG)
        order = list(range(n_sg))
        rng.shuffle(order)
        sg.order = np.asarray(order, np.int64)
        return sg

    def marker_locs(self, subgraphs: "Subgraphs", record_offsets, n_tar: int, kmerlen: int, windowsize: int,
                    keep_rows: bool = False) -> "Markers":
        """markers._get_cks' per-subgraph work (src/seqwin/markers.py:192-299) on the device (csrc/markers.hip): where every
        subgraph lies in every assembly and its representative k-mer ordering.  ``self`` is the kept index
        (``ix.filter_kmers(f, subgraphs)``).  Raises ValueError, as the reference does, when a subgraph lies in no target."""
        ro = np.ascontiguousarray(record_offsets, np.uint32)
        if ro.ndim != 1 or len(ro) < 1:
            raise ValueError("record_offsets needs one entry per assembly and one more")
        h = c_vp()
        check(lib.sw_index_marker_locs(self._h, subgraphs._h, _ptr(ro), c_u64(max(len(ro) - 1, 0)), c_u64(int(n_tar)),
                                       c_u64(int(kmerlen)), c_u64(int(windowsize)), ctypes.c_int(1 if keep_rows else 0),
                                       ctypes.byref(h)))
        return Markers(h, subgraphs.order)

    def save_npz(self, path, record_offsets) -> None:
        """Write ``graph.npz`` exactly as ``--save-graph`` does (src/seqwin/core.py:134-145)."""
        kmers, nodes, edges = self.export()
        np.savez(path, allow_pickle=False, kmers=kmers, nodes=nodes, edges=edges,
                 record_offsets=np.asarray(record_offsets, np.uint32))

    def checksums(self, kmer_base: int = 0, node_base: int = 0, edge_base: int = 0):
        """(kmers, nodes, edges) checksums; with bases: this slice's share of the checksums of the concatenated arrays
        (the shares of all slices add up modulo 2^64)."""
        v = (c_u64 * 3)()
        check(lib.sw_index_checksums_at(self._h, c_u64(kmer_base), c_u64(node_base), c_u64(edge_base), v))
        return tuple(int(x) for x in v)

    def verify(self, n_assemblies: int, scored: bool = True) -> dict:
        """Device-side self-check (sw_index_verify): violation counts of the output's structural properties."""
        v = (c_u64 * 10)()
        check(lib.sw_index_verify(self._h, c_u64(n_assemblies), ctypes.c_int(1 if scored else 0), v))
        names = ("node_order", "node_ranges", "kmer_order", "edge_order", "edge_first_gt_second", "edge_weight_range",
                 "edge_endpoint_missing", "count_range", "weight_sum", "reserved")
        return dict(zip(names, (int(x) for x in v)))

    def close(self) -> None:
        if self._h:
            lib.sw_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_U64_MAX = (1 << 64) - 1
NO_SUBGRAPH_MSG = ('No low-penalty subgraph was found. '
                   'Try decrease --stringency, or increase --penalty-th (penalty threshold, check log for the calculated value)')


class Subgraphs:
    """Low-penalty subgraphs of a filtered index, resident on the device (:meth:`Index.subgraphs`).

    The device keeps them in commit order; ``order`` is the reference's final rng.shuffle of that list (kmers.py:309):
    subgraph i of the result is committed subgraph order[i]."""

    def __init__(self, handle: c_vp):
        self._h = handle
        self.order = np.zeros(0, np.int64)

    def sizes(self):
        """(subgraphs, their nodes, induced edges, nodes of the filtered graph)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_subgraphs_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def csr(self):
        """(offsets[n_sg + 1], hashes) in the final order, hashes ascending inside every subgraph."""
        n_sg, n_out, _, _ = self.sizes()
        offs = np.empty(n_sg + 1, np.uint64)
        hashes = np.empty(n_out, np.uint64)
        check(lib.sw_subgraphs_export(self._h, _ptr(offs), _ptr(hashes), None, None, None, None))
        return _reorder(offs, hashes, self.order)

    def as_reference(self):
        """(tuple[frozenset[np.uint64], ...], frozenset[np.uint64]): what kmers._get_subgraphs returns."""
        offs, hashes = self.csr()
        vals = list(hashes)   # np.uint64 elements, as the reference's sets hold them
        o = offs.tolist()
        sgs = tuple(frozenset(vals[o[i]:o[i + 1]]) for i in range(len(o) - 1))
        return sgs, frozenset(vals)

    def used_hashes(self) -> np.ndarray:
        """The hashes of all subgraph nodes, ascending."""
        n_out = self.sizes()[1]
        out = np.empty(n_out, np.uint64)
        check(lib.sw_subgraphs_export(self._h, None, None, None, None, None, _ptr(out)))
        return out

    def used_mask(self) -> np.ndarray:
        """bool[n] over the filtered graph's nodes."""
        n = self.sizes()[3]
        out = np.empty(n, np.uint8)
        check(lib.sw_subgraphs_export(self._h, None, None, None, None, _ptr(out), None))
        return out.astype(bool)

    def induced_edges(self):
        """For every subgraph (final order): the filtered edges with both endpoints in it (nx_graph.subgraph(sg), markers.py:418),
        in edge order."""
        n_sg, _, n_ie, _ = self.sizes()
        offs = np.empty(n_sg + 1, np.uint64)
        edges = np.empty(n_ie, EDGE_DTYPE)
        check(lib.sw_subgraphs_export(self._h, None, None, _ptr(offs), _ptr(edges), None, None))
        o = offs.astype(np.int64)
        return [edges[o[i]:o[i + 1]] for i in self.order.tolist()]

    def stats(self) -> dict:
        c = (c_u64 * 10)()
        ms = (ctypes.c_double * 3)()
        check(lib.sw_subgraphs_stats(self._h, c, ms))
        names = ("seeds", "rounds", "expansions", "invalidated", "skipped_used", "kept", "discarded", "max_frontier", "spilled",
                 "window")
        d = dict(zip(names, (int(x) for x in c)))
        d.update(adjacency_ms=ms[0], walk_ms=ms[1], results_ms=ms[2])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_subgraphs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MARKER_ROW_DTYPE = np.dtype([("assembly_idx", "<u4"), ("record_idx", "<u4"), ("start", "<u4"), ("stop", "<u4"), ("n_kmers", "<u4"),
                             ("n_repeats", "<u4")])
MARKER_REP_DTYPE = np.dtype(MARKER_ROW_DTYPE.descr + [("n_rep", "<u4"), ("flags", "<u4")])
MARKER_SINGLE, MARKER_DUP, MARKER_NO_TARGET = 1, 2, 4


class Markers:
    """Location and representative of every subgraph (:meth:`Index.marker_locs`), resident on the device.

    The device keeps the subgraphs in commit order; every table handed out here is in the final order (``Subgraphs.order``, as
    ``Subgraphs.csr`` applies it).  ``len`` of a row is ``stop - start`` in uint32, as the reference's column."""

    def __init__(self, handle: c_vp, order=None):
        self._h = handle
        n_sg = self.sizes()[0]
        self.order = np.arange(n_sg, dtype=np.int64) if order is None else np.asarray(order, np.int64)
        if len(self.order) != n_sg:
            self.close()
            raise ValueError(f"the order has {len(self.order)} entries for {n_sg} subgraphs")
        reps = self._reps_raw()[0]
        bad = np.flatnonzero(reps["flags"][self.order] & MARKER_NO_TARGET)
        if len(bad):
            self.close()
            raise ValueError(f"subgraph {int(bad[0])} lies in no target assembly (max() of an empty sequence in the reference)")

    @classmethod
    def from_arrays(cls, kmers, nodes, sg_offsets, sg_nodes, record_offsets, n_tar: int, kmerlen: int, windowsize: int,
                    keep_rows: bool = False, order=None) -> "Markers":
        """The direct route on host arrays: nodes ascending by hash with [start, stop) into kmers, subgraphs as CSR of node
        indices."""
        kmers = np.ascontiguousarray(kmers, KMER_DTYPE)
        nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
        so = np.ascontiguousarray(sg_offsets, np.uint64)
        sn = np.ascontiguousarray(sg_nodes, np.uint64)
        ro = np.ascontiguousarray(record_offsets, np.uint32)
        if len(so) < 1 or len(ro) < 1 or int(so[-1]) != len(sn):
            raise ValueError("sg_offsets / record_offsets need at least one entry and sg_offsets[-1] == len(sg_nodes)")
        h = c_vp()
        check(lib.sw_marker_locs_from_arrays(_ptr(kmers), c_u64(len(kmers)), _ptr(nodes), c_u64(len(nodes)), _ptr(so), _ptr(sn),
                                             c_u64(len(so) - 1), _ptr(ro), c_u64(len(ro) - 1), c_u64(int(n_tar)), c_u64(int(kmerlen)),
                                             c_u64(int(windowsize)), ctypes.c_int(1 if keep_rows else 0), ctypes.byref(h)))
        return cls(h, order)

    def sizes(self):
        """(subgraphs, hashes of the representative orderings, rows, hashes of the rows' orderings -- 0 unless kept)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_markers_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _reps_raw(self):
        n_sg, n_rk, _, _ = self.sizes()
        reps = np.empty(n_sg, MARKER_REP_DTYPE)
        offs = np.empty(n_sg + 1, np.uint64)
        hashes = np.empty(n_rk, np.uint64)
        check(lib.sw_markers_export(self._h, _ptr(reps), _ptr(offs), _ptr(hashes)))
        return reps, offs, hashes

    def reps(self):
        """(reps[MARKER_REP_DTYPE], offsets, hashes): the representative row, n_rep and flags of every subgraph, and the
        representative orderings as CSR."""
        reps, offs, hashes = self._reps_raw()
        offs, hashes = _reorder(offs, hashes, self.order)
        return reps[self.order], offs, hashes

    def rows(self):
        """For every subgraph: (rows[MARKER_ROW_DTYPE] ascending by assembly, offsets, hashes of the rows' orderings) -- the
        reference's ``loc``.  Needs ``keep_rows=True``."""
        n_sg, _, n_rows, n_rk = self.sizes()
        row_offs = np.empty(n_sg + 1, np.uint64)
        rows = np.empty(n_rows, MARKER_ROW_DTYPE)
        k_offs = np.empty(n_rows + 1, np.uint64)
        hashes = np.empty(n_rk, np.uint64)
        check(lib.sw_markers_export_rows(self._h, _ptr(row_offs), _ptr(rows), _ptr(k_offs), _ptr(hashes)))
        ro, ko = row_offs.astype(np.int64), k_offs.astype(np.int64)
        out = []
        for i in self.order.tolist():
            a, b = ro[i], ro[i + 1]
            out.append((rows[a:b], (k_offs[a:b + 1] - k_offs[a]), hashes[ko[a]:ko[b]]))
        return out

    def _selected(self, select) -> np.ndarray:
        """Device (commit-order) indices of the subgraphs ``select`` names in the final order; None: all of them."""
        sel = self.order if select is None else self.order[np.asarray(select, np.int64).reshape(-1)]
        return np.ascontiguousarray(sel, np.uint64)

    def sequences(self, batch: "Batch", which: str = "reps", select=None, stats: bool = False):
        """``(offsets, blob, inexact)`` as :meth:`Batch.fetch` returns them, of the representative rows (``which="reps"``) or of
        every row (``"rows"``, subgraph after subgraph, ascending by assembly: the concatenation of :meth:`rows`; needs
        ``keep_rows=True``) of the subgraphs ``select`` (indices in the final order; None: all), in that order.  The intervals are
        made on the device from the tables; a row's global record is ``batch.record_offsets()[assembly_idx] + record_idx``.
        ValueError if the batch's record table does not cover the markers' records."""
        if which not in ("reps", "rows"):
            raise ValueError(f'which must be "reps" or "rows" (got {which!r})')
        sel = self._selected(select)
        h = c_vp()   # ("rows" without the rows kept: the library's ValueError, as rows() gives it)
        check(lib.sw_markers_fetch(self._h, batch._h, ctypes.c_int(1 if which == "rows" else 0), _ptr(sel), c_u64(len(sel)), ctypes.byref(h)))
        return _export_seqs(h, stats)

    def row_distances(self, batch: "Batch", select=None, stats: bool = False):
        """``(dist, strand)`` of :meth:`Batch.edit_distances` with R = the subgraph's representative interval and S = the row's, one
        entry per kept row in the order of ``sequences(batch, "rows", select)``.  A representative's own row reads (0, 0) when it
        holds no invalid base.  Needs ``keep_rows=True``; ValueError if the batch's record table does not cover the markers' records."""
        sel = self._selected(select)
        row_offs = np.empty(self.sizes()[0] + 1, np.uint64)
        check(lib.sw_markers_export_rows(self._h, _ptr(row_offs), None, None, None))   # ValueError unless the rows were kept
        n = int(np.diff(row_offs.astype(np.int64))[sel.astype(np.int64)].sum())
        dist = np.empty(n, np.uint32)
        strand = np.empty(n, np.uint8)
        c = (c_u64 * 6)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_markers_row_distances(self._h, batch._h, _ptr(sel), c_u64(len(sel)), _ptr(dist), _ptr(strand), c, ms))
        return (dist, strand, _distance_stats(c, ms)) if stats else (dist, strand)

    def screen(self, batch: "Batch", kmerlen: int, select=None, profile=None, n_groups=None, copies: bool = False) -> "Screen":
        """:meth:`Batch.screen` of the representatives' text -- ``sequences(batch, "reps", select)``, in that order -- against every
        assembly of ``batch``.  A flagged (inexact) representative is screened as fetched: its ``N``s carry no k-mers.  ``kmerlen``
        is the caller's choice; it need not be the graph's k.  ``profile``, ``n_groups`` and ``copies`` are that call's: the k-mer
        profile of every position of every representative, by group of assembly."""
        offs, blob, _ = self.sequences(batch, "reps", select)
        o = offs.astype(np.int64)
        return batch.screen([blob[o[i]:o[i + 1]] for i in range(len(o) - 1)], kmerlen, profile=profile, n_groups=n_groups, copies=copies)

    def best_hits(self, batch: "Batch", kmerlen: int, select=None, align: bool = False, loci: bool = False, min_seeds: int = 1,
                  seed_copies=None, local: bool = False, scoring=(2, -3, 5, 2), pileup=None, n_groups=None, max_dist_permille: int = 1000,
                  window_lengths=None, window_mismatch: int = 2, window_three_prime: int = 3) -> "BestHits":
        """:meth:`Batch.best_hits` of the representatives' text -- ``sequences(batch, "reps", select)``, in that order -- against
        every assembly of ``batch``.  ``kmerlen`` is the caller's choice; it need not be the graph's k.  ``seed_copies`` is that
        call's: ``None`` keeps a k-mer as a seed only if one window of all representatives has it, ``c`` in 1..256 lets up to c
        windows share it (representatives that overlap or repeat keep their k-mers) and drops a k-mer with more windows whole.
        ``local`` and ``scoring`` are that call's too: the local alignment of every winner (and locus) with affine gap scores; so
        are ``pileup``, ``n_groups`` and ``max_dist_permille``: the winners' base counts per position of every representative, by
        group of assembly; and ``window_lengths``, ``window_mismatch`` and ``window_three_prime``: the joint mismatch classes of every
        window of every representative (it needs ``pileup``)."""
        offs, blob, _ = self.sequences(batch, "reps", select)
        o = offs.astype(np.int64)
        return batch.best_hits([blob[o[i]:o[i + 1]] for i in range(len(o) - 1)], kmerlen, align=align, loci=loci, min_seeds=min_seeds,
                               seed_copies=seed_copies, local=local, scoring=scoring, pileup=pileup, n_groups=n_groups,
                               max_dist_permille=max_dist_permille, window_lengths=window_lengths, window_mismatch=window_mismatch,
                               window_three_prime=window_three_prime)

    def candidates(self, min_len: int) -> np.ndarray:
        """Indices of the subgraphs the reference keeps (markers.py:514-517): len >= min_len, neither single nor dup."""
        reps = self.reps()[0]
        length = (reps["stop"] - reps["start"]).astype(np.uint32)
        return np.flatnonzero((length >= min_len) & ((reps["flags"] & (MARKER_SINGLE | MARKER_DUP)) == 0))

    def stats(self) -> dict:
        c = (c_u64 * 4)()
        ms = (ctypes.c_double * 4)()
        check(lib.sw_markers_stats(self._h, c, ms))
        d = dict(zip(("pairs", "spilled", "largest_pair", "vote_spilled"), (int(x) for x in c)))
        d.update(count_ms=ms[0], rows_ms=ms[1], vote_ms=ms[2], results_ms=ms[3])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_markers_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _block_range(r, n: int):
    """None, (lo, hi), a slice or a range of step 1 -> (lo, hi)."""
    if r is None:
        return 0, n
    if isinstance(r, slice):
        lo, hi, step = r.indices(n)
        r = range(lo, max(hi, lo), step)
    if isinstance(r, range):
        if r.step != 1:
            raise ValueError("rows / cols must be contiguous")
        return r.start, max(r.stop, r.start)
    lo, hi = r
    return int(lo), int(hi)


def _cell_block(fn, handle, field, n_rows: int, n_cols: int, rows, cols, dtype=np.uint32) -> np.ndarray:
    """``rows`` x ``cols`` of a ``[n_rows][n_cols]`` table of 32-bit cells, copied out by the library's block export ``fn``;
    ``field`` selects the table (None: ``fn`` takes none)."""
    (r0, r1), (c0, c1) = _block_range(rows, n_rows), _block_range(cols, n_cols)
    out = np.empty((max(r1 - r0, 0), max(c1 - c0, 0)), dtype)
    which = () if field is None else (c_u64(field),)
    check(fn(handle, *which, c_u64(r0), c_u64(r1), c_u64(c0), c_u64(c1), _ptr(out)))
    return out


class MinHash:
    """MinHash sketches of a set of assemblies, resident on the device (:meth:`Batch.minhash`, :meth:`from_sketches`), and the
    pair counts ``mash dist`` derives from them: what ``Assemblies.mash`` (src/seqwin/assemblies.py:76-99) gets from the Mash
    binary.  ``rows`` / ``cols`` are None (all), a ``(lo, hi)`` pair, a slice or a range."""

    def __init__(self, handle: c_vp):
        self._h = handle

    @classmethod
    def from_sketches(cls, offsets, hashes, sketchsize: int, hash_bits: int = 64) -> "MinHash":
        """Sketches given as host arrays in CSR form: strictly ascending lists of at most ``sketchsize`` values."""
        offs = np.ascontiguousarray(offsets, np.uint64)
        hs = np.ascontiguousarray(hashes, np.uint64)
        if offs.ndim != 1 or len(offs) < 1 or int(offs[-1]) != len(hs):
            raise ValueError("offsets needs one entry per sketch and one more, and offsets[-1] == len(hashes)")
        h = c_vp()
        check(lib.sw_minhash_from_sketches(_ptr(offs), _ptr(hs), c_u64(len(offs) - 1), c_u64(int(sketchsize)), c_u64(int(hash_bits)),
                                           ctypes.byref(h)))
        return cls(h)

    def sizes(self):
        """(sketches, hashes of all sketches, sketch size, hash bits)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_minhash_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def __len__(self) -> int:
        return self.sizes()[0]

    def sketches(self):
        """(offsets[n + 1], hashes): sketch a is hashes[offsets[a]:offsets[a + 1]], ascending, uint64."""
        n, nh, _, _ = self.sizes()
        offs = np.empty(n + 1, np.uint64)
        hs = np.empty(nh, np.uint64)
        check(lib.sw_minhash_export(self._h, _ptr(offs), _ptr(hs)))
        return offs, hs

    def counts(self, rows=None, cols=None):
        """(shared, total): uint32[rows, cols] of the block, as ``mash dist`` reports them (``shared/total`` in its output)."""
        n = self.sizes()[0]
        (r0, r1), (c0, c1) = _block_range(rows, n), _block_range(cols, n)
        shape = (max(r1 - r0, 0), max(c1 - c0, 0))
        shared = np.empty(shape, np.uint32)
        total = np.empty(shape, np.uint32)
        check(lib.sw_minhash_counts(self._h, c_u64(r0), c_u64(r1), c_u64(c0), c_u64(c1), _ptr(shared), _ptr(total)))
        return shared, total

    def jaccard(self, rows=None, cols=None) -> np.ndarray:
        """float64[rows, cols]: ``shared / total`` as Python divides the two ints the reference parses (a pair of two empty
        sketches raises ZeroDivisionError, as that division does)."""
        shared, total = self.counts(rows, cols)
        if np.any(total == 0):
            raise ZeroDivisionError("division by zero")
        return shared.astype(np.float64) / total.astype(np.float64)

    def frac_rowsums(self, rows=None, cols=None) -> np.ndarray:
        """Per row of the block: the sum of 2J / (1 + J) over its columns, added on the device in a fixed order."""
        n = self.sizes()[0]
        (r0, r1), (c0, c1) = _block_range(rows, n), _block_range(cols, n)
        out = np.empty(max(r1 - r0, 0), np.float64)
        try:
            check(lib.sw_minhash_frac_rowsums(self._h, c_u64(r0), c_u64(r1), c_u64(c0), c_u64(c1), _ptr(out)))
        except ValueError as e:
            if "division by zero" in str(e):
                raise ZeroDivisionError("division by zero") from None
            raise
        return out

    def expected_frac(self, rows=None, cols=None) -> float:
        """kmers._expected_frac (src/seqwin/kmers.py:315-323) of the block's Jaccard matrix: mean(2J / (1 + J)), without
        materialising the matrix on the host."""
        sums = self.frac_rowsums(rows, cols)
        n = self.sizes()[0]
        (r0, r1), (c0, c1) = _block_range(rows, n), _block_range(cols, n)
        return float(np.float64(sums.sum()) / np.float64((r1 - r0) * (c1 - c0)))

    def penalty_fracs(self, n_tar: int):
        """(e_absence_tar, e_presence_neg) of kmers.filter_graph (src/seqwin/kmers.py:419-420); targets are the first ``n_tar``
        assemblies."""
        n = self.sizes()[0]
        n_tar = int(n_tar)
        if not 0 < n_tar < n:
            raise ValueError(f"n_tar = {n_tar} must leave a target and a non-target among the {n} assemblies")
        return 1 - self.expected_frac((0, n_tar), (0, n_tar)), self.expected_frac((n_tar, n), (0, n_tar))

    def stats(self) -> dict:
        c = (c_u64 * 4)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_minhash_stats(self._h, c, ms))
        d = dict(zip(("general_route", "candidates", "largest_candidates", "capacity"), (int(x) for x in c)))
        d.update(hash_ms=ms[0], select_ms=ms[1])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_minhash_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Screen:
    """Exact k-mer containment counts of a list of queries in every assembly of a batch, resident on the device
    (:meth:`Batch.screen`, :meth:`Markers.screen`; csrc/screen.hip).  It stands where ``eval_markers`` (src/seqwin/markers.py:607-696)
    BLASTs the representatives, has no counterpart in the reference, is not BLAST and fills none of ``MarkerMetrics``.
    ``rows`` (queries) / ``cols`` (assemblies) are None (all), a ``(lo, hi)`` pair, a slice or a range.  A screen made with
    ``profile=groups`` also answers :meth:`profile`."""

    def __init__(self, handle: c_vp, offsets=None, copies: bool = False):
        self._h = handle
        self._offs = None if offsets is None else np.array(offsets, np.uint64)   # (of a call with a profile)
        self._copies = bool(copies)

    def profile(self) -> "KmerProfile":
        """The :class:`KmerProfile` of a screen made with ``profile=groups``; ValueError for any other."""
        if self._offs is None:
            raise ValueError("this screen was made without a profile (screen(..., profile=groups) makes one)")
        return KmerProfile(self, self._offs, self._copies)

    def sizes(self):
        """(queries, assemblies, distinct canonical k-mers of all queries, k)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_screen_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def n_kmers(self) -> np.ndarray:
        """uint32[queries]: the distinct canonical k-mers of every query (0: shorter than k, or no valid window)."""
        out = np.empty(self.sizes()[0], np.uint32)
        check(lib.sw_screen_n_kmers(self._h, _ptr(out)))
        return out

    def counts(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: how many of the query's distinct canonical k-mers occur in the assembly."""
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_screen_counts, self._h, None, nq, na, rows, cols)

    def containment(self, rows=None, cols=None) -> np.ndarray:
        """float64[rows, cols]: ``counts / n_kmers``; ``nan`` for a query without a k-mer."""
        r0, r1 = _block_range(rows, self.sizes()[0])
        nk = self.n_kmers()[r0:r1].astype(np.float64)
        nk[nk == 0] = np.nan
        return self.counts(rows, cols).astype(np.float64) / nk[:, None]

    def stats(self) -> dict:
        c = (c_u64 * 10)()
        ms = (ctypes.c_double * 3)()
        check(lib.sw_screen_stats(self._h, c, ms))
        d = dict(zip(("query_positions", "query_kmers", "distinct_kmers", "table_capacity", "longest_chain", "batch_kmers", "hits", "atomics",
                      "chunks", "launches"), (int(x) for x in c)))
        probe = (ctypes.c_double * max(d["chunks"], 1))()
        reduce_ = (ctypes.c_double * max(d["chunks"], 1))()
        check(lib.sw_screen_chunk_ms(self._h, probe, reduce_))
        d.update(table_ms=ms[0], probe_ms=ms[1], reduce_ms=ms[2], chunk_probe_ms=list(probe)[:d["chunks"]],
                 chunk_reduce_ms=list(reduce_)[:d["chunks"]])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_screen_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KmerProfile:
    """Per position of every query and per group of assemblies: in how many assemblies of the group the canonical k-mer of the window
    that starts there occurs anywhere (``present``), and how many valid windows of those assemblies hold it (``copies``, with
    ``copies=True``) -- ``Screen.profile()`` of a ``screen(..., profile=groups)``; csrc/screen.hip, DESIGN.md section 3.2m.  Every locus
    of every assembly on both strands, exactly; a window counts once whatever its strand.  A row where no window starts (the last
    k - 1 bytes of a query, a window with an invalid byte, a query shorter than k) reads ``NO_WINDOW`` in ``present`` and
    ``NO_WINDOW_COPIES`` in ``copies``.  It has no counterpart in the reference, is not BLAST and fills none of ``MarkerMetrics``:
    no mismatches, no Tm, no dG.  :mod:`seqwin_amd.kprofile` reads it."""

    NO_WINDOW = 0xFFFFFFFF
    NO_WINDOW_COPIES = 0xFFFFFFFFFFFFFFFF

    def __init__(self, screen: "Screen", offsets: np.ndarray, copies: bool):
        self._screen = screen   # (the tables live in the screen's handle)
        self._offs = np.array(offsets, np.uint64)
        self._has_copies = bool(copies)
        self._tab = None

    @property
    def k(self) -> int:
        return self._screen.sizes()[3]

    def sizes(self):
        """(rows: the bytes of all queries, groups, whether copies were counted)"""
        v = [c_u64() for _ in range(3)]
        check(lib.sw_screen_profile_sizes(self._screen._h, *[ctypes.byref(x) for x in v]))
        return v[0].value, v[1].value, bool(v[2].value)

    def _export(self):
        if self._tab is None:
            rows, ng, has = self.sizes()
            present = np.empty((rows, ng), np.uint32)
            cop = np.empty((rows, ng), np.uint64) if has else None
            sizes = np.empty(ng, np.uint32)
            check(lib.sw_screen_profile_export(self._screen._h, _ptr(present), _ptr(cop) if has else None, _ptr(sizes)))
            self._tab = (present, cop, sizes)
        return self._tab

    def _query(self, q: int):
        q = int(q)
        if not 0 <= q < len(self._offs) - 1:
            raise ValueError(f"query {q} is none of the call's {len(self._offs) - 1}")
        return int(self._offs[q]), int(self._offs[q + 1])

    def present(self, q: int) -> np.ndarray:
        """uint32[len(query q), groups]"""
        lo, hi = self._query(q)
        return self._export()[0][lo:hi].copy()

    def copies(self, q: int) -> np.ndarray:
        """uint64[len(query q), groups]; ValueError for a profile made without ``copies=True``."""
        if not self._has_copies:
            raise ValueError("this profile was made without copies (screen(..., profile=groups, copies=True) counts them)")
        lo, hi = self._query(q)
        return self._export()[1][lo:hi].copy()

    def table(self):
        """``(offsets, present uint32[total, groups], copies uint64[total, groups] or None)``: the rows of query q are
        ``[offsets[q], offsets[q + 1])``."""
        present, cop, _ = self._export()
        return self._offs.copy(), present.copy(), None if cop is None else cop.copy()

    def group_sizes(self) -> np.ndarray:
        """uint32[groups]: the assemblies of every label."""
        return self._export()[2].copy()

    def stats(self) -> dict:
        c = (c_u64 * 2)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_screen_profile_stats(self._screen._h, c, ms))
        return dict(table_bytes=int(c[0]), copy_adds=int(c[1]), profile_ms=ms[0], gather_ms=ms[1])


SITE_FIELDS = ("oligo", "assembly", "record", "pos", "strand", "mm")
SITE_FIELDS_EDIT = ("oligo", "assembly", "record", "pos", "strand", "end", "mismatch", "gaps")


class OligoHits:
    """The sites of a list of oligos in every assembly of a batch, resident on the device (:meth:`Batch.oligo_hits`; csrc/oligo.hip,
    DESIGN.md section 3.2j): per (oligo, assembly) ``n_sites``, the number of hits on both strands, and the hit that is least in the
    order (mm, record, pos, strand) as ``best_mm``, ``best_record`` (global), ``best_pos`` and ``best_strand`` -- NO_HIT without a
    hit.  It has no counterpart in the reference, is not BLAST and fills none of ``MarkerMetrics``.  Made with ``thermo=`` (DESIGN.md
    section 3.2o) it also holds ``n_stable`` and the ``stable_*`` fields of the hit that is least in (dg, record, pos, strand).  A
    single-device object on a resident batch.  ``rows`` (oligos) / ``cols`` (assemblies) are None (all), a ``(lo, hi)`` pair, a slice
    or a range.  Made with ``sites=True`` it also holds the list of all hits.

    Made with ``max_edits`` a site has a ``pos``, an ``end``, a ``dist`` = ``mismatch`` + ``gaps``; the best
    site is the least in (dist, record, pos, strand), then end, and ``best_mm`` is a ValueError: ask for ``best_dist``.  On a result
    without it ``dist`` and ``mismatch`` are ``mm``, ``end`` is ``pos + L`` and ``gaps`` is 0."""

    def __init__(self, handle: c_vp, lengths, sites: bool = False, thermo: bool = False):
        self._h = handle
        self.lengths = np.asarray(lengths, np.uint32)
        self._sites = sites
        self.thermo = thermo
        v = ctypes.c_int64()
        check(lib.sw_oligos_max_edits(self._h, ctypes.byref(v)))
        self.max_edits = None if v.value < 0 else int(v.value)

    def sizes(self):
        """(oligos, assemblies, max_mismatch, three_prime)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_oligos_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _block(self, field: int, rows, cols) -> np.ndarray:
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_oligos_block, self._h, field, nq, na, rows, cols)

    def n_sites(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the hits of the oligo in the assembly, both strands together; 0: none."""
        return self._block(0, rows, cols)

    def best_mm(self, rows=None, cols=None) -> np.ndarray:
        if self.max_edits is not None:
            raise ValueError("these oligo hits were made with max_edits: ask for best_dist, best_mismatch and best_gaps")
        return self._block(1, rows, cols)

    def best_dist(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the best site's edit distance (without ``max_edits``: its mismatches); NO_HIT without a site."""
        return self._block(1, rows, cols)

    def best_end(self, rows=None, cols=None) -> np.ndarray:
        return self._block(5, rows, cols)

    def best_mismatch(self, rows=None, cols=None) -> np.ndarray:
        return self._block(6, rows, cols)

    def best_gaps(self, rows=None, cols=None) -> np.ndarray:
        return self._block(7, rows, cols)

    def best_record(self, rows=None, cols=None) -> np.ndarray:
        return self._block(2, rows, cols)

    def best_pos(self, rows=None, cols=None) -> np.ndarray:
        return self._block(3, rows, cols)

    def best_strand(self, rows=None, cols=None) -> np.ndarray:
        return self._block(4, rows, cols)

    def _thermo_block(self, field: int, rows, cols, dtype) -> np.ndarray:
        if not self.thermo:
            raise ValueError("these oligo hits were made without thermo=")
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_oligos_thermo_block, self._h, field, nq, na, rows, cols, dtype)

    def n_stable(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the hits with ``dg <= max_dg`` (every hit without a ``max_dg``).  This and the ``stable_*`` fields:
        ValueError on a result made without ``thermo=``."""
        return self._thermo_block(0, rows, cols, np.uint32)

    def stable_dg(self, rows=None, cols=None) -> np.ndarray:
        """int32[rows, cols], cal/mol: dg of the most stable hit -- the least in (dg, record, pos, strand) among all hits, stable or
        not; INT32_MIN (``oligos.NO_SUM``) without a hit, as ``stable_dh`` and ``stable_ds``."""
        return self._thermo_block(1, rows, cols, np.int32)

    def stable_dh(self, rows=None, cols=None) -> np.ndarray:
        return self._thermo_block(2, rows, cols, np.int32)

    def stable_ds(self, rows=None, cols=None) -> np.ndarray:
        return self._thermo_block(3, rows, cols, np.int32)

    def stable_record(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the most stable hit's record (global); NO_HIT without a hit, as ``stable_pos``, ``stable_strand`` and
        ``stable_mm``."""
        return self._thermo_block(4, rows, cols, np.uint32)

    def stable_pos(self, rows=None, cols=None) -> np.ndarray:
        return self._thermo_block(5, rows, cols, np.uint32)

    def stable_strand(self, rows=None, cols=None) -> np.ndarray:
        return self._thermo_block(6, rows, cols, np.uint32)

    def stable_mm(self, rows=None, cols=None) -> np.ndarray:
        return self._thermo_block(7, rows, cols, np.uint32)

    def sites(self) -> dict:
        """Every hit, ascending by (oligo, assembly, record, pos, strand), as parallel uint32 arrays ``oligo``, ``assembly``,
        ``record``, ``pos``, ``strand``, ``end``, ``dist``, ``mismatch``, ``gaps`` -- and ``mm`` on a result without ``max_edits``;
        with it the order is (oligo, assembly, record, pos, end, strand).  ``cell_offsets`` (uint64[oligos * assemblies + 1]) bounds
        the hits of every pair."""
        if not self._sites:
            raise ValueError("these oligo hits were made without sites=True")
        nq, na, _, _ = self.sizes()
        n = c_u64()
        check(lib.sw_oligos_sites_size(self._h, ctypes.byref(n)))
        offs = np.empty(nq * na + 1, np.uint64)
        if self.max_edits is None:     # the call and the columns of section 3.2j; the four new ones follow from them
            cols = [np.empty(n.value, np.uint32) for _ in SITE_FIELDS]
            check(lib.sw_oligos_sites(self._h, _ptr(offs), *[_ptr(a) if n.value else None for a in cols]))
            out = dict(zip(SITE_FIELDS, cols))
            out.update(end=out["pos"] + self.lengths[out["oligo"]], dist=out["mm"].copy(), mismatch=out["mm"].copy(), gaps=np.zeros(n.value, np.uint32))
            if self.thermo:                # int32 dh, ds, dg of every entry (section 3.2o)
                sums = [np.empty(n.value, np.int32) for _ in range(3)]
                check(lib.sw_oligos_sites_thermo(self._h, *[_ptr(a) if n.value else None for a in sums]))
                out.update(dh=sums[0], ds=sums[1], dg=sums[2])
        else:
            cols = [np.empty(n.value, np.uint32) for _ in SITE_FIELDS_EDIT]
            check(lib.sw_oligos_sites_edit(self._h, _ptr(offs), *[_ptr(a) if n.value else None for a in cols]))
            out = dict(zip(SITE_FIELDS_EDIT, cols))
            out["dist"] = out["mismatch"] + out["gaps"]
        out["cell_offsets"] = offs
        return out

    def intervals(self) -> np.ndarray:
        """INTERVAL_DTYPE ``(record, pos, end)`` of every hit, in the list's order, as :meth:`Batch.fetch` takes them (the text
        of a strand-1 hit faces the oligo's reverse complement); ``end`` is ``pos + L`` unless the site has gaps."""
        S = self.sites()
        iv = np.empty(len(S["oligo"]), INTERVAL_DTYPE)
        iv["record"], iv["start"], iv["stop"] = S["record"], S["pos"], S["end"]
        return iv

    def stats(self) -> dict:
        """``windows`` (window ends scanned, summed over the passes), ``passes`` (groups of oligos), ``chunks`` (of assemblies),
        ``launches``, ``hits``, ``buffer_doublings``, ``chunk_splits``, ``comparisons`` (window x oligo x strand), ``scan_ms`` and
        ``order_ms`` (HIP events); ``dp_steps`` (steps of the bit-vector column, an upper bound), ``candidates`` (resolved by the
        alignment kernel) and ``resolve_ms`` -- zeros without ``max_edits``; with it ``scan_ms`` excludes ``resolve_ms``.
        ``stable_hits`` (the sum of ``n_stable``), ``thermo_ms`` (the kernel of the ``stable_*`` fields; ``scan_ms`` excludes it)
        and ``site_thermo_ms`` (the kernel of the list's sums) -- zeros without ``thermo=``."""
        c = (c_u64 * 8)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_oligos_stats(self._h, c, ms))
        d = dict(zip(("windows", "passes", "chunks", "launches", "hits", "buffer_doublings", "chunk_splits", "comparisons"), (int(x) for x in c)))
        d.update(scan_ms=ms[0], order_ms=ms[1])
        c2 = (c_u64 * 2)()
        ms2 = ctypes.c_double()
        check(lib.sw_oligos_edit_stats(self._h, c2, ctypes.byref(ms2)))
        d.update(dp_steps=int(c2[0]), candidates=int(c2[1]), resolve_ms=ms2.value)
        d.update(stable_hits=0, thermo_ms=0.0, site_thermo_ms=0.0)   # (zeros without thermo=)
        if self.thermo:
            n3 = c_u64()
            ms3 = (ctypes.c_double * 2)()
            check(lib.sw_oligos_thermo_stats(self._h, ctypes.byref(n3), ms3))
            d.update(stable_hits=int(n3.value), thermo_ms=ms3[0], site_thermo_ms=ms3[1])
        return d

    def amplicons(self, pairs, min_len: int, max_len: int, probes=None, products: bool = True, max_dg=None, stream: int = 0) -> "Amplicons":
        """The products of primer pairs over the resident site list, and the probes inside them (csrc/amplicons.hip, DESIGN.md
        section 3.2p): :func:`seqwin_amd.oligos.amplicons` on the device, with probes and a ``dg`` filter.  ``pairs`` is an (n, 2)
        array of ``(f, r)`` oligo indices (1..65 536 rows; a pair listed twice is two rows).  Orientation ``+`` (0): a site of f on
        strand 0 at ``pf`` and a site of r on strand 1 of the same record with ``pos_r >= pf``, product ``[pf, end_r)``; ``-`` (1):
        f and r exchanged; with ``f == r`` only ``+``.  A product is kept iff ``min_len <= end - start <= max_len``; every
        combination counts.  ``probes`` (None, or one entry per pair: an oligo index, or None / ``NO_PROBE`` for a pair without
        one): ``n_probe`` of a product counts the probe's sites in that record, on either strand, that lie strictly between the two
        primer sites (``end_first <= pos_p`` and ``end_p <= pos_last``).  ``max_dg`` (cal/mol; the hits must have been made with
        ``thermo=``): a PRIMER site takes part only if its ``dg <= max_dg``; probe sites are not filtered.  ``products=False``
        keeps the two count matrices only.  ValueError for anything else, before the library is called."""
        if not self._sites:
            raise ValueError("these oligo hits were made without sites=True")
        nq = len(self.lengths)
        try:
            p = np.asarray(pairs, np.int64).reshape(-1, 2)
        except (TypeError, ValueError):
            raise ValueError("pairs must be an (n, 2) array of oligo indices") from None
        if not 1 <= len(p) <= AMPLICON_MAX_PAIRS:
            raise ValueError(f"{len(p)} pairs; 1..{AMPLICON_MAX_PAIRS} are taken")
        if p.min() < 0 or p.max() >= nq:
            raise ValueError(f"a pair names an oligo outside the call's {nq}")
        if int(min_len) != min_len or int(max_len) != max_len or min_len < 1:
            raise ValueError(f"min_len and max_len must be integers of 1 or more (got {min_len!r}, {max_len!r})")
        if min_len > max_len:
            raise ValueError(f"min_len {min_len} exceeds max_len {max_len}")
        pr = None
        if probes is not None:
            pl = [NO_PROBE if x is None else int(x) for x in probes]
            if len(pl) != len(p):
                raise ValueError(f"{len(pl)} probes for {len(p)} pairs")
            if any(x != NO_PROBE and not 0 <= x < nq for x in pl):
                raise ValueError(f"a probe names an oligo outside the call's {nq}")
            pr = np.asarray(pl, np.uint32)
        if max_dg is not None:
            if not self.thermo:
                raise ValueError("max_dg needs oligo hits made with thermo=")
            try:
                whole = int(max_dg) == max_dg and -2 ** 31 <= int(max_dg) < 2 ** 31
            except (TypeError, ValueError, OverflowError):
                whole = False
            if not whole:
                raise ValueError(f"max_dg must be an integer of cal/mol that fits int32 (got {max_dg!r})")
        p32 = np.ascontiguousarray(p, np.uint32)
        h = c_vp()
        check(lib.sw_oligos_amplicons(self._h, _ptr(p32), None if pr is None else _ptr(pr), c_u64(len(p32)), c_u64(int(min_len)), c_u64(int(max_len)),
                                      ctypes.c_int(1 if products else 0), ctypes.c_int64(0 if max_dg is None else int(max_dg)),
                                      ctypes.c_int(1 if max_dg is None else 0), c_vp(stream), ctypes.byref(h)))
        return Amplicons(h, bool(products))

    def close(self) -> None:
        if self._h:
            lib.sw_oligos_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


AMPLICON_MAX_PAIRS = 65536
NO_PROBE = 0xFFFFFFFF
PRODUCT_FIELDS = ("pair", "assembly", "record", "start", "end", "orientation", "mm_f", "mm_r", "n_probe")


class Amplicons:
    """The products of primer pairs in every assembly, resident on the device (:meth:`OligoHits.amplicons`; csrc/amplicons.hip,
    DESIGN.md section 3.2p): per (pair, assembly) ``n_amplicons`` and ``n_detected``, the products with at least one probe site
    between the primers (zero for a pair without a probe), and -- made with ``products=True`` -- the list of products.  It has no
    counterpart in the reference.  It does not depend on the :class:`OligoHits` it came from.  ``rows`` (pairs) / ``cols``
    (assemblies) as for :class:`OligoHits`; either matrix goes to :func:`seqwin_amd.oligos.assay_summary` unchanged."""

    def __init__(self, handle: c_vp, products: bool):
        self._h = handle
        self._products = products

    def sizes(self):
        """(pairs, assemblies, min_len, max_len)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_amplicons_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _block(self, field: int, rows, cols) -> np.ndarray:
        n, na, _, _ = self.sizes()
        return _cell_block(lib.sw_amplicons_block, self._h, field, n, na, rows, cols)

    def n_amplicons(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the products of the pair in the assembly, both orientations together."""
        return self._block(0, rows, cols)

    def n_detected(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the products with ``n_probe >= 1``."""
        return self._block(1, rows, cols)

    def products(self) -> dict:
        """Every product, ascending by (pair, assembly, record, start, end, orientation, mm_f, mm_r) -- the order of
        :func:`seqwin_amd.oligos.amplicons` --, as parallel uint32 arrays of those names and ``n_probe``; ``cell_offsets``
        (uint64[pairs * assemblies + 1]) bounds the products of every cell.  ValueError on a result made with ``products=False``."""
        if not self._products:
            raise ValueError("these amplicons were made with products=False")
        n_pairs, na, _, _ = self.sizes()
        n = c_u64()
        check(lib.sw_amplicons_products_size(self._h, ctypes.byref(n)))
        offs = np.empty(n_pairs * na + 1, np.uint64)
        cols = [np.empty(n.value, np.uint32) for _ in PRODUCT_FIELDS]
        check(lib.sw_amplicons_products(self._h, _ptr(offs), *[_ptr(a) if n.value else None for a in cols]))
        out = dict(zip(PRODUCT_FIELDS, cols))
        out["cell_offsets"] = offs
        return out

    def intervals(self) -> np.ndarray:
        """INTERVAL_DTYPE ``(record, start, end)`` of every product, in the list's order, as :meth:`Batch.fetch` takes them."""
        P = self.products()
        iv = np.empty(len(P["pair"]), INTERVAL_DTYPE)
        iv["record"], iv["start"], iv["stop"] = P["record"], P["start"], P["end"]
        return iv

    def stats(self) -> dict:
        """``items`` (first sites offered to a pair and orientation), ``wave_items`` (those handed to the wave-per-item kernel),
        ``partners`` (sites visited as the other primer), ``products``, ``detected``, ``launches``; ``count_ms``, ``emit_ms`` and
        ``order_ms`` (HIP events; the last two are 0 without the list)."""
        c = (c_u64 * 6)()
        ms = (ctypes.c_double * 3)()
        check(lib.sw_amplicons_stats(self._h, c, ms))
        d = dict(zip(("items", "wave_items", "partners", "products", "detected", "launches"), (int(x) for x in c)))
        d.update(count_ms=ms[0], emit_ms=ms[1], order_ms=ms[2])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_amplicons_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LOCI_FIELDS = ("query", "assembly", "record", "strand", "band", "seeds", "dist", "end", "start", "nident", "mismatch", "gaps", "dup")


class Pileup:
    """Base counts per query position and group over the canonical alignments of a call's pairs, resident on the device
    (:meth:`Batch.infix_pileup`, ``Batch.best_hits(pileup=...)``; csrc/align.hip).  The last axis is
    PILE_CLASSES: the text bases ``A``, ``C``, ``G``, ``T`` facing the position (in the query's orientation), ``N`` for an invalid text
    base, ``DEL`` for a gap facing it; ``INS`` counts the insertions between positions u - 1 and u, ``INS_BASES`` their bases.  Exact
    integers; the first six add up to the depth at every position.  Not BLAST and not a multiple alignment."""

    def __init__(self, handle: c_vp, offsets: np.ndarray):
        self._h = handle
        self._offs = np.array(offsets, np.uint64)

    def sizes(self):
        """(queries, bases of all queries, groups)"""
        v = [c_u64() for _ in range(3)]
        check(lib.sw_pileup_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _rows(self, q0: int, q1: int) -> np.ndarray:
        ng = self.sizes()[2]
        out = np.empty((int(self._offs[q1] - self._offs[q0]), ng, len(PILE_CLASSES)), np.uint32)
        check(lib.sw_pileup_export(self._h, c_u64(q0), c_u64(q1), _ptr(out) if out.size else None))
        return out

    def counts(self, q: int) -> np.ndarray:
        """uint32[len(query q), groups, 8]"""
        q = int(q)
        if not 0 <= q < len(self._offs) - 1:
            raise ValueError(f"query {q} is none of the call's {len(self._offs) - 1}")
        return self._rows(q, q + 1)

    def table(self):
        """``(offsets, uint32[total, groups, 8])``: the rows of query q are ``[offsets[q], offsets[q + 1])``."""
        return self._offs.copy(), self._rows(0, len(self._offs) - 1)

    def depth(self) -> np.ndarray:
        """uint32[queries, groups]: the pairs of every query piled into every group."""
        nq, _, ng = self.sizes()
        out = np.empty((nq, ng), np.uint32)
        check(lib.sw_pileup_depth(self._h, _ptr(out) if out.size else None))
        return out

    def stats(self) -> dict:
        """The call's counters and ``pile_walk_ms``, the time of the walk that filled the table.  In a call with windows one walk
        fills both tables: ``pile_walk_ms`` is then that walk's time, the same figure as ``Windows.stats()["window_walk_ms"]``, and
        not what the pileup alone would have taken."""
        c = (c_u64 * 5)()
        ms = (ctypes.c_double * 1)()
        check(lib.sw_pileup_stats(self._h, c, ms))
        d = dict(zip(("piled", "filtered_by_distance", "left_out_by_label", "adds", "table_bytes"), (int(x) for x in c)))
        d.update(pile_walk_ms=ms[0])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_pileup_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Windows:
    """Joint mismatch classes per query window, window length and group over the canonical alignments of a call's piled pairs,
    resident on the device (:meth:`Batch.infix_windows`, ``Batch.best_hits(pileup=..., window_lengths=...)``; csrc/align.hip, DESIGN.md
    section 3.2l).  A row is a window's start in the query; rows whose window would pass the query's end stay 0.  The last axis is
    WINDOW_CLASSES: ``MM0`` .. ``MM3`` count the pairs whose copy faces the whole window without a gap and with exactly 0..3
    mismatches, ``MM4P`` with 4 or more, ``GAPPED`` with an indel inside the window -- these six add up to the pileup's depth;
    ``FWD_OK`` / ``REV_OK`` count the ungapped pairs with at most ``max_mismatch`` mismatches and none in the ``three_prime`` bases at
    the 3' end of the window itself / of its reverse complement as an oligo.  Exact integers.  Not BLAST, no Tm, no dG."""

    def __init__(self, handle: c_vp, offsets: np.ndarray):
        self._h = handle
        self._offs = np.array(offsets, np.uint64)

    def sizes(self):
        """(queries, bases of all queries, groups, lengths, max_mismatch, three_prime)"""
        v = [c_u64() for _ in range(6)]
        check(lib.sw_windows_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @property
    def lengths(self) -> tuple:
        """The window lengths, in the order the call gave them: the table's second axis."""
        out = np.zeros(self.sizes()[3], np.uint32)
        check(lib.sw_windows_lengths(self._h, _ptr(out)))
        return tuple(int(x) for x in out)

    def _rows(self, q0: int, q1: int) -> np.ndarray:
        _, _, ng, nl, _, _ = self.sizes()
        out = np.empty((int(self._offs[q1] - self._offs[q0]), nl, ng, len(WINDOW_CLASSES)), np.uint32)
        check(lib.sw_windows_export(self._h, c_u64(q0), c_u64(q1), _ptr(out) if out.size else None))
        return out

    def counts(self, q: int) -> np.ndarray:
        """uint32[len(query q), lengths, groups, 8]"""
        q = int(q)
        if not 0 <= q < len(self._offs) - 1:
            raise ValueError(f"query {q} is none of the call's {len(self._offs) - 1}")
        return self._rows(q, q + 1)

    def table(self):
        """``(offsets, uint32[total, lengths, groups, 8])``: the rows of query q are ``[offsets[q], offsets[q + 1])``."""
        return self._offs.copy(), self._rows(0, len(self._offs) - 1)

    def stats(self) -> dict:
        """Windows visited, adds issued, table bytes; ``window_walk_ms`` is the one walk that fills this table and the pileup's,
        ``finish_ms`` the finishing pass."""
        c = (c_u64 * 3)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_windows_stats(self._h, c, ms))
        d = dict(zip(("windows", "adds", "table_bytes"), (int(x) for x in c)))
        d.update(window_walk_ms=ms[0], finish_ms=ms[1])
        return d

    def close(self) -> None:
        if self._h:
            lib.sw_windows_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BestHits:
    """The best hit of every query in every assembly of a batch, resident on the device (:meth:`Batch.best_hits`,
    :meth:`Markers.best_hits`; csrc/hits.hip): per (query, assembly) the winning locus' vote ``seeds``, its
    global ``record`` and ``strand``, and the infix edit distance ``dist`` of the query to the best substring of the locus' window,
    which ends at record position ``end``.  A pair without a hit reads seeds 0, strand 0 and NO_HIT elsewhere.  It covers the ground
    of ``eval_markers`` (src/seqwin/markers.py:607-696), has no counterpart in the reference, is not BLAST and fills none of
    ``MarkerMetrics``.  A single-device object on a resident batch.  ``rows`` (queries) / ``cols`` (assemblies) are None (all), a
    ``(lo, hi)`` pair, a slice or a range.  Made with ``align=True`` it also holds the canonical alignment of every hit (csrc/align.hip,
    DESIGN.md section 3.2f): ``start``, ``nident``, ``mismatch`` and ``gaps``, NO_HIT where there is no hit.  Made with ``loci=True`` it
    also holds every seeded locus of every pair: the list ``loci()`` and, per pair, ``n_loci`` and
    ``sum_nident`` over the loci that are no duplicates -- counts, 0 where there is none.  Made with ``local=True`` it also holds the
    optimal local alignment of every hit on its window under an affine scoring system (csrc/local.hip; still
    not BLAST): ``score``, ``qstart``, ``qend``, ``sstart``, ``send``, ``local_nident``, ``local_mismatch``, ``local_gapopen`` and
    ``local_gaps``, NO_HIT where there is no hit.  Made with ``pileup=groups`` it also holds the :class:`Pileup` of the winners'
    canonical alignments by group of assembly: ``pileup()``; made with ``window_lengths`` too, the
    :class:`Windows` of the same winners: ``windows()``."""

    def __init__(self, handle: c_vp, aligned: bool = False, loci: bool = False, local: bool = False, pileup: "Pileup | None" = None,
                 windows: "Windows | None" = None):
        self._h = handle
        self._aligned = aligned
        self._loci = loci
        self._local = local
        self._pileup = pileup
        self._windows = windows

    def windows(self) -> "Windows":
        """The :class:`Windows` of the winners; it is closed with these hits."""
        if self._windows is None:
            raise ValueError("these best hits were made without window_lengths")
        return self._windows

    def pileup(self) -> "Pileup":
        """The :class:`Pileup` of the winners; it is closed with these hits."""
        if self._pileup is None:
            raise ValueError("these best hits were made without pileup=groups")
        return self._pileup

    def sizes(self):
        """(queries, assemblies, seeds of all queries, k)"""
        v = [c_u64() for _ in range(4)]
        check(lib.sw_hits_sizes(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def n_seeds(self) -> np.ndarray:
        """uint32[queries]: the canonical k-mers of every query that no other window of the query text has."""
        out = np.empty(self.sizes()[0], np.uint32)
        check(lib.sw_hits_n_seeds(self._h, _ptr(out)))
        return out

    def _block(self, field: int, rows, cols) -> np.ndarray:
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_hits_block, self._h, field, nq, na, rows, cols)

    def seeds(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the winner's vote (hits of its band and the next); 0: no hit."""
        return self._block(0, rows, cols)

    def record(self, rows=None, cols=None) -> np.ndarray:
        return self._block(1, rows, cols)

    def strand(self, rows=None, cols=None) -> np.ndarray:
        return self._block(2, rows, cols).astype(np.uint8)

    def end(self, rows=None, cols=None) -> np.ndarray:
        return self._block(3, rows, cols)

    def dist(self, rows=None, cols=None) -> np.ndarray:
        return self._block(4, rows, cols)

    def _align_block(self, field: int, rows, cols) -> np.ndarray:
        if not self._aligned:
            raise ValueError("these best hits were made without align=True")
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_hits_align_block, self._h, field, nq, na, rows, cols)

    def start(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: where the located copy starts in its record; it is ``[start, end)``."""
        return self._align_block(0, rows, cols)

    def nident(self, rows=None, cols=None) -> np.ndarray:
        return self._align_block(1, rows, cols)

    def mismatch(self, rows=None, cols=None) -> np.ndarray:
        return self._align_block(2, rows, cols)

    def gaps(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: gap columns of either side; ``mismatch + gaps == dist``."""
        return self._align_block(3, rows, cols)

    def intervals(self, rows=None, cols=None):
        """``(intervals, row, col)`` of the block's pairs WITH a hit, row-major: INTERVAL_DTYPE ``(record, start, end)`` as
        :meth:`Batch.fetch` takes them (the text of a strand-1 hit is the reverse complement of the query's copy), and the query
        and assembly index of each."""
        rec, a, e = self.record(rows, cols), self.start(rows, cols), self.end(rows, cols)
        nq, na, _, _ = self.sizes()
        r0, c0 = _block_range(rows, nq)[0], _block_range(cols, na)[0]
        r, c = np.nonzero(rec != np.uint32(NO_HIT))
        iv = np.empty(len(r), INTERVAL_DTYPE)
        iv["record"], iv["start"], iv["stop"] = rec[r, c], a[r, c], e[r, c]
        return iv, r + r0, c + c0

    def align_stats(self) -> dict:
        if not self._aligned:
            raise ValueError("these best hits were made without align=True")
        c = (c_u64 * 8)()
        ms = (ctypes.c_double * 2)()
        check(lib.sw_hits_align_stats(self._h, c, ms))
        d = dict(zip(_ALIGN_COUNTERS, (int(x) for x in c)))
        d.update(store_ms=ms[0], walk_ms=ms[1])
        return d

    def _local_block(self, field: int, rows, cols) -> np.ndarray:
        if not self._local:
            raise ValueError("these best hits were made without local=True")
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_hits_local_block, self._h, field, nq, na, rows, cols)

    def score(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the raw score of the winner's optimal local alignment on its window (0: nothing matches)."""
        return self._local_block(0, rows, cols)

    def qstart(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the local alignment covers ``[qstart, qend)`` of the query, in the hit's orientation."""
        return self._local_block(1, rows, cols)

    def qend(self, rows=None, cols=None) -> np.ndarray:
        return self._local_block(2, rows, cols)

    def sstart(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the local alignment covers ``[sstart, send)`` of the hit's record."""
        return self._local_block(3, rows, cols)

    def send(self, rows=None, cols=None) -> np.ndarray:
        return self._local_block(4, rows, cols)

    def local_nident(self, rows=None, cols=None) -> np.ndarray:
        return self._local_block(5, rows, cols)

    def local_mismatch(self, rows=None, cols=None) -> np.ndarray:
        return self._local_block(6, rows, cols)

    def local_gapopen(self, rows=None, cols=None) -> np.ndarray:
        return self._local_block(7, rows, cols)

    def local_gaps(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: gap columns of either side of the local alignment."""
        return self._local_block(8, rows, cols)

    def local_stats(self) -> dict:
        """The local stage's counters, winners and loci together: ``pairs``, ``cells`` (sum of m * n), ``striped_pairs`` (more than
        one pass over the text), ``hbm_carry_pairs``, ``launches``, ``pass_rows`` and ``local_ms``."""
        if not self._local:
            raise ValueError("these best hits were made without local=True")
        c = (c_u64 * 6)()
        ms = (ctypes.c_double * 1)()
        check(lib.sw_hits_local_stats(self._h, c, ms))
        return dict(zip(_LOCAL_COUNTERS, (int(x) for x in c)), local_ms=ms[0])

    def _loci_block(self, field: int, rows, cols) -> np.ndarray:
        if not self._loci:
            raise ValueError("these best hits were made without loci=True")
        nq, na, _, _ = self.sizes()
        return _cell_block(lib.sw_hits_loci_block, self._h, field, nq, na, rows, cols)

    def n_loci(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the pair's loci with ``min_seeds`` or more seeds, duplicates counted once; 0: none."""
        return self._loci_block(0, rows, cols)

    def sum_nident(self, rows=None, cols=None) -> np.ndarray:
        """uint32[rows, cols]: the sum of ``nident`` over the loci ``n_loci`` counts."""
        return self._loci_block(1, rows, cols)

    def loci(self) -> dict:
        """The list of all loci, ascending by (query, record, strand, band), as parallel arrays: ``query``, ``assembly``, ``record``,
        ``strand``, ``band``, ``seeds``, ``dist``, ``end``, ``start``, ``nident``, ``mismatch``, ``gaps`` and ``dup`` (1: the locus
        before it is the same copy); ``cell_offsets`` (uint64[queries * assemblies + 1]) bounds the loci of every pair.  Made with
        ``local=True`` too: also ``local_score``, ``local_qstart``, ``local_qend``, ``local_sstart``, ``local_send``, ``local_nident``,
        ``local_mismatch``, ``local_gapopen`` and ``local_gaps`` of every locus."""
        if not self._loci:
            raise ValueError("these best hits were made without loci=True")
        nq, na, _, _ = self.sizes()
        n, nd = c_u64(), c_u64()
        check(lib.sw_hits_loci_sizes(self._h, ctypes.byref(n), ctypes.byref(nd)))
        offs = np.empty(nq * na + 1, np.uint64)
        cols = [np.empty(n.value, np.uint32) for _ in LOCI_FIELDS]
        check(lib.sw_hits_loci(self._h, _ptr(offs), *[_ptr(a) if n.value else None for a in cols]))
        out = {f: (a.astype(np.uint8) if f in ("strand", "dup") else a) for f, a in zip(LOCI_FIELDS, cols)}
        out["cell_offsets"] = offs
        if self._local:   # the local alignment of every locus on its window, in the list's order
            lc = [np.empty(n.value, np.uint32) for _ in LOCAL_FIELDS]
            check(lib.sw_hits_loci_local(self._h, *[_ptr(a) if n.value else None for a in lc]))
            out.update({"local_" + f: a for f, a in zip(LOCAL_FIELDS, lc)})
        return out

    def loci_intervals(self) -> np.ndarray:
        """INTERVAL_DTYPE ``(record, start, end)`` of every locus that is no duplicate, in the list's order, as :meth:`Batch.fetch`
        takes them."""
        L = self.loci()
        keep = L["dup"] == 0
        iv = np.empty(int(keep.sum()), INTERVAL_DTYPE)
        iv["record"], iv["start"], iv["stop"] = L["record"][keep], L["start"][keep], L["end"][keep]
        return iv

    def loci_stats(self) -> dict:
        if not self._loci:
            raise ValueError("these best hits were made without loci=True")
        c = (c_u64 * 5)()
        ms = (ctypes.c_double * 4)()
        check(lib.sw_hits_loci_stats(self._h, c, ms))
        d = dict(zip(("loci", "duplicates", "max_loci_per_cell", "pairs_aligned", "rounds"), (int(x) for x in c)))
        d.update(peaks_ms=ms[0], distance_ms=ms[1], traceback_ms=ms[2], order_ms=ms[3])
        return d

    def stats(self) -> dict:
        c = (c_u64 * 10)()
        ms = (ctypes.c_double * 4)()
        check(lib.sw_hits_stats(self._h, c, ms))
        d = dict(zip(("hits", "seeds", "chunks", "chunk_splits", "launches", "pairs_aligned", "striped_pairs", "distinct_kmers", "buffer_keys",
                      "buffer_doublings"), (int(x) for x in c)))
        per = (c_u64 * max(d["chunks"], 1))()
        check(lib.sw_hits_chunk_hits(self._h, per))
        d.update(query_ms=ms[0], probe_ms=ms[1], vote_ms=ms[2], distance_ms=ms[3], chunk_hits=[int(x) for x in per][:d["chunks"]])
        return d

    def seed_stats(self) -> dict:
        """What the seed rule kept and dropped: ``seed_copies`` (0: the default, unique-seed call, whose
        rule is the one at 1), ``seed_words`` and the ``seed_windows`` that own them, ``dropped_words`` with more windows than the
        cap and their ``dropped_windows``, ``palindromic_words`` (their own reverse complement: never a seed, not counted as
        dropped), ``longest_owner_list`` and ``hits`` appended over all chunks."""
        c = (c_u64 * 8)()
        check(lib.sw_hits_seed_stats(self._h, c))
        return dict(zip(("seed_copies", "seed_words", "seed_windows", "dropped_words", "dropped_windows", "palindromic_words", "longest_owner_list",
                         "hits"), (int(x) for x in c)))

    def close(self) -> None:
        if self._pileup is not None:
            self._pileup.close()
        if self._windows is not None:
            self._windows.close()
        if self._h:
            lib.sw_hits_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _reorder(offs: np.ndarray, hashes: np.ndarray, order: np.ndarray):
    """CSR (offs, hashes) with its rows taken in ``order``."""
    o = offs.astype(np.int64)
    lens = np.diff(o)[order]
    new_offs = np.zeros(len(order) + 1, np.uint64)
    np.cumsum(lens, out=new_offs[1:])
    if len(hashes) == 0:
        return new_offs, hashes
    starts = o[:-1][order]
    idx = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
    return new_offs, hashes[idx]


_G = np.uint64(0x9E3779B97F4A7C15)


def _mix64(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    x ^= x >> np.uint64(30); x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27); x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
    return x


CHECKSUM_SCHEME = 2   # r06: every field carries the element index (1: kmers, nodes.hash and edges.first only)
_K1, _K2, _K3, _K4 = (np.uint64(0xA0761D6478BD642F), np.uint64(0xE7037ED1A0B428DB), np.uint64(0x8EBC6AF09C88C6E3),
                      np.uint64(0x589965CC75374CC3))


def host_checksums(kmers, nodes, edges, kmer_base: int = 0, node_base: int = 0, edge_base: int = 0):
    """numpy restatement of sw_index_checksums / sw_index_checksums_at (csrc/device.hpp: ck_kmer / ck_node / ck_edge) for host
    arrays.  Every field of an element is mixed with the element's index (r06): kmers; nodes' hash, start, stop, (n_tar, n_neg) and
    the penalty's bit pattern; edges' first, second, weight -- whole rows, as tests/smoke/test_graph.py:281-291 compares them."""
    with np.errstate(over="ignore"):
        x = (np.arange(len(kmers), dtype=np.uint64) + np.uint64(kmer_base)) * _G
        a = _mix64(x + (kmers["pos"].astype(np.uint64) | (kmers["record_idx"].astype(np.uint64) << np.uint64(32)))).sum(dtype=np.uint64)
        x = (np.arange(len(nodes), dtype=np.uint64) + np.uint64(node_base)) * _G
        b = (_mix64(x + nodes["hash"]) + _mix64((x ^ _K1) + nodes["start"].astype(np.uint64)) +
             _mix64((x ^ _K2) + nodes["stop"].astype(np.uint64)) +
             _mix64((x ^ _K3) + ((nodes["n_tar"].astype(np.uint64) << np.uint64(32)) | nodes["n_neg"].astype(np.uint64))) +
             _mix64((x ^ _K4) + np.ascontiguousarray(nodes["penalty"]).view(np.uint64))).sum(dtype=np.uint64)
        x = (np.arange(len(edges), dtype=np.uint64) + np.uint64(edge_base)) * _G
        c = (_mix64(x + edges["first"]) + _mix64((x ^ _K1) + edges["second"].astype(np.uint64)) +
             _mix64((x ^ _K2) + edges["weight"].astype(np.uint64))).sum(dtype=np.uint64)
    return int(a), int(b), int(c)
