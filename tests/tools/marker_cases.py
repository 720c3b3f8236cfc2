"""Crafted inputs for the marker step (csrc/markers.hip): the smallest kept indexes that reach each branch of the run cut, the
row choice and the representative vote.  A case is a dict of the direct route's arguments
(kmers, nodes, sg_offsets, sg_nodes, record_offsets, n_tar, kmerlen, windowsize) plus ``name``.

An input is described by its occurrences: a subgraph is a list of ``(label, global record, pos)`` with small integer labels;
label i becomes hash H(i), which spreads over the whole uint64 range (orderings compare as UNSIGNED hash values, not by label)."""
from __future__ import annotations

import numpy as np

KMER_DTYPE = np.dtype([("pos", "<u4"), ("record_idx", "<u4")])
NODE_DTYPE = np.dtype([("hash", "<u8"), ("start", "<u8"), ("stop", "<u8"), ("n_tar", "<u4"), ("n_neg", "<u4"), ("penalty", "<f8")])


def H(label: int) -> int:
    return ((label + 1) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def build(name, subgraphs, record_offsets, n_tar, kmerlen=5, windowsize=10):
    """subgraphs: list of lists of (label, global record, pos); labels are private to a subgraph."""
    occ = {}
    sg_hashes = []
    for s, items in enumerate(subgraphs):
        hs = set()
        for label, rec, pos in items:
            h = H(label + 1000 * s)
            occ.setdefault(h, []).append((rec, pos))
            hs.add(h)
        sg_hashes.append(sorted(hs))
    hashes = sorted(occ)
    nodes = np.zeros(len(hashes), NODE_DTYPE)
    kmers = []
    for i, h in enumerate(hashes):
        lst = sorted(occ[h])
        assert len(set(lst)) == len(lst)
        nodes[i]["hash"], nodes[i]["start"], nodes[i]["stop"] = h, len(kmers), len(kmers) + len(lst)
        kmers += lst
    allpos = [(rec, pos) for lst in occ.values() for rec, pos in lst]
    assert len(set(allpos)) == len(allpos), "one position has one minimizer"
    k = np.zeros(len(kmers), KMER_DTYPE)
    if kmers:
        k["record_idx"], k["pos"] = [r for r, _ in kmers], [p for _, p in kmers]
    rank = {h: i for i, h in enumerate(hashes)}
    return dict(name=name, kmers=k, nodes=nodes, sg_offsets=np.concatenate([[0], np.cumsum([len(x) for x in sg_hashes])]).astype(np.uint64),
                sg_nodes=np.array([rank[h] for hs in sg_hashes for h in hs], np.uint64), record_offsets=np.asarray(record_offsets, np.uint32),
                n_tar=n_tar, kmerlen=kmerlen, windowsize=windowsize)


def at(labels, rec, pos0=0, step=5):
    """The ordering ``labels`` laid out in record ``rec`` from ``pos0`` on, ``step`` apart."""
    return [(lab, rec, pos0 + i * step) for i, lab in enumerate(labels)]


def vote(name, orders, n_tar, **kw):
    """One subgraph, one single-record assembly per ordering (None: the assembly has no item)."""
    items = []
    for a, o in enumerate(orders):
        if o is not None:
            items += at(o, a)
    return build(name, [items], list(range(len(orders) + 1)), n_tar, **kw)


def gaps(name, w, diffs):
    pos, items = 0, [(0, 0, 0)]
    for i, d in enumerate(diffs):
        pos += d
        items.append((i + 1, 0, pos))
    return build(name, [items], [0, 1], 1, windowsize=w)


def many_assemblies(n_asm, seed):
    """Two subgraphs over n_asm assemblies of two records: forward, reversed, truncated and repeated copies, gaps in between."""
    rng = np.random.default_rng(seed)
    sgs = []
    for s in range(2):
        m = 4 + 3 * s
        items, used = [], set()
        for a in range(n_asm):
            if rng.random() < 0.15:
                continue
            for _ in range(int(rng.integers(1, 4))):
                o = list(range(m))
                kind = int(rng.integers(0, 5))
                if kind == 1:
                    o = o[::-1]
                elif kind == 2:
                    o = o[:-1]
                elif kind == 3:
                    o = o[::-1][: m - 2]
                rec = 2 * a + int(rng.integers(0, 2))
                p0 = int(rng.integers(0, 40)) * 100 + 50 * s
                if (rec, p0) in used:
                    continue
                used.add((rec, p0))
                items += at(o, rec, p0, int(rng.integers(1, 8)))
        sgs.append(items)
    return build(f"asm{n_asm}", sgs, list(range(0, 2 * n_asm + 1, 2)), n_asm // 2)


def cases():
    A, B, C = [0, 1, 2], [2, 1, 0], [0, 1, 3]
    canon, other = sorted([A, B], key=lambda o: tuple(map(H, o)))   # canonical: the smaller as unsigned hash values
    out = [
        # the cut: 2 * diff > 3 * w
        gaps("gap_even_w10", 10, [15, 16, 15]), gaps("gap_odd_w11", 11, [16, 17, 16]), gaps("gap_w1", 1, [1, 2, 1, 1]),
        gaps("gap_w_huge", 1 << 40, [1 << 31, 5]),
        # record changes with a smaller, equal and larger pos; the same local record index in two assemblies
        build("records", [at([0, 1], 0, 100) + at([2], 1, 50) + at([3], 2, 50) + at([4], 3, 60) + at([0, 1, 2], 5, 7) + at([0, 1], 7, 7)],
              [0, 4, 6, 8], 2),
        # two runs of equal size: the first; a later larger run wins; an assembly without an item; n_tar - 1 against n_tar
        build("repeats", [at([0, 1], 0, 0) + at([1, 0], 0, 500) + at([0], 1, 0) + at([0, 1, 2], 1, 400) + at([2], 1, 900) + at([0, 1, 2], 3, 0)
                          + at([2, 1, 0], 4, 9)], [0, 1, 2, 3, 4, 5], 4),
        build("all_targets", [at(A, 0) + at(B, 1) + at(A, 2)], [0, 1, 2, 3], 3),
        build("single_assembly", [at(A, 0) + at(A, 0, 1000)], [0, 1], 1),
        build("empty_assemblies_and_records", [at(A, 2) + at(A, 5)], [0, 0, 2, 3, 3, 6, 6], 5),
        many_assemblies(63, 1), many_assemblies(64, 2), many_assemblies(65, 3),
        # the vote
        vote("reverse_more_common", [other, other, canon], 3), vote("reverse_more_common_seen_last", [canon, other, other], 3),
        vote("orientations_tie", [B, A, A, B], 4), vote("orientations_tie_other_first", [A, B, B, A], 4),
        vote("two_canonicals_tie", [[0, 1, 2, 3], [4, 5], [4, 5], C], 3), vote("two_canonicals_tie_swapped", [[4, 5], [0, 1, 2, 3], [4, 5], C], 3),
        vote("long_rare_beats_short_common", [[0, 1, 2, 3, 4, 5, 6], [0, 1], [0, 1], [0, 1]], 4),
        vote("short_common_beats_long_rare", [[0, 1, 2, 3, 4, 5, 6], [0, 1], [0, 1], [0, 1], [0, 1]], 5),
        vote("palindrome", [[0, 1, 0], [0, 1, 0], A], 3),
        vote("dup", [[0, 1, 0, 2], [0, 1, 0, 2], A], 3),
        vote("single", [[0], [0], None, [0, 1]], 3),
        vote("last_element_differs", [A, C, C, A, C], 5),
        vote("rep_row_is_a_later_target", [B, C, A, A, None, A], 5),
        vote("non_targets_vote_nothing", [A, B, B, B], 1),
        # more than 8 items in a pair (the spill with the LDS bound lowered), in two runs and two records
        build("big_pair", [at(list(range(11)), 0, 0, 3) + at(list(range(11))[::-1], 1, 0, 3) + at([0, 1, 2], 2, 0)], [0, 2, 3], 2),
    ]
    out.append(build("two_subgraphs", [at(A, 0) + at(B, 1), at([0, 1, 2, 3], 0, 300) + at([0, 1, 2, 3], 1, 300) + at([0, 1], 2, 0)],
                     [0, 1, 2, 3], 2))
    return out


def no_target_case():
    return vote("non_targets_only", [None, [0, 1, 2], [0, 1, 2]], 1)
