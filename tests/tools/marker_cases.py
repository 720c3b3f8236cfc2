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


# ---- the bounds of csrc/markers.hip (tests/test_markers_bounds_cpu.py pins them against the source) --------------------------
LOC_CAP, VOTE_CAP, WAVE, TPB = 384, 1536, 64, 256
U32 = 1 << 32


def run_positions(lens, step=3, gap=100):
    pos, p = [], 0
    for ln in lens:
        pos += [p + i * step for i in range(ln)]
        p = pos[-1] + gap
    return pos


def runs(name, lens, **kw):
    """One subgraph, two target assemblies: runs of ``lens`` items (run_positions), distinct labels in position order in
    assembly 0 and the same layout with the labels reversed in assembly 1."""
    n, pos = sum(lens), run_positions(lens)
    items = [(i, 0, q) for i, q in enumerate(pos)] + [(n - 1 - i, 1, q) for i, q in enumerate(pos)]
    return build(name, [items], [0, 1, 2], 2, **kw)


def run_starts(lens):
    return [int(x) for x in np.cumsum([0] + list(lens[:-1]))]


# name -> the lengths of the runs of both assemblies (chunks of k_loc's run cut are 64 items)
RUN_LAYOUTS = {
    "run_starts_at_64": [64, 70],                          # the largest run starts on the chunk edge and carries into items 128..133
    "run_ends_at_63": [10, 54, 30],                        # the largest run ends in the last lane of the first chunk
    "run_spans_60_70": [10, 10, 10, 10, 10, 10, 11, 9],    # the largest run is items 60..70: seven of them need the carry
    "tie_first_chunk_wins": [4, 40, 20, 40, 10],           # 4..43 and 64..103: candidates of two lanes (43 and 39), equal length
    "later_larger_run_wins": [4, 40, 20, 41, 10],
    "run_over_three_chunks": [5, 150, 7],                  # 5..154: the carry crosses two chunk edges
}


def nodes_case(n):
    """n nodes, each once per assembly, in a different seeded order in each of three assemblies (two targets)."""
    rng = np.random.default_rng(n)
    items = []
    for a in range(3):
        items += at([int(x) for x in rng.permutation(n)], a, 0, 3)
    return build(f"nodes_{n}", [items], [0, 1, 2, 3], 2)


RAGGED_HEAVY, RAGGED_ABSENT = 50, tuple(range(3, 130, 7))


def nodes_ragged():
    """130 nodes.  Assembly 0: the 19 nodes of RAGGED_ABSENT have no occurrence, node RAGGED_HEAVY has 100 (one lane writes 100
    items), the other 110 one each; all 210 items are ONE run, so the duplicate lies in assembly 0's row.  Assembly 1 holds every
    node once (130 items).  210 x 1 beats 130 x 1: the representative is assembly 0's row and FLAG_DUP is set."""
    items = [(i, 0, 3 * i) for i in range(130) if i not in RAGGED_ABSENT and i != RAGGED_HEAVY]
    items += [(RAGGED_HEAVY, 0, 390 + 3 * i) for i in range(100)]
    items += at(list(range(130)), 1, 0, 3)
    return build("nodes_130_ragged", [items], [0, 1, 2], 2)


def pair_sizes(name, sizes):
    """One subgraph per size: n labels forward in assembly 0, reversed in assembly 1."""
    sgs = [at(list(range(n)), 0, 10000 * s, 3) + at(list(range(n))[::-1], 1, 10000 * s, 3) for s, n in enumerate(sizes)]
    return build(name, sgs, [0, 1, 2], 2)


POOL = ([0, 1, 2, 3], [3, 2, 1, 0], [0, 1, 2], [0, 1, 2, 3, 4])   # forward, reverse, a truncation, a longer one


def pool_orders(T, seed, pool=POOL):
    return [pool[int(i)] for i in np.random.default_rng(seed).integers(0, len(pool), T)]


def distinct_orders(n, labels, seed):
    """n different orderings of ``labels``, none the reverse of another (first label < last label), in a seeded order."""
    from itertools import permutations
    perms = [list(p) for p in permutations(labels) if p[0] < p[-1]]
    pick = np.random.default_rng(seed).permutation(len(perms))[:n]
    assert len(pick) == n
    return [perms[int(i)] for i in pick]


TIE_LONG, TIE_SHORT = [0, 1, 2, 3, 4, 5], [6, 7, 8, 9]   # 6 x 2 rows against 4 x 3 rows: both score 12
FILL = [10, 11, 12, 13, 14, 15, 16]                       # fillers: distinct orderings of seven other labels, score 7 each


def placed(name, T, places, n_tar=None, extra=()):
    """T target rows of distinct fillers with the orderings of ``places`` ({row: ordering}) put over them; ``extra``: more
    assemblies after them."""
    orders = distinct_orders(T, FILL, T)
    for row, o in places.items():
        orders[row] = o
    return vote(name, orders + list(extra), T if n_tar is None else n_tar)


PARTNER = [0, 1, 2, 3, 4, 5]
PALINDROMES = ([0, 1, 0], [1, 0, 1], [0, 1, 2, 1, 0], [2, 2], [0, 1, 2], [2, 1, 0])


def two_votes_mixed():
    """Three subgraphs over 1 600 single-record target assemblies with 1 600, 4 and 1 540 target rows."""
    pool = ([0, 1, 2], [2, 1, 0], [0, 1], [0, 1, 2, 3])
    sgs = []
    for s, T in enumerate((1600, 4, 1540)):
        items = []
        for a, o in enumerate(pool_orders(T, 100 + s, pool)):
            items += at(o, a, 1000 * s)
        sgs.append(items)
    return build("two_votes_mixed", sgs, list(range(1601)), 1600)


def without_occurrences(case, node):
    """``case`` with the occurrences of node ``node`` (its rank in the nodes) removed: start == stop."""
    nodes, kmers = case["nodes"].copy(), case["kmers"]
    a, b = int(nodes["start"][node]), int(nodes["stop"][node])
    nodes["stop"][node] = a
    nodes["start"][node + 1:] -= b - a
    nodes["stop"][node + 1:] -= b - a
    return dict(case, nodes=nodes, kmers=np.concatenate([kmers[:a], kmers[b:]]))


def pair_counts(case):
    """int64[n_sg, n_asm]: the items of every (subgraph, assembly) pair, counted from the arrays."""
    ro = np.asarray(case["record_offsets"], np.int64)
    so = np.asarray(case["sg_offsets"], np.int64)
    out = np.zeros((len(so) - 1, len(ro) - 1), np.int64)
    for s in range(len(so) - 1):
        for nd in case["nodes"][np.asarray(case["sg_nodes"][so[s]:so[s + 1]], np.int64)]:
            rec = case["kmers"]["record_idx"][int(nd["start"]):int(nd["stop"])].astype(np.int64)
            np.add.at(out[s], np.searchsorted(ro, rec, side="right") - 1, 1)
    return out


def bounds():
    """Inputs at the sizes where k_loc and k_vote change behaviour, each named for the branch it is built to reach."""
    out = [runs(f"pair_n{n}", [n]) for n in (63, 64, 65, 127, 128, 129, 383, 384, 385, 1000)]
    out += [runs(name, lens) for name, lens in RUN_LAYOUTS.items()]
    out.append(runs("many_runs", [1] * 200))
    out += [nodes_case(n) for n in (63, 64, 65, 130)]
    out.append(nodes_ragged())
    out.append(pair_sizes("three_subgraphs_mixed", (400, 5, 390)))
    # the vote
    out += [vote(f"vote_T{T}", pool_orders(T, T), T) for T in (255, 256, 257, 513, 1536, 1537)]
    out.append(vote("vote_all_equal_1537", [[0, 1, 2]] * 1537, 1537))
    out.append(vote("vote_all_distinct_600", distinct_orders(600, list(range(7)), 600), 600))
    out.append(placed("vote_tie_same_thread", 262, {3: TIE_LONG, 100: TIE_LONG, 259: TIE_SHORT, 260: TIE_SHORT, 261: TIE_SHORT}))
    out.append(placed("vote_tie_across_threads", 302, {300: TIE_LONG, 301: TIE_LONG, 5: TIE_SHORT, 6: TIE_SHORT, 7: TIE_SHORT}))
    P, Q = PARTNER, PARTNER[::-1]
    canon, other = sorted([P, Q], key=lambda o: tuple(map(H, o)))
    out.append(placed("vote_partner_far", 402, {2: P, 3: P, 400: Q}))
    out.append(placed("vote_partner_far_reverse_more_common", 402, {2: P, 400: Q, 401: Q}))
    out.append(placed("vote_partner_far_tie", 402, {2: canon, 400: other}))
    out.append(placed("vote_partner_far_tie_other_first", 402, {2: other, 400: canon}))
    out.append(vote("vote_palindromes_300", pool_orders(300, 300, PALINDROMES), 300))
    # 780 x [0, 1, 2] against 757 x [3, 4, 5] among the targets; the 50 non-targets would lift the second to 807
    xy = [[0, 1, 2]] * 780 + [[3, 4, 5]] * 757
    xy = [xy[int(i)] for i in np.random.default_rng(1537).permutation(1537)]
    out.append(vote("vote_non_targets_after_1537", xy + [[3, 4, 5]] * 50, 1537))
    out.append(two_votes_mixed())
    # 32-bit edges
    near = [(0, 0, U32 - 13), (1, 0, U32 - 8), (2, 0, U32 - 3)]
    out.append(build("stop_wraps", [near], [0, 1], 1, kmerlen=5))
    out.append(build("stop_wraps_kmerlen_2p32", [near], [0, 1], 1, kmerlen=U32 + 5))
    ends = [(0, 0, 0), (1, 0, U32 - 1)]
    out.append(build("cut_at_u32_max_one_run", [ends], [0, 1], 1, windowsize=2863311530))   # 3 w == 2 * (2^32 - 1)
    out.append(build("cut_at_u32_max_two_runs", [ends], [0, 1], 1, windowsize=2863311529))
    out.append(build("w_at_saturation", [ends], [0, 1], 1, windowsize=1 << 34))
    out.append(build("w_above_saturation", [ends], [0, 1], 1, windowsize=(1 << 34) + 1))
    hi = [(0, 0, 7), (1, 0, 12), (0, 1 << 31, 12), (1, 1 << 31, 17), (0, U32 - 2, 17), (1, U32 - 2, 22)]
    out.append(build("high_records", [hi], [0, 1, 1 << 31, (1 << 31) + 1, U32 - 1], 4))
    # empty shapes
    some = build("no_subgraphs", [at([0, 1, 2], 0) + at([2, 1, 0], 1)], [0, 1, 2], 2)
    out.append(dict(some, sg_offsets=np.zeros(1, np.uint64), sg_nodes=np.zeros(0, np.uint64)))
    nodes = np.zeros(3, NODE_DTYPE)
    nodes["hash"] = sorted(H(i) for i in range(3))
    out.append(dict(name="no_occurrences", kmers=np.zeros(0, KMER_DTYPE), nodes=nodes, sg_offsets=np.zeros(1, np.uint64),
                    sg_nodes=np.zeros(0, np.uint64), record_offsets=np.array([0, 1], np.uint32), n_tar=1, kmerlen=5, windowsize=10))
    out.append(without_occurrences(build("node_without_occurrences", [at([0, 1, 2], 0) + at([2, 1, 0], 1)], [0, 1, 2], 2), 1))
    assert len({c["name"] for c in out}) == len(out)
    return out


# The seeds of the sweep: 1 .. 43 without 6, 18 and 39, whose draws leave a subgraph without an item in any target assembly.
SWEEP_SEEDS = tuple(x for x in range(1, 44) if x not in (6, 18, 39))


def sweep(seed):
    """A small kept index drawn from ``seed``: 1-4 subgraphs of 1-150 nodes over 1-300 assemblies of 1-3 records; every subgraph
    has copies of its ordering -- forward, reversed, truncated or repeated -- in some of the assemblies, with steps around 1.5 w so
    that runs are cut at random.  About 1 500 occurrences per subgraph at the most."""
    rng = np.random.default_rng(seed)
    n_sg, n_asm, w = int(rng.integers(1, 5)), int(rng.integers(1, 301)), int(rng.integers(2, 30))
    ro = np.concatenate([[0], np.cumsum(rng.integers(1, 4, n_asm))])
    sgs = []
    for s in range(n_sg):
        m = int(rng.integers(1, 151))
        base = [int(x) for x in rng.permutation(m)]
        p = min(1.0, 1500 / (n_asm * m))
        items = []
        for a in range(n_asm):
            if rng.random() >= p:
                continue
            for copy in range(int(rng.integers(1, 3))):
                kind = int(rng.integers(0, 4))
                o = base
                if kind == 1:
                    o = base[::-1]
                elif kind == 2:
                    i = int(rng.integers(0, m))
                    o = base[i:int(rng.integers(i, m)) + 1]
                elif kind == 3 and m <= 40:
                    o = base + base
                rec = int(ro[a] + rng.integers(0, ro[a + 1] - ro[a]))
                pos = (4 * s + copy) * 200000 + int(rng.integers(0, 1000))
                for lab in o:
                    items.append((lab, rec, pos))
                    pos += int(rng.integers(w, 2 * w + 1))
        sgs.append(items)
    return build(f"sweep{seed}", sgs, ro, int(rng.integers(1, n_asm + 1)), kmerlen=int(rng.integers(5, 32)), windowsize=w)


def no_target_case():
    return vote("non_targets_only", [None, [0, 1, 2], [0, 1, 2]], 1)
