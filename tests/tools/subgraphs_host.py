"""Host restatement of the low-penalty subgraph walk (Seqwin's kmers._get_subgraphs semantics) over a CSR adjacency.

Written independently of the reference, as the oracle of tests/test_gpu_subgraphs.py and tests/tools/subgraph_time.py; the goldens
under tests/golden/subgraphs/ (recorded from the reference itself) pin it.  Semantics:
  seeds = nodes of the graph (endpoints of an edge) with penalty <= penalty_th, ascending hash, then rng.shuffle;
  for every seed not yet used: grow {seed} by the least (penalty, hash) neighbour of the subgraph that is not used, while the
  running mean of the penalties (double sum in acceptance order, divided by the new size) stays <= penalty_th and the size is
  below max_nodes; keep it if it has >= min_nodes nodes (its nodes become used); nothing kept -> RuntimeError; rng.shuffle of
  the kept subgraphs.
rng.shuffle depends only on the length of the list, so both shuffles are done on index lists.
"""
from __future__ import annotations

import heapq

import numpy as np

NO_SUBGRAPH_MSG = ('No low-penalty subgraph was found. '
                   'Try decrease --stringency, or increase --penalty-th (penalty threshold, check log for the calculated value)')


def csr(node_hashes, first, second):
    """(off[n + 1], nbr, in_graph[n]) of the undirected graph on the ranks of ``node_hashes`` (sorted ascending).
    Self-loops put their node in the graph but are left out of the neighbour lists; repeated edges appear once."""
    h = np.asarray(node_hashes, np.uint64)
    first = np.asarray(first, np.uint64)
    second = np.asarray(second, np.uint64)
    n = len(h)
    ra = np.searchsorted(h, first)
    rb = np.searchsorted(h, second)
    if len(first) and (ra.max() >= n or rb.max() >= n or not (np.array_equal(h[ra], first) and np.array_equal(h[rb], second))):
        raise ValueError("an edge endpoint is not among the nodes")
    in_graph = np.zeros(n, bool)
    in_graph[ra] = True
    in_graph[rb] = True
    src = np.concatenate([ra, rb]).astype(np.int64)
    dst = np.concatenate([rb, ra]).astype(np.int64)
    keep = src != dst
    pairs = np.unique(src[keep] * max(n, 1) + dst[keep])
    src, dst = pairs // max(n, 1), pairs % max(n, 1)
    off = np.searchsorted(src, np.arange(n + 1))
    return off, dst, in_graph


def seeds(penalty, in_graph, penalty_th):
    return np.flatnonzero(in_graph & (np.asarray(penalty) <= penalty_th))


def walk(penalty, off, nbr, seed_ranks, penalty_th, min_nodes, max_nodes):
    """The walk over shuffled seed ranks: (list of subgraphs as rank lists in acceptance order, in commit order; used mask)."""
    pen = np.asarray(penalty, np.float64).tolist()
    offl = np.asarray(off).tolist()
    nbrl = np.asarray(nbr).tolist()
    used = bytearray(len(pen))
    out = []
    for s in np.asarray(seed_ranks).tolist():
        if used[s]:
            continue
        sg = [s]
        seen = {s}
        total = pen[s]
        heap = []

        def push(u):
            for v in nbrl[offl[u]:offl[u + 1]]:
                if not used[v] and v not in seen:
                    seen.add(v)
                    heapq.heappush(heap, (pen[v], v))

        push(s)
        while heap and (max_nodes is None or len(sg) < max_nodes):
            p, v = heapq.heappop(heap)
            t = total + p
            if not (t / (len(sg) + 1) <= penalty_th):
                break   # every later pop has a (penalty, hash) at least as large: rejected too
            sg.append(v)
            total = t
            push(v)
        if len(sg) >= min_nodes:
            out.append(sg)
            for v in sg:
                used[v] = 1
    return out, np.frombuffer(bytes(used), np.uint8).astype(bool)


def get_subgraphs(nodes, edges, penalty_th, min_nodes, max_nodes, rng):
    """Drop-in restatement on the filtered (nodes, edges) arrays: (tuple of frozensets of np.uint64, frozenset of np.uint64),
    leaving ``rng`` where the reference leaves it.  Also returns the subgraphs as rank lists in final order (third item)."""
    h = np.asarray(nodes["hash"], np.uint64)
    off, nbr, in_graph = csr(h, edges["first"], edges["second"])
    sd = seeds(nodes["penalty"], in_graph, penalty_th)
    perm = list(range(len(sd)))
    rng.shuffle(perm)
    sgs, used = walk(nodes["penalty"], off, nbr, sd[np.asarray(perm, np.int64)] if len(sd) else sd, penalty_th, min_nodes, max_nodes)
    if not sgs:
        raise RuntimeError(NO_SUBGRAPH_MSG)
    order = list(range(len(sgs)))
    rng.shuffle(order)
    sgs = [sgs[i] for i in order]
    return (tuple(frozenset(h[np.asarray(sg, np.int64)].tolist()) for sg in sgs), frozenset(h[used].tolist()),
            [sorted(sg) for sg in sgs])


def as_np_sets(subgraphs, used):
    """The reference's element type (np.uint64)."""
    return tuple(frozenset(np.uint64(x) for x in sg) for sg in subgraphs), frozenset(np.uint64(x) for x in used)


def induced_edges(edges, node_hashes, rank_subgraphs):
    """For every subgraph (rank lists), the rows of ``edges`` with both endpoints in it, in edge order."""
    h = np.asarray(node_hashes, np.uint64)
    sg_of = np.full(len(h), -1, np.int64)
    for i, sg in enumerate(rank_subgraphs):
        sg_of[np.asarray(sg, np.int64)] = i
    if len(edges) == 0:
        return [edges[:0] for _ in rank_subgraphs]
    a = sg_of[np.searchsorted(h, edges["first"])]
    b = sg_of[np.searchsorted(h, edges["second"])]
    hit = (a >= 0) & (a == b)
    return [edges[hit & (a == i)] for i in range(len(rank_subgraphs))]


def thresholds(nodes, n_tar: int, n_neg: int, stringency: int = 5, edge_w_th_mul: float = 0.3, cap: float = 0.2):
    """(penalty_th, edge_weight_th) from minimizer sketches, the way kmers.filter_graph computes them (kmers.py:426-453)."""
    nt = nodes["n_tar"]
    e_abs = 1 - np.sum((nt / n_tar) * nt) / np.sum(nt)
    e_pre = np.sum((nodes["n_neg"] / n_neg) * nt) / np.sum(nt)
    th = min(float((1 - stringency / 10) * (e_abs * e_pre) ** 0.5), cap)
    return th, edge_w_th_mul * (1 - th) * n_tar


def thresholds_from_sums(sums, n_tar: int, n_neg: int, stringency: int = 5, edge_w_th_mul: float = 0.3, cap: float = 0.2):
    """The same from Index.threshold_sums() = (sum n_tar, sum n_tar^2, sum n_tar * n_neg) (for graphs too large to export)."""
    s1, s2, s3 = (float(x) for x in sums)
    e_abs = 1 - s2 / n_tar / s1
    e_pre = s3 / n_neg / s1
    th = min(float((1 - stringency / 10) * (e_abs * e_pre) ** 0.5), cap)
    return th, edge_w_th_mul * (1 - th) * n_tar


def load_golden(golden_dir):
    """tests/golden/subgraphs: [(graph entry of the manifest, nodes, edges, [(case, expected (offsets, hashes) or None)])]."""
    import json
    from pathlib import Path

    from seqwin_amd._core import EDGE_DTYPE, NODE_DTYPE
    d = Path(golden_dir) / "subgraphs"
    out = []
    for g in json.loads((d / "manifest.json").read_text())["graphs"]:
        z = np.load(d / f"graph_{g['name']}.npz")
        h = z["hash"]
        nodes = np.zeros(len(h), NODE_DTYPE)
        nodes["hash"] = h
        nodes["penalty"] = z["penalty"]
        edges = np.zeros(len(z["first"]), EDGE_DTYPE)
        edges["first"] = h[z["first"].astype(np.int64)]
        edges["second"] = h[z["second"].astype(np.int64)]
        edges["weight"] = z["weight"]
        c = np.load(d / f"cases_{g['name']}.npz")
        cases = []
        for i, case in enumerate(g["cases"]):
            exp = None
            if case["error"] is None:
                exp = (c[f"c{i}_offsets"], h[c[f"c{i}_ranks"].astype(np.int64)])
            cases.append((case, exp))
        out.append((g, nodes, edges, cases))
    return out


def csr_to_sets(offsets, hashes):
    o = np.asarray(offsets).astype(np.int64).tolist()
    v = np.asarray(hashes, np.uint64).tolist()
    return tuple(frozenset(v[o[i]:o[i + 1]]) for i in range(len(o) - 1))
