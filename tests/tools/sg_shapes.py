"""Adversarial graphs for the subgraph walk (csrc/subgraph.hip) and a second host restatement with selectable arithmetic.

make(family, params, seed) returns the (nodes, edges) arrays (NODE_DTYPE / EDGE_DTYPE, nodes strictly ascending by hash, every
edge weight >= 1, so the reference's _filter_edges_and_nodes(nodes, edges, 0) only drops the nodes without an edge).  It is
deterministic and uses numpy's default_rng(seed) through integers / random / permutation only; digest() pins its output
(tests/golden/subgraphs/shapes.json).  Families, and the part of the kernel each one aims at:
  star         one seed (the hub, penalty 0) and `deg` leaves with penalties in (th, 2 th]: the LDS frontier bound SG_FCAP = 1024;
               `deg2` > 0 gives the leaf accepted first `deg2` neighbours of its own, so its batch crosses the bound mid-batch
  long         paths, ladders and cliques of 127..130 low-penalty nodes: the LDS subgraph bound SG_SCAP = 128
  many_seeds   `n` disjoint triangles with one seed each and no conflicts: the adaptive window grows to SG_BMAX = 4096
  dense        a preferential-attachment graph with overlapping expansions: invalidation
  multi_spill  hubs of degree `deg` among ordinary seeds that reach into them: several spills in one walk
  ties         penalties in {-0.0, +0.0, 0.05, 0.1, 0.25} (the zeros alternate by hash), hashes over the full 64-bit range
  rounding     paths whose last acceptance is decided within a few ulps of penalty_th, each one decided differently by at least
               one wrong arithmetic (WRONG)
  rounding_edge  thresholds equal to a penalty, penalty_th 0.0 with +-0.0 seeds, subnormal penalties, a negative threshold
  dropin       edges in both orientations, repeated edges, self-loops and nodes without an edge
"""
from __future__ import annotations

import hashlib
import heapq
from fractions import Fraction

import numpy as np

from seqwin_amd._core import EDGE_DTYPE, NODE_DTYPE

U64_MAX = (1 << 64) - 1


# ---- arithmetic of the acceptance test -------------------------------------------------------------------------------------
def _accept_exact(acc, p, th):
    """The reference: the sum in acceptance order, divided by the new size, <= th."""
    t = 0.0
    for x in acc:
        t += x
    return (t + p) / (len(acc) + 1) <= th


def _accept_recip(acc, p, th):
    """Wrong: a reciprocal multiply instead of the division."""
    t = 0.0
    for x in acc:
        t += x
    return (t + p) * (1.0 / (len(acc) + 1)) <= th


def _accept_sorted(acc, p, th):
    """Wrong: the sum in ascending order instead of acceptance order."""
    t = 0.0
    for x in sorted(acc + [p]):
        t += x
    return t / (len(acc) + 1) <= th


def _accept_fma(acc, p, th):
    """Wrong: the comparison as a contracted fma(-th, size, sum) <= 0 (one rounding of the exact sum - th * size)."""
    t = 0.0
    for x in acc:
        t += x
    t += p
    return float(Fraction(t) - Fraction(th) * (len(acc) + 1)) <= 0.0


ARITH = {"exact": _accept_exact, "recip": _accept_recip, "sorted": _accept_sorted, "fma": _accept_fma}
WRONG = ("recip", "sorted", "fma")


def walk_heap(nodes, edges, penalty_th, min_nodes, max_nodes, rng, arith="exact"):
    """Second restatement, written without the first restatement's shortcuts: a (penalty, hash) heap over Python floats and ints,
    the expansion goes on after a rejection (every frontier node is popped once), ties are broken by hash, and the acceptance test
    is ARITH[arith].  Returns (tuple of frozensets of int hashes in final order, frozenset of used hashes) or raises RuntimeError."""
    h = np.asarray(nodes["hash"], np.uint64).tolist()
    pen = dict(zip(h, np.asarray(nodes["penalty"], np.float64).tolist()))
    adj: dict[int, set] = {}
    for a, b in zip(np.asarray(edges["first"], np.uint64).tolist(), np.asarray(edges["second"], np.uint64).tolist()):
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    ok = ARITH[arith]
    seeds = [x for x in sorted(adj) if pen[x] <= penalty_th]
    rng.shuffle(seeds)
    used: set = set()
    out = []
    for s in seeds:
        if s in used:
            continue
        sg, acc = {s}, [pen[s]]
        heap, fset = [], set()
        for v in adj[s]:
            if v not in used and v not in sg:
                heapq.heappush(heap, (pen[v], v))
                fset.add(v)
        while heap and (max_nodes is None or len(sg) < max_nodes):
            p, v = heapq.heappop(heap)
            if ok(acc, p, penalty_th):
                sg.add(v)
                acc.append(p)
                for x in adj[v]:
                    if x not in used and x not in sg and x not in fset:
                        heapq.heappush(heap, (pen[x], x))
                        fset.add(x)
            fset.discard(v)
        if len(sg) >= min_nodes:
            out.append(sg)
            used |= sg
    if not out:
        raise RuntimeError("No low-penalty subgraph was found.")
    rng.shuffle(out)
    return tuple(frozenset(s) for s in out), frozenset(used)


# ---- building blocks ---------------------------------------------------------------------------------------------------------
def _hashes(rng, n, special=()):
    """n distinct uint64 hashes, ascending, drawn over the full range; ``special`` values are included."""
    sp = np.asarray(special, np.uint64)
    h = np.unique(sp)
    while len(h) < n:
        h = np.unique(np.concatenate([h, rng.integers(0, U64_MAX, 2 * (n - len(h)) + 16, dtype=np.uint64, endpoint=True)]))
    if len(h) > n:   # keep the special values, drop random others
        keep = np.isin(h, sp)
        drop = rng.permutation(np.flatnonzero(~keep))[:len(h) - n]
        h = np.delete(h, drop)
    return h


def _assemble(pen, a, b, rng, special=(), orient="sorted", weight=None):
    """Arrays of a graph on structure nodes 0..n-1 (penalties ``pen``, edges a[i] -- b[i]): structure node i gets the hash of a
    random rank, so the walk's ties by hash do not follow the structure.  orient: 'sorted' (first < second) or 'as_is'."""
    n = len(pen)
    h = _hashes(rng, n, special)
    rank = rng.permutation(n)
    nodes = np.zeros(n, NODE_DTYPE)
    nodes["hash"] = h
    nodes["penalty"][rank] = pen
    a, b = rank[np.asarray(a, np.int64)], rank[np.asarray(b, np.int64)]
    if orient == "sorted":
        a, b = np.minimum(a, b), np.maximum(a, b)
    edges = np.zeros(len(a), EDGE_DTYPE)
    edges["first"] = h[a]
    edges["second"] = h[b]
    edges["weight"] = weight if weight is not None else 1 + rng.integers(0, 100, len(a))
    return nodes, edges


def _above(rng, n, th, hi=2.0):
    """n penalties in (th, hi * th]."""
    return th + (1.0 - rng.random(n)) * (hi - 1.0) * th


def _star(p, rng):
    th, deg, deg2 = p["th"], p["deg"], p.get("deg2", 0)
    n = 1 + deg + deg2
    pen = np.empty(n)
    pen[0] = 0.0
    pen[1:1 + deg] = _above(rng, deg, th)
    pen[1] = th * (1 + 1e-9)   # the least leaf: accepted first
    pen[1 + deg:] = 3.0 * th   # its own neighbours: frontier entries that are never accepted
    a = np.concatenate([np.zeros(deg, np.int64), np.ones(deg2, np.int64)])
    b = np.concatenate([np.arange(1, 1 + deg), np.arange(1 + deg, n)])
    return _assemble(pen, a, b, rng)


def _long(p, rng):
    th = p["th"]
    pens, A, B, base = [], [], [], 0
    for kind in ("path", "ladder", "clique"):
        for size in p["sizes"]:
            i = np.arange(size)
            if kind == "path":
                a, b = i[:-1], i[1:]
            elif kind == "ladder":   # rails 0 2 4 ... and 1 3 5 ..., rungs 2k -- 2k+1
                a = np.concatenate([i[:-2], i[:-1:2]])
                b = np.concatenate([i[2:], i[1::2]])
            else:
                a, b = np.triu_indices(size, 1)
            pens.append(rng.random(size) * 0.9 * th)   # all seeds, every mean stays below th: one expansion takes the component
            A.append(a + base)
            B.append(b + base)
            base += size
    return _assemble(np.concatenate(pens), np.concatenate(A), np.concatenate(B), rng)


def _many_seeds(p, rng):
    th, t = p["th"], p["n"]
    pen = _above(rng, 3 * t, th, 1.4)
    pen[0::3] = rng.random(t) * 0.5 * th   # one seed per triangle: no expansion meets another
    i = 3 * np.arange(t)
    a = np.concatenate([i, i, i + 1])
    b = np.concatenate([i + 1, i + 2, i + 2])
    return _assemble(pen, a, b, rng)


def _dense(p, rng):
    """Preferential attachment: every new node links to m targets drawn from the endpoint list (degree-proportional)."""
    n, m, th = p["n"], p["m"], p["th"]
    ends = np.empty(2 * m * n + 2, np.int64)
    ends[:2] = (0, 1)
    L = 2
    A, B = [0], [1]
    for v in range(2, n):
        t = ends[rng.integers(0, L, m)]
        A.extend([v] * m)
        B.extend(t.tolist())
        ends[L:L + m] = v
        ends[L + m:L + 2 * m] = t
        L += 2 * m
    a, b = np.asarray(A), np.asarray(B)
    pen = rng.random(n) * p["pmax"]
    return _assemble(pen, a, b, rng)


def _multi_spill(p, rng):
    th, hubs, deg, n_ord = p["th"], p["hubs"], p["deg"], p["ordinary"]
    n_hub = hubs * (1 + deg)
    n = n_hub + 3 * n_ord
    pen = np.empty(n)
    A, B = [], []
    for k in range(hubs):
        c = k * (1 + deg)
        pen[c] = 0.0
        pen[c + 1:c + 1 + deg] = _above(rng, deg, th)
        A.append(np.full(deg, c))
        B.append(np.arange(c + 1, c + 1 + deg))
    o = n_hub + 3 * np.arange(n_ord)   # ordinary triangles: a seed and two acceptable nodes
    pen[n_hub:] = _above(rng, 3 * n_ord, th, 1.4)
    pen[o] = rng.random(n_ord) * 0.5 * th
    A += [o, o, o + 1]
    B += [o + 1, o + 2, o + 2]
    # a quarter of the triangles touch a leaf of some hub: their expansions reach into the hubs and conflict with the hubs' own
    links = o[rng.permutation(n_ord)[:n_ord // 4]]
    hub_of = rng.integers(0, hubs, len(links))
    leaf = hub_of * (1 + deg) + 1 + rng.integers(0, deg, len(links))
    A.append(links)
    B.append(leaf)
    return _assemble(pen, np.concatenate(A), np.concatenate(B), rng)


TIE_VALUES = (0.05, 0.1, 0.25)


def _ties(p, rng):
    n, m = p["n"], p["m"]
    special = (0, U64_MAX, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, 1, U64_MAX - 1)
    nodes, edges = _assemble(np.zeros(n), rng.integers(0, n, m), rng.integers(0, n, m), rng, special)
    k = rng.integers(0, 5, n)   # 0, 1: a zero; 2..4: TIE_VALUES
    pen = np.asarray((0.0, 0.0) + TIE_VALUES)[k]
    z = np.flatnonzero(k < 2)
    pen[z[0::2]] = -0.0        # the zeros alternate -0.0, +0.0 in hash order
    nodes["penalty"] = pen
    keep = edges["first"] != edges["second"]
    return nodes, edges[keep]


def _rounding_path(rng, th, m, target):
    """Penalties of a path of m nodes (node 0 the only seed) whose last node is accepted or not within a few ulps of th, and
    decided differently by ARITH[target] (any wrong one if target is None); None if this draw is not sensitive."""
    a = rng.random() * 0.5
    pen = [a * th]
    budget = (1 - a) * th
    for _ in range(m - 2):
        pen.append(th + rng.random() * budget / m)
    t = 0.0
    for x in pen:
        t += x
    last = th * m - t
    for _ in range(abs(int(rng.integers(-4, 5)))):
        last = np.nextafter(last, np.inf if rng.integers(0, 2) else -np.inf)
    last = float(last)
    if not last > th:
        return None
    want = _accept_exact(pen, last, th)
    wrong = WRONG if target is None else (target,)
    if all(ARITH[w](pen, last, th) == want for w in wrong):
        return None
    return pen + [last]


def _rounding(p, rng):
    th, n_paths = p["th"], p["paths"]
    targets = p.get("targets", list(WRONG))
    pens, A, B, base = [], [], [], 0
    for k in range(n_paths):
        target = targets[k % len(targets)]
        for _ in range(200000):
            path = _rounding_path(rng, th, int(rng.integers(2, 9)), target)
            if path is not None:
                break
        else:
            raise RuntimeError(f"rounding: no path sensitive to {target} at th = {th!r}")
        pens += path
        m = len(path)
        A.append(np.arange(base, base + m - 1))
        B.append(np.arange(base + 1, base + m))
        base += m
    return _assemble(np.asarray(pens), np.concatenate(A), np.concatenate(B), rng)


def _rounding_edge(p, rng):
    """Small components: a seed whose penalty equals th, a pair whose mean equals th exactly, +-0.0 seeds and neighbours,
    subnormal penalties, and a seed at the threshold next to a node one ulp above it."""
    th = p["th"]
    up = float(np.nextafter(th, np.inf))
    comps = [[th, 0.5], [th, th], [0.0, -0.0, 0.0], [-0.0, th], [5e-324, 1e-323, 0.0], [2.5e-320, 7.5e-320, 1e-310],
             [th, up], [0.0, up, up], [th / 3, th / 3, th / 3, th]]
    pens, A, B, base = [], [], [], 0
    for c in comps:
        pens += c
        A.append(np.arange(base, base + len(c) - 1))
        B.append(np.arange(base + 1, base + len(c)))
        base += len(c)
    return _assemble(np.asarray(pens), np.concatenate(A), np.concatenate(B), rng)


def _dropin(p, rng):
    """A random graph given the way a caller might: both orientations, repeated edges, self-loops and nodes without an edge."""
    n, m, th = p["n"], p["m"], p["th"]
    pen = rng.random(n) * 2 * th
    a, b = rng.integers(0, n - n // 10, m), rng.integers(0, n - n // 10, m)   # the last tenth has no edge
    rep = rng.integers(0, m, m // 5)
    loops = rng.integers(0, n - n // 10, m // 20)
    flip = rng.integers(0, 2, m + len(rep)).astype(bool)
    a, b = np.concatenate([a, a[rep]]), np.concatenate([b, b[rep]])
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    a, b = np.concatenate([a, loops]), np.concatenate([b, loops])
    order = rng.permutation(len(a))
    return _assemble(pen, a[order], b[order], rng, orient="as_is")


FAMILIES = {"star": _star, "long": _long, "many_seeds": _many_seeds, "dense": _dense, "multi_spill": _multi_spill, "ties": _ties,
            "rounding": _rounding, "rounding_edge": _rounding_edge, "dropin": _dropin}


def make(family: str, params: dict, seed: int):
    return FAMILIES[family](params, np.random.default_rng(seed))


def digest(nodes, edges) -> str:
    """sha256 of the hash and penalty fields of the nodes and the three fields of the edges."""
    d = hashlib.sha256()
    for a in (nodes["hash"], nodes["penalty"], edges["first"], edges["second"], edges["weight"]):
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


def canonical_csr(subgraphs):
    """(offsets, hashes) of subgraphs in the given order, hashes ascending inside each: uint64 arrays."""
    lens = [len(s) for s in subgraphs]
    offs = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.uint64)
    hashes = np.array([x for s in subgraphs for x in sorted(int(y) for y in s)], np.uint64)
    return offs, hashes


def csr_digest(offsets, hashes) -> str:
    d = hashlib.sha256()
    d.update(np.asarray(offsets, np.uint64).tobytes())
    d.update(np.asarray(hashes, np.uint64).tobytes())
    return d.hexdigest()


# ---- the cases --------------------------------------------------------------------------------------------------------------
# (family, params, seed, [(penalty_th, min_nodes, max_nodes)]); rng seeds are assigned in order.
TH = 0.1
GRAPHS = [
    *[("star", dict(th=TH, deg=d), 100 + d, [(TH, 1, None), (TH, 3, 100)]) for d in (1023, 1024, 1025, 1087, 2048)],
    *[("star", dict(th=TH, deg=1000, deg2=d2), 200 + d2, [(TH, 1, None)]) for d2 in (25, 26, 40)],
    ("long", dict(th=TH, sizes=[127, 128, 129, 130]), 300, [(TH, 1, None), (TH, 1, 128), (TH, 1, 129), (TH, 1, 1000), (TH, 3, 100)]),
    ("many_seeds", dict(th=TH, n=100_000), 400, [(TH, 1, None), (TH, 3, 100)]),
    # (max_nodes bounded: with None one expansion takes 77 000 nodes through the one-wave spill path, round after round)
    ("dense", dict(th=TH, n=200_000, m=2, pmax=0.4), 500, [(TH, 1, 128), (TH, 3, 100)]),
    ("multi_spill", dict(th=TH, hubs=6, deg=1500, ordinary=3000), 600, [(TH, 1, None), (TH, 3, None)]),
    ("ties", dict(n=4000, m=10000), 700, [(0.0, 1, None), (-0.0, 1, 3), (0.05, 1, None), (0.05, 2, 2), (0.1, 1, 5), (0.1, 3, None),
                                          (0.25, 1, 3)]),
    *[("rounding", dict(th=th, paths=30), 800 + i, [(th, 1, None), (th, 2, None)])
      for i, th in enumerate((0.1, 0.2, 1 / 3, 0.0123456789, 0.7, 3.1e-5))],
    ("rounding", dict(th=4.4e-321, paths=12, targets=[None]), 810, [(4.4e-321, 1, None)]),
    ("rounding_edge", dict(th=TH), 900, [(TH, 1, None), (0.0, 1, None), (-0.0, 1, None), (1e-323, 1, None), (-0.5, 1, None),
                                          (float(np.nextafter(TH, -np.inf)), 1, None)]),
    ("dropin", dict(th=TH, n=600, m=1500), 1000, [(TH, 1, None), (TH, 3, 100), (0.2, 2, 10)]),
]


def graph_id(family, params, seed) -> str:
    extra = "_".join(f"{k}-{v}" for k, v in params.items() if k not in ("th", "sizes", "targets"))
    return f"{family}_{extra}_s{seed}" if extra else f"{family}_s{seed}"


def cases():
    """[(graph id, family, params, seed, [dict(penalty_th, min_nodes, max_nodes, seed)])]"""
    out, r = [], 0
    for family, params, seed, runs in GRAPHS:
        cs = []
        for th, mn, mx in runs:
            cs.append(dict(penalty_th=th, min_nodes=mn, max_nodes=mx, seed=r))
            r += 1
        out.append((graph_id(family, params, seed), family, params, seed, cs))
    return out


def load_golden(golden_dir, families=None, max_nodes=None):
    """tests/golden/subgraphs/shapes.json with the graphs regenerated: [(graph entry, nodes, edges, [(case, expected)])], expected
    the stored (offsets, hashes) of the case or None (error, or a large case: only its csr_sha256 is stored)."""
    import json
    from pathlib import Path
    d = Path(golden_dir) / "subgraphs"
    z = np.load(d / "shapes_cases.npz")
    out = []
    for g in json.loads((d / "shapes.json").read_text())["graphs"]:
        if (families is not None and g["family"] not in families) or (max_nodes is not None and g["n_nodes"] > max_nodes):
            continue
        nodes, edges = make(g["family"], g["params"], g["seed"])
        cases = []
        for c in g["cases"]:
            exp = None
            if c.get("stored"):
                exp = (z[c["stored"] + "__offsets"].astype(np.uint64), nodes["hash"][z[c["stored"] + "__ranks"].astype(np.int64)])
            cases.append((c, exp))
        out.append((g, nodes, edges, cases))
    return out
