#!/usr/bin/env python3
"""Time the subgraph walk (kmers._get_subgraphs) on the device against the host restatement, on synthetic bacteria15k genomes.

    python tests/tools/subgraph_time.py --genomes 2048 15000 [--target-ancestors 1 10] [--reps 3] [--json OUT]

Per (genomes, target ancestors): the batch of the bench's bacteria15k generator (50 records x 100 kbp per genome, 30 ancestors,
10 000 ppm SNPs), targets = the genomes of the first `a` ancestors (a target clade: the reference's edge-weight threshold keeps the
edges the clade shares), index k=21 w=200, thresholds as kmers.filter_graph computes them from minimizer sketches
(stringency 5, edge_w_th_mul 0.3, min_nodes 3, max_nodes 100; on this generator the computed penalty_th is ~0 -- the
ancestors share no k-mers, so no non-target holds a target k-mer -- and the walk has no seed: --penalty-th 0.2 is the run with work), filter_graph on the device.  The timed device call starts from the
resident filtered index and ends with the subgraph CSR on the host (Index.subgraphs + Subgraphs.csr); device ms from the library's
HIP events.  The host restatement (tests/tools/subgraphs_host.py: numpy CSR + heapq walk) runs on the exported arrays, and the
networkx graph construction the reference does first (kmers.py:164-170) is timed separately where networkx is installed.
Both results are compared.
"""
from __future__ import annotations

import argparse
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import subgraphs_host as H  # noqa: E402


def run_case(ix, G: int, ta: int, n_tar: int, given: float, a) -> dict:
    pth, ewt = H.thresholds_from_sums(ix.threshold_sums(), n_tar, G - n_tar)
    if given >= 0:
        pth, ewt = given, 0.3 * (1 - given) * n_tar
    f = ix.filter_graph(ewt)
    _, nn, ne = f.sizes()
    row = dict(genomes=G, target_ancestors=ta, n_tar=n_tar, penalty_th=pth, penalty_th_given=given >= 0, edge_weight_th=ewt,
               filtered_nodes=nn, filtered_edges=ne, seeds=f.subgraph_seeds(pth))
    walls, res, st = [], None, None
    for r in range(a.reps + 1):   # the first call is a warm-up (code objects, pool)
        rng = random.Random(a.seed)
        t0 = time.perf_counter()
        try:
            sg = f.subgraphs(pth, 3, 100, rng)
            offs, hashes = sg.csr()
        except RuntimeError:
            sg = None
        t1 = time.perf_counter()
        if r:
            walls.append((t1 - t0) * 1e3)
        if sg is not None:
            st = sg.stats()
            res = (offs, hashes, rng.random())
            sg.close()
    row.update(device_wall_ms=min(walls), device_wall_ms_all=walls)
    if st:
        row.update(st)
        row["subgraphs"] = st["kept"]
    if not a.no_host:
        _, fn, fe = f.export()
        rng = random.Random(a.seed)
        t0 = time.perf_counter()
        try:
            sgs, _, _ = H.get_subgraphs(fn, fe, pth, 3, 100, rng)
            ok = res is not None and H.csr_to_sets(res[0], res[1]) == sgs and rng.random() == res[2]
        except RuntimeError:
            ok = res is None
        row["host_restatement_s"] = time.perf_counter() - t0
        row["equal"] = bool(ok)
        try:
            import networkx as nx
            t0 = time.perf_counter()
            g = nx.Graph()
            g.add_weighted_edges_from(fe.view(np.uint64).reshape(-1, 3), weight="weight")
            nx.set_node_attributes(g, values=dict(zip(fn["hash"], fn["penalty"])), name="penalty")
            row["host_networkx_build_s"] = time.perf_counter() - t0
            del g
        except ImportError:
            row["host_networkx_build_s"] = None
    f.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[2048, 15000])
    ap.add_argument("--target-ancestors", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--penalty-th", type=float, nargs="+", default=[-1.0, 0.2],
                    help="-1: computed from the sketches (kmers.py:426-440); otherwise given, as --penalty-th is to the reference "
                         "(the edge-weight threshold follows from it, kmers.py:453)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    rows = []
    for G in a.genomes:
        b = Batch.synthetic(G, 50, 100_000, n_ancestors=30, snp_ppm=10_000, seed=a.seed)
        for ta in a.target_ancestors:
            tar = [g % 30 < ta for g in range(G)]
            ix = b.build_index(21, 200, tar)
            for given in a.penalty_th:
                row = run_case(ix, G, ta, sum(tar), given, a)
                print(json.dumps(row), flush=True)
                rows.append(row)
            ix.close()
        b.close()
    if a.json:
        Path(a.json).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
