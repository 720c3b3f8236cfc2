#!/usr/bin/env python3
"""Time the best hits with shared seeds (csrc/hits.hip: owner lists + k_hit_probe_shared) against the default route on synthetic
bacteria15k genomes.

    python tests/tools/shared_seeds_time.py [--genomes 15000] [--kmerlen 21] [--reps 2] [--json profiles/shared_seeds_time.json]

The batch, the index (k=21, w=200), the walk, the marker step and the queries (the representatives of all subgraphs: 4 085 at
15 000 genomes) are those of tests/tools/best_hits_time.py.  Four runs in one process on one batch, each a warm-up call and --reps
timed ones, the one with the fastest probe pass kept: (1) the default call; (2) seed_copies=1 -- the same result, the difference is
the owner-list indirection and the second walk; (3) seed_copies=16; (4) the representatives given twice at seed_copies=2.  Timed as
the library's HIP events report them (BestHits.stats), with the whole call on the host clock, the seed stats and the total hits.
"""
from __future__ import annotations

import argparse
import json
import random
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[15000])
    ap.add_argument("--kmerlen", type=int, default=21)
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import numpy as np

    from seqwin_amd.device import Batch, set_device
    set_device(0)
    out = []
    for G in a.genomes:
        b = Batch.synthetic(G, 50, 100_000, n_ancestors=30, snp_ppm=10_000, seed=a.seed)
        tar = [g % 30 < 1 for g in range(G)]
        n_tar = sum(tar)
        ix = b.build_index(21, 200, tar)
        f = ix.filter_graph(0.3 * (1 - a.penalty_th) * n_tar)
        sg = f.subgraphs(a.penalty_th, 3, 100, random.Random(a.seed))
        kept = ix.filter_kmers(f, sg)
        m = kept.marker_locs(sg, b.record_offsets(), n_tar, 21, 200)
        offs, blob, _ = m.sequences(b, "reps")
        o = offs.astype("int64")
        queries = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        for x in (m, kept, sg, f, ix):
            x.close()
        row = dict(genomes=G, n_tar=n_tar, kmerlen=a.kmerlen, queries=len(queries), query_bytes=len(blob), total_bp=b.info()["total_bp"], reps=a.reps)
        print(json.dumps(row), flush=True)
        runs = [("default", queries, None), ("seed_copies_1", queries, 1), ("seed_copies_16", queries, 16), ("twice_seed_copies_2", queries + queries, 2)]
        ref = None
        for name, qs, c in runs:
            best, probes, sides, walls = None, [], [], []
            for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
                t0 = time.perf_counter()
                h = b.best_hits(qs, a.kmerlen, seed_copies=c)
                t1 = time.perf_counter()
                st = h.stats()
                if r:
                    probes.append(st["probe_ms"])
                    sides.append(st["query_ms"])
                    walls.append((t1 - t0) * 1e3)
                if r and (best is None or st["probe_ms"] < best["probe_ms"]):
                    dist = h.dist()
                    best = dict(st, call_wall_ms=(t1 - t0) * 1e3, seed_stats=h.seed_stats(), pairs_with_a_hit=int((dist != 0xFFFFFFFF).sum()),
                                pairs_at_distance_0=int((dist == 0).sum()))
                    if name == "default":
                        ref = dist
                    elif name == "seed_copies_1":
                        best["equals_default"] = bool(np.array_equal(dist, ref))
                    elif name == "twice_seed_copies_2":
                        best["halves_equal_default"] = bool(np.array_equal(dist[:len(queries)], ref) and np.array_equal(dist[len(queries):], ref))
                    del dist
                h.close()
            best.update(probe_ms_all=probes, query_ms_all=sides, call_wall_ms_all=walls)
            row[name] = best
            print(json.dumps({name: best}), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
