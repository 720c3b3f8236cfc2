#!/usr/bin/env python3
"""Time the loci mode of the best hits (csrc/hits.hip) on synthetic bacteria15k genomes.

    python tests/tools/loci_time.py --genomes 15000 [--kmerlen 21] [--reps 2] [--json profiles/loci_time.json]

The batch, the index (k=21, w=200), the walk, the marker step and the queries are those of tests/tools/alignments_time.py (the
representatives of all subgraphs, 4 085 at 15 000 genomes).  In one process: best_hits(align=True) -- the code path the loci mode
leaves as it was --, then best_hits(loci=True) with min_seeds 1 and 2, each --reps times behind a warm-up: the call on the host
clock, the four stage times of loci_stats(), loci, duplicates and the largest n_loci, and the ratio of the call to align=True's.
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
        row = dict(genomes=G, n_tar=n_tar, kmerlen=a.kmerlen, queries=len(queries), query_bytes=len(blob), total_bp=b.info()["total_bp"])
        print(json.dumps(row), flush=True)
        for name, kw in (("aligned", dict(align=True)), ("loci_min_seeds_1", dict(loci=True, min_seeds=1)), ("loci_min_seeds_2", dict(loci=True, min_seeds=2))):
            runs = []
            for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
                t0 = time.perf_counter()
                h = b.best_hits(queries, a.kmerlen, **kw)
                t1 = time.perf_counter()
                if r:
                    st = {k: v for k, v in h.stats().items() if k != "chunk_hits"}
                    st["call_wall_ms"] = (t1 - t0) * 1e3
                    if "loci" in kw:
                        st["loci"] = h.loci_stats()
                    runs.append(st)
                h.close()
            row[name] = dict(runs=runs, call_wall_ms_min=min(x["call_wall_ms"] for x in runs))
            if "loci" in kw:
                best = min(runs, key=lambda x: x["call_wall_ms"])["loci"]
                row[name].update(best, ratio_to_aligned=row[name]["call_wall_ms_min"] / row["aligned"]["call_wall_ms_min"])
            print(json.dumps({name: {k: v for k, v in row[name].items() if k != "runs"}}), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
