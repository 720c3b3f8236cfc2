#!/usr/bin/env python3
"""Time the local alignment of the best hits (csrc/local.hip) on synthetic bacteria15k genomes.

    python tests/tools/local_time.py --genomes 15000 [--kmerlen 21] [--reps 2] [--modes default aligned local loci_local] [--json profiles/local_time.json]

The batch, the index (k=21, w=200), the walk, the marker step and the queries are those of tests/tools/alignments_time.py (the
representatives of all subgraphs, 4 085 at 15 000 genomes).  In one process: the default call, align=True, local=True and loci=True
with local=True, each --reps times behind a warm-up, the call on the host clock and the stages as the library's HIP events report
them -- the local stage next to the distances' and the traceback's --, the local stage's cells per second and the share of pairs in
more than one stripe.  The default and the align=True calls are there to be held against profiles/shared_seeds_time.json and
profiles/alignments_time.json: their spread over the repeated runs is recorded with them.
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

MODES = (("default", {}), ("aligned", dict(align=True)), ("local", dict(local=True)), ("loci_local", dict(loci=True, local=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[15000])
    ap.add_argument("--kmerlen", type=int, default=21)
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--modes", nargs="+", default=[n for n, _ in MODES], choices=[n for n, _ in MODES])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    from seqwin_amd.markers import local_summary
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
        for name, kw in MODES:
            if name not in a.modes:
                continue
            runs = []
            for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
                t0 = time.perf_counter()
                h = b.best_hits(queries, a.kmerlen, **kw)
                t1 = time.perf_counter()
                if r:
                    st = {k: v for k, v in h.stats().items() if k != "chunk_hits"}
                    st["call_wall_ms"] = (t1 - t0) * 1e3
                    if kw.get("align") or kw.get("loci"):
                        st["align"] = h.align_stats()
                    if kw.get("loci"):
                        st["loci"] = h.loci_stats()
                    if kw.get("local"):
                        ls = h.local_stats()
                        ls["cells_per_s"] = ls["cells"] / (ls["local_ms"] * 1e-3) if ls["local_ms"] else None
                        ls["striped_share"] = ls["striped_pairs"] / max(ls["pairs"], 1)
                        st["local"] = ls
                        if r == a.reps and not kw.get("loci"):
                            s = local_summary(h, [len(q) for q in queries], n_tar)
                            st["mean_coverage_tar"] = float(s["coverage_tar"].mean())
                            st["mean_distance_local_neg"] = float(s["distance_local_neg"].mean())
                    runs.append(st)
                h.close()
            walls = [x["call_wall_ms"] for x in runs]
            row[name] = dict(runs=runs, call_wall_ms_min=min(walls), call_wall_ms_spread=max(walls) - min(walls),
                             distance_ms_min=min(x["distance_ms"] for x in runs))
            if kw.get("local"):
                row[name]["local_ms_min"] = min(x["local"]["local_ms"] for x in runs)
        print(json.dumps(row), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
