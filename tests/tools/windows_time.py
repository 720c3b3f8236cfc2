#!/usr/bin/env python3
"""Time the oligo windows of the best hits (the window walk of csrc/align.hip) on synthetic bacteria15k genomes.

    python tests/tools/windows_time.py --genomes 15000 [--kmerlen 21] [--reps 2] [--json profiles/windows_time.json]

The batch, the index (k=21, w=200), the marker step, the queries and the groups are those of tests/tools/pileup_time.py (the
representatives of all subgraphs, 4 085 at 15 000 genomes; 500 targets, 14 500 non-targets).  In one process, each --reps times behind
a warm-up: best_hits(pileup=groups) -- the call this feature must leave as it was --, then the same with window_lengths=(20,) and with
window_lengths=(18, 20, 22, 25): the call on the host clock, the store pass and the walk as the library's HIP events report them, the
finishing kernel, the windows visited, the adds issued and the table's bytes, and the window walk next to the pile walk.
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

CONFIGS = (("pileup", None), ("windows_1", (20,)), ("windows_4", (18, 20, 22, 25)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[15000])
    ap.add_argument("--kmerlen", type=int, default=21)
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--mismatch", type=int, default=2)
    ap.add_argument("--three-prime", type=int, default=3)
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
        groups = [0 if t else 1 for t in tar]
        row = dict(genomes=G, n_tar=n_tar, kmerlen=a.kmerlen, queries=len(queries), query_bytes=len(blob), total_bp=b.info()["total_bp"],
                   max_mismatch=a.mismatch, three_prime=a.three_prime,
                   adds="imperfect windows only, the finishing kernel fills MM0 (the plain three-add form was not built)")
        print(json.dumps(row), flush=True)
        for name, lengths in CONFIGS:
            runs = []
            for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
                t0 = time.perf_counter()
                if lengths is None:
                    h = b.best_hits(queries, a.kmerlen, pileup=groups)
                else:
                    h = b.best_hits(queries, a.kmerlen, pileup=groups, window_lengths=lengths, window_mismatch=a.mismatch, window_three_prime=a.three_prime)
                t1 = time.perf_counter()
                if r:
                    st = {k: v for k, v in h.stats().items() if k != "chunk_hits"}
                    st["call_wall_ms"] = (t1 - t0) * 1e3
                    st["align"] = h.align_stats()
                    st["pileup"] = h.pileup().stats()
                    if lengths is not None:
                        st["windows"] = h.windows().stats()
                    runs.append(st)
                h.close()
            res = dict(lengths=lengths, runs=runs, call_wall_ms_min=min(x["call_wall_ms"] for x in runs),
                       store_ms_min=min(x["align"]["store_ms"] for x in runs), walk_ms_min=min(x["align"]["walk_ms"] for x in runs))
            if lengths is not None:
                res.update(finish_ms_min=min(x["windows"]["finish_ms"] for x in runs), windows=runs[-1]["windows"]["windows"],
                           adds=runs[-1]["windows"]["adds"], table_bytes=runs[-1]["windows"]["table_bytes"])
            row[name] = res
            print(json.dumps(res), flush=True)
        for name in ("windows_1", "windows_4"):
            row[name + "_walk_over_pile_walk"] = row[name]["walk_ms_min"] / row["pileup"]["walk_ms_min"]
        print(json.dumps({k: v for k, v in row.items() if k not in [c[0] for c in CONFIGS]}), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
