#!/usr/bin/env python3
"""Time the pileup of the best hits (the pile walk of csrc/align.hip) on synthetic bacteria15k genomes.

    python tests/tools/pileup_time.py --genomes 15000 [--kmerlen 21] [--reps 2] [--json profiles/pileup_time.json]

The batch, the index (k=21, w=200), the marker step and the queries are those of tests/tools/alignments_time.py (the representatives
of all subgraphs, 4 085 at 15 000 genomes).  In one process: best_hits(align=True) -- the call this feature must leave as it was --
and best_hits(pileup=targets / non-targets), each --reps times behind a warm-up: the call on the host clock, the store pass and the
walk as the library's HIP events report them, the pile walk next to the plain walk, the adds issued and the table's bytes.
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
        groups = [0 if t else 1 for t in tar]
        row = dict(genomes=G, n_tar=n_tar, kmerlen=a.kmerlen, queries=len(queries), query_bytes=len(blob), total_bp=b.info()["total_bp"],
                   atomics="one add per column, result unused (the wave-combined form was not built)")
        print(json.dumps(row), flush=True)
        for pile in (False, True):
            runs = []
            for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
                t0 = time.perf_counter()
                h = b.best_hits(queries, a.kmerlen, pileup=groups) if pile else b.best_hits(queries, a.kmerlen, align=True)
                t1 = time.perf_counter()
                if r:
                    st = {k: v for k, v in h.stats().items() if k != "chunk_hits"}
                    st["call_wall_ms"] = (t1 - t0) * 1e3
                    st["align"] = h.align_stats()
                    if pile:
                        st["pileup"] = h.pileup().stats()
                        if r == a.reps:
                            depth = h.pileup().depth()
                            st["depth_sum_tar"], st["depth_sum_neg"] = int(depth[:, 0].sum()), int(depth[:, 1].sum())
                    runs.append(st)
                h.close()
            row["pileup" if pile else "aligned"] = dict(runs=runs, call_wall_ms_min=min(x["call_wall_ms"] for x in runs),
                                                        store_ms_min=min(x["align"]["store_ms"] for x in runs),
                                                        walk_ms_min=min(x["align"]["walk_ms"] for x in runs))
            print(json.dumps(row["pileup" if pile else "aligned"]), flush=True)
        row["pile_walk_over_plain_walk"] = row["pileup"]["walk_ms_min"] / row["aligned"]["walk_ms_min"]
        print(json.dumps({k: v for k, v in row.items() if k not in ("aligned", "pileup")}), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
