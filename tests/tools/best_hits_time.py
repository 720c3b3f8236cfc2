#!/usr/bin/env python3
"""Time the best hits (csrc/hits.hip: seed vote + infix edit distance) on synthetic bacteria15k genomes.

    python tests/tools/best_hits_time.py --genomes 2048 15000 [--kmerlen 21] [--reps 2] [--json profiles/best_hits_time.json]

The batch, the index (k=21, w=200), the walk and the marker step are those of tests/tools/screen_time.py; the queries are the
representatives of all subgraphs (4 085 at 15 000 genomes), searched in every genome at --kmerlen.  Timed, as the library's HIP events
report them (BestHits.stats): the query side, the probe pass, sort + vote and the distances, with every counter and the hits of
every chunk; on the host clock: the whole call.  The yardstick for the new probe pass is the screen's probe pass on the same
queries, taken in the same process on the same batch.
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
    ap.add_argument("--genomes", type=int, nargs="+", default=[2048, 15000])
    ap.add_argument("--kmerlen", type=int, default=21)
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    from seqwin_amd.markers import hit_summary
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
        best = None
        for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
            t0 = time.perf_counter()
            h = b.best_hits(queries, a.kmerlen)
            t1 = time.perf_counter()
            st = h.stats()
            if r and (best is None or st["probe_ms"] < best["probe_ms"]):
                dist = h.dist()
                best = dict(st, call_wall_ms=(t1 - t0) * 1e3, pairs_with_a_hit=int((dist != 0xFFFFFFFF).sum()), pairs_at_distance_0=int((dist == 0).sum()),
                            mean_similarity_tar=float(hit_summary(dist, [len(q) for q in queries], n_tar)["similarity_tar"].mean()))
                del dist
            h.close()
        row["best_hits"] = best
        probe_ms = []
        for r in range(a.reps + 1):
            s = b.screen(queries, a.kmerlen)
            if r:
                probe_ms.append(s.stats()["probe_ms"])
            s.close()
        row["screen_probe_ms"] = min(probe_ms)
        row["probe_over_screen_probe"] = best["probe_ms"] / min(probe_ms) if min(probe_ms) else None
        print(json.dumps(row), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
