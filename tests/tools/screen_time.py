#!/usr/bin/env python3
"""Time the exact k-mer containment screen (csrc/screen.hip) on synthetic bacteria15k genomes.

    python tests/tools/screen_time.py --genomes 2048 15000 [--kmerlen 21] [--reps 2] [--json OUT]

The batch, the index (k=21, w=200), the walk and the marker step are those of tests/tools/marker_seqs_time.py; the queries are the
representatives of all subgraphs (4 085 at 15 000 genomes), screened against every genome at --kmerlen.  Timed, as the library's
HIP events report them (Screen.stats): the query side with the table build, the probe pass and the reduce, in total and per chunk
of assemblies; on the host clock: the whole call and the download of the full counts matrix.  Derived: batch k-mers per second of
the probe pass and atomics per hit.  The figure to set the probe pass against is the MinHash hash pass over the same walk
(tests/tools/minhash_time.py); --minhash takes it in the same process, on the same batch.
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
    ap.add_argument("--minhash", action="store_true", help="also time Batch.minhash(kmerlen, 1000) on the same batch")
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
        best = None
        for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
            t0 = time.perf_counter()
            s = b.screen(queries, a.kmerlen)
            t1 = time.perf_counter()
            counts = s.counts()
            t2 = time.perf_counter()
            st = s.stats()
            if r and (best is None or st["probe_ms"] < best["probe_ms"]):
                best = dict(st, call_wall_ms=(t1 - t0) * 1e3, download_ms=(t2 - t1) * 1e3, matrix_bytes=int(counts.nbytes),
                            nonzero_pairs=int((counts != 0).sum()), full_pairs=int((counts == s.n_kmers()[:, None]).sum()))
            s.close()
            del counts
        best["probe_gkmers_per_s"] = best["batch_kmers"] / best["probe_ms"] / 1e6 if best["probe_ms"] else None
        best["atomics_per_hit"] = best["atomics"] / best["hits"] if best["hits"] else None
        row["screen"] = best
        if a.minhash:
            hash_ms = []
            for r in range(a.reps + 1):
                mh = b.minhash(a.kmerlen, 1000)
                if r:
                    hash_ms.append(mh.stats()["hash_ms"])
                mh.close()
            row["minhash_hash_ms"] = min(hash_ms)
            row["probe_over_hash"] = best["probe_ms"] / min(hash_ms)
        print(json.dumps(row), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
