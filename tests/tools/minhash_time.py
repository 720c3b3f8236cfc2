#!/usr/bin/env python3
"""Time the MinHash step (Assemblies.mash's replacement, csrc/minhash.hip) on synthetic bacteria15k genomes.

    python tests/tools/minhash_time.py --genomes 2048 15000 [--reps 2] [--json OUT]

The batch is that of tests/tools/marker_locs_time.py (50 records of 100 kbp per genome, 30 ancestors, 1 % SNPs); k = 21,
S = 1000.  Targets are the genomes of the first ancestor, as the benchmark splits them; the pair block is the n_tar x n block the
reference needs (rows: the first n_tar assemblies, as MinHash.penalty_fracs takes them).  Timed: the hash / pre-select pass and
the selection (the library's HIP events, MinHash.stats), the pair block to the host (wall, MinHash.counts), the two reductions of
kmers.py:419-420 (wall, MinHash.penalty_fracs: pairs + row sums, nothing but the row sums leaves the device).  Recorded: how many
assemblies took the general route.  There is no reference figure: the `mash` binary cannot be run here.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[2048, 15000])
    ap.add_argument("--kmerlen", type=int, default=21)
    ap.add_argument("--sketchsize", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    out = []
    for G in a.genomes:
        b = Batch.synthetic(G, 50, 100_000, n_ancestors=30, snp_ppm=10_000, seed=a.seed)
        n_tar = sum(g % 30 < 1 for g in range(G))
        row = dict(genomes=G, n_tar=n_tar, kmerlen=a.kmerlen, sketchsize=a.sketchsize, total_bp=b.info()["total_bp"])
        sketch_wall, hash_ms, select_ms, pair_ms, reduce_ms = [], [], [], [], []
        for r in range(a.reps + 1):            # the first call is a warm-up (code objects, pool)
            t0 = time.perf_counter()
            mh = b.minhash(a.kmerlen, a.sketchsize)
            t1 = time.perf_counter()
            st = mh.stats()
            shared, total = mh.counts((0, n_tar), None)
            t2 = time.perf_counter()
            fr = mh.penalty_fracs(n_tar)
            t3 = time.perf_counter()
            if r:
                sketch_wall.append((t1 - t0) * 1e3)
                hash_ms.append(st["hash_ms"])
                select_ms.append(st["select_ms"])
                pair_ms.append((t2 - t1) * 1e3)
                reduce_ms.append((t3 - t2) * 1e3)
            row.update(general_route=st["general_route"], candidates=st["candidates"], largest_candidates=st["largest_candidates"],
                       capacity=st["capacity"], n_hashes=mh.sizes()[1], e_absence_tar=fr[0], e_presence_neg=fr[1],
                       mean_shared=float(shared.mean()), pairs=int(shared.size))
            mh.close()
        row.update(sketch_wall_ms=min(sketch_wall), hash_ms=min(hash_ms), select_ms=min(select_ms), pair_block_ms=min(pair_ms),
                   reduce_ms=min(reduce_ms), hash_gkmers_per_s=row["total_bp"] / min(hash_ms) / 1e6)
        print(json.dumps(row), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
