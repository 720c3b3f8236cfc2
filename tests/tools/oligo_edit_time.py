#!/usr/bin/env python3
"""Time the oligo search with indels (csrc/oligo.hip) next to the Hamming search, in one process.

    python tests/tools/oligo_edit_time.py [--genomes 15000] [--oligos 128] [--edits 0 1 2 4] [--reps 2] [--json profiles/oligo_edit_time.json]

The batch and the oligos are those of tests/tools/oligo_time.py (synthetic bacteria15k genomes; the first and the reverse-complemented
last 20 bases of the representatives).  Behind one warm-up call: max_mismatch = 2 first -- it runs the kernel of the parent commit and is
to be set against its recorded figure --, then max_edits of --edits, --reps runs each, the one with the least scan time kept.  Recorded
per call, as the library's HIP events report them (OligoHits.stats): scan ms, resolve ms, order ms, sites, DP steps per second.
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

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=15000)
    ap.add_argument("--oligos", type=int, default=128)
    ap.add_argument("--edits", type=int, nargs="+", default=[0, 1, 2, 4])
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "oligo_edit_time.json"))
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    G = a.genomes
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
    reps = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
    for x in (m, kept, sg, f, ix):
        x.close()
    usable = [t for t in reps if len(t) >= 40 and b"N" not in t]
    oligos = [x for t in usable for x in (t[:20], t[-20:].translate(COMP)[::-1])][:a.oligos]
    row = dict(genomes=G, oligos=len(oligos), total_bp=b.info()["total_bp"], runs=[])
    print(json.dumps({k: v for k, v in row.items() if k != "runs"}), flush=True)
    b.oligo_hits(oligos[:2], 0).close()                      # the warm-up (code objects, pool)
    b.oligo_hits(oligos[:2], max_edits=1).close()
    for kind, v in [("max_mismatch", 2)] + [("max_edits", d) for d in a.edits]:
        best = None
        for r in range(a.reps):
            t0 = time.perf_counter()
            h = b.oligo_hits(oligos, **{kind: v})
            t1 = time.perf_counter()
            st = h.stats()
            h.close()
            st["call_wall_ms"] = (t1 - t0) * 1e3
            if best is None or st["scan_ms"] < best["scan_ms"]:
                best = st
        best.update({kind: v}, windows_per_s=best["windows"] / best["scan_ms"] * 1e3, dp_steps_per_s=best["dp_steps"] / best["scan_ms"] * 1e3)
        print(json.dumps(best), flush=True)
        row["runs"].append(best)
    ham = row["runs"][0]["scan_ms"]
    for x in row["runs"][1:]:
        x["scan_ms_over_max_mismatch_2"] = x["scan_ms"] / ham
    b.close()
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps([row], indent=1) + "\n")


if __name__ == "__main__":
    main()
