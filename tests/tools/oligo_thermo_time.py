#!/usr/bin/env python3
"""Time the oligo search with a nearest-neighbour model (csrc/oligo.hip) next to the search without one, in one
process.

    python tests/tools/oligo_thermo_time.py [--genomes 15000] [--oligos 128] [--mismatch 2] [--reps 4] [--json profiles/oligo_thermo_time.json]

The batch and the oligos are those of tests/tools/oligo_edit_time.py (synthetic bacteria15k genomes; the first and the
reverse-complemented last 20 bases of the representatives).  Three kinds of call: the plain one -- k_ol_scan<false>, the kernel of the
parent commit, to be set against its recorded figure --, and thermo=santalucia98() without and with sites=True (k_ol_scan<true>).  All
three are warmed up first (small and at full size); then --reps rounds, the kinds in turn, the order reversed in every other round so
that no kind is always the first of a round; the run with the least scan time of a kind is kept and every run's scan time and place
in its round is recorded.  Per call, as the library's HIP events report them (OligoHits.stats): scan, thermo, site_thermo and order
ms, hits and stable hits, and the scan time over the plain call's.
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
    ap.add_argument("--mismatch", type=int, default=2)
    ap.add_argument("--max-dg", type=int, default=-15000, help="cal/mol; n_stable counts the hits at or below it")
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "oligo_thermo_time.json"))
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    from seqwin_amd.oligos import santalucia98
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
    model = santalucia98()
    row = dict(genomes=G, oligos=len(oligos), total_bp=b.info()["total_bp"], max_mismatch=a.mismatch, max_dg=a.max_dg, runs=[])
    print(json.dumps({k: v for k, v in row.items() if k != "runs"}), flush=True)
    kinds = [("plain", dict()), ("thermo", dict(thermo=model, max_dg=a.max_dg)), ("thermo_sites", dict(thermo=model, max_dg=a.max_dg, sites=True))]
    for kind, kw in kinds:                                   # the warm-ups: code objects, then the pool and the clocks at full size
        b.oligo_hits(oligos[:2], 0, **kw).close()
    b.oligo_hits(oligos, a.mismatch).close()
    best, every = {}, {kind: [] for kind, _ in kinds}
    for r in range(a.reps):
        for place, (kind, kw) in enumerate(kinds if r % 2 == 0 else kinds[::-1]):
            t0 = time.perf_counter()
            h = b.oligo_hits(oligos, a.mismatch, **kw)
            t1 = time.perf_counter()
            st = h.stats()
            h.close()
            st["call_wall_ms"] = (t1 - t0) * 1e3
            every[kind].append(dict(round=r, place=place, scan_ms=st["scan_ms"]))
            print(json.dumps(dict(kind=kind, round=r, place=place, scan_ms=st["scan_ms"])), flush=True)
            if kind not in best or st["scan_ms"] < best[kind]["scan_ms"]:
                best[kind] = st
    for kind, _ in kinds:
        best[kind].update(kind=kind, windows_per_s=best[kind]["windows"] / best[kind]["scan_ms"] * 1e3, all_runs=every[kind])
        print(json.dumps(best[kind]), flush=True)
        row["runs"].append(best[kind])
    plain = row["runs"][0]["scan_ms"]
    for x in row["runs"][1:]:
        x["scan_ms_over_plain"] = x["scan_ms"] / plain
    b.close()
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps([row], indent=1) + "\n")


if __name__ == "__main__":
    main()
