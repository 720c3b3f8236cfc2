#!/usr/bin/env python3
"""Time the oligo search (csrc/oligo.hip) on synthetic bacteria15k genomes.

    python tests/tools/oligo_time.py --genomes 15000 [--pairs 2048] [--mismatch 0 3] [--reps 2] [--screen] [--json OUT] [--notes OUT]

The batch, the index (k=21, w=200), the walk and the marker step are those of tests/tools/screen_time.py; the oligos are cut from the
representatives of all subgraphs (4 085 at 15 000 genomes): the first 20 bases of each as the forward primer, the reverse complement
of the last 20 as the reverse primer -- 2 x 4 085 exceeds the 4 096 oligos a call takes, so the first --pairs (2 048) pairs are used.
Timed, as the library's HIP events report them (OligoHits.stats), behind one warm-up call, --reps runs each: max_mismatch of --mismatch,
with and without sites=True.  Derived: windows/s, window x oligo x strand comparisons/s, time per pass.  --screen also times
Batch.screen's probe pass (k = 21, the representatives) in the same process: the yardstick of profiles/screen_time.json.  The
comparison rate is to be set against the VALU issue rate of the device.
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
    ap.add_argument("--genomes", type=int, nargs="+", default=[15000])
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--mismatch", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-sites", action="store_true", help="skip the sites=True runs")
    ap.add_argument("--screen", action="store_true", help="also time Batch.screen(representatives, 21) on the same batch")
    ap.add_argument("--json", default=None)
    ap.add_argument("--notes", default=None, help="write a NOTES.md paragraph with the figures here")
    a = ap.parse_args()
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    out, notes = [], []
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
        reps = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        for x in (m, kept, sg, f, ix):
            x.close()
        usable = [t for t in reps if len(t) >= 40 and b"N" not in t][:a.pairs]
        oligos = [x for t in usable for x in (t[:20], t[-20:].translate(COMP)[::-1])]
        row = dict(genomes=G, representatives=len(reps), pairs=len(usable), oligos=len(oligos), total_bp=b.info()["total_bp"], runs=[])
        print(json.dumps({k: v for k, v in row.items() if k != "runs"}), flush=True)
        b.oligo_hits(oligos[:2], 0).close()                # the warm-up (code objects, pool)
        for mm in a.mismatch:
            for sites in ((False,) if a.no_sites else (False, True)):
                best = None
                for r in range(a.reps):
                    t0 = time.perf_counter()
                    h = b.oligo_hits(oligos, mm, 0, sites=sites)
                    t1 = time.perf_counter()
                    st = h.stats()
                    h.close()
                    st["call_wall_ms"] = (t1 - t0) * 1e3
                    if best is None or st["scan_ms"] < best["scan_ms"]:
                        best = st
                best.update(max_mismatch=mm, sites=sites, windows_per_s=best["windows"] / best["scan_ms"] * 1e3,
                            comparisons_per_s=best["comparisons"] / best["scan_ms"] * 1e3, ms_per_pass=best["scan_ms"] / max(best["passes"], 1))
                print(json.dumps(best), flush=True)
                row["runs"].append(best)
        if a.screen:
            probe = []
            for r in range(a.reps + 1):
                s = b.screen(reps, 21)
                if r:
                    probe.append(s.stats()["probe_ms"])
                s.close()
            row["screen_probe_ms"] = min(probe)
            print(json.dumps(dict(screen_probe_ms=row["screen_probe_ms"])), flush=True)
        out.append(row)
        for x in row["runs"]:
            notes.append(f"{G} genomes, {row['oligos']} oligos, max_mismatch {x['max_mismatch']}, sites={x['sites']}: scan {x['scan_ms']:.0f} ms in "
                         f"{x['passes']} pass(es) ({x['ms_per_pass']:.0f} ms per pass), {x['windows_per_s']:.3g} windows/s, "
                         f"{x['comparisons_per_s']:.3g} comparisons/s, {x['hits']} hits, order {x['order_ms']:.0f} ms")
        if "screen_probe_ms" in row:
            notes.append(f"{G} genomes: Batch.screen's probe pass in the same process {row['screen_probe_ms']:.0f} ms")
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    if a.notes:
        Path(a.notes).parent.mkdir(parents=True, exist_ok=True)
        Path(a.notes).write_text("Oligo search, measured by tests/tools/oligo_time.py: " + "; ".join(notes) + ".\n")


if __name__ == "__main__":
    main()
