#!/usr/bin/env python3
"""Time the interval fetch and the row edit distances (csrc/seqs.hip) on synthetic bacteria15k genomes with the rows kept.

    python tests/tools/marker_seqs_time.py --genomes 2048 15000 [--reps 3] [--host-sample 64] [--host-rows 3] [--json OUT]

The batch, the index (k=21, w=200), the walk and the marker step are those of tests/tools/marker_locs_time.py's "resident" run
(n_tar = the clade's size, targets = the first n_tar assemblies), with keep_rows=True.  Timed, as the library's HIP events report
them (no download of the text): the fetch of the representatives, the fetch of every row -- with the bytes written and the GB/s
that implies --, and Markers.row_distances with its pairs, the total cell count sum |R| |S|, the share of pairs on the striped
(HBM) route and the longest pair.  The host restatement (tests/tools/seqs_host.py) runs on --host-rows rows (first, middle, last)
of each of a SAMPLE of subgraphs; its time is extrapolated to all rows by the cell count and labelled "extrapolated", and the
sample's results are compared with the device's.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import seqs_host as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[2048, 15000])
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--host-rows", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from seqwin_amd._core import _ptr
    from seqwin_amd._lib import c_u64, c_vp, check, lib
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
        m = kept.marker_locs(sg, b.record_offsets(), n_tar, 21, 200, keep_rows=True)
        n_sg, _, n_rows, _ = m.sizes()
        row = dict(genomes=G, n_tar=n_tar, subgraphs=n_sg, rows=n_rows)
        print(json.dumps(row), flush=True)
        sel = np.ascontiguousarray(m.order, np.uint64)

        def fetch(rows):
            best = None
            for r in range(a.reps + 1):   # the first call is a warm-up (code objects, pool)
                h, c, ms = c_vp(), (c_u64 * 2)(), (ctypes.c_double * 1)()
                t0 = time.perf_counter()
                check(lib.sw_markers_fetch(m._h, b._h, ctypes.c_int(rows), _ptr(sel), c_u64(len(sel)), ctypes.byref(h)))
                wall = (time.perf_counter() - t0) * 1e3
                check(lib.sw_seqs_stats(h, c, ms))
                lib.sw_seqs_free(h)
                if r and (best is None or ms[0] < best["device_ms"]):
                    best = dict(device_ms=ms[0], wall_ms=wall, launches=int(c[0]), bytes=int(c[1]))
            best["GB_per_s_written"] = best["bytes"] / best["device_ms"] / 1e6 if best["device_ms"] else None
            return best

        row["fetch_reps"] = fetch(0)
        row["fetch_rows"] = fetch(1)
        print(json.dumps(dict(fetch_reps=row["fetch_reps"], fetch_rows=row["fetch_rows"])), flush=True)
        best = None
        for r in range(a.reps + 1):
            t0 = time.perf_counter()
            dist, strand, st = m.row_distances(b, stats=True)
            wall = (time.perf_counter() - t0) * 1e3
            if r and (best is None or st["distance_ms"] < best["distance_ms"]):
                best = dict(st, wall_ms=wall)
        best["striped_share"] = best["striped_pairs"] / best["pairs"] if best["pairs"] else 0.0
        best["Gcells_per_s"] = best["cells"] / best["distance_ms"] / 1e6 if best["distance_ms"] else None
        best["nonzero_rows"] = int((dist != 0).sum())
        best["reverse_rows"] = int(strand.sum())
        row["row_distances"] = best
        print(json.dumps(dict(row_distances=best)), flush=True)
        if a.host_sample and n_sg:
            take = np.random.default_rng(a.seed).choice(n_sg, min(a.host_sample, n_sg), replace=False)
            ro, rb, _ = m.sequences(b, "reps", select=take)
            reps = [rb[int(ro[i]):int(ro[i + 1])].decode() for i in range(len(take))]
            so, sb, _ = m.sequences(b, "rows", select=take)
            dd, ds = m.row_distances(b, select=take)
            per = m.rows()
            counts = [len(per[i][0]) for i in take]
            base = np.concatenate([[0], np.cumsum(counts)])
            cells, dt, ok, pairs = 0, 0.0, True, 0
            for j in range(len(take)):
                for x in sorted({0, counts[j] // 2, counts[j] - 1})[:a.host_rows] if counts[j] else []:
                    q = int(base[j] + x)
                    s = sb[int(so[q]):int(so[q + 1])].decode()
                    t0 = time.perf_counter()
                    want = H.distance(reps[j], s)
                    dt += time.perf_counter() - t0
                    cells += len(reps[j]) * len(s)
                    pairs += 1
                    ok = ok and want == (int(dd[q]), int(ds[q]))
            row.update(host_restatement_subgraphs=len(take), host_restatement_pairs=pairs, host_restatement_cells=cells, host_restatement_s=dt,
                       host_restatement_s_extrapolated=(dt * best["cells"] / cells if cells else None),
                       extrapolated_by="cell count: time per cell of the sampled pairs times the cells of all rows", equal_on_sample=bool(ok))
        print(json.dumps(row), flush=True)
        out.append(row)
        for x in (m, kept, sg, f, ix, b):
            x.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
