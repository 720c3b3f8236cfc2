#!/usr/bin/env python3
"""Time the marker step (markers._get_cks' per-subgraph work) on the device against the host restatement, on synthetic
bacteria15k genomes.

    python tests/tools/marker_locs_time.py --genomes 2048 15000 [--reps 3] [--host-sample 64] [--json OUT]

The batch, the index (k=21, w=200) and the walk (penalty_th 0.2, min_nodes 3, max_nodes 100, targets = the genomes of the first
ancestor) are those of tests/tools/subgraph_time.py.  The generator deals the ancestors round-robin, so that clade is not a prefix
of the assemblies, while the marker step (like the reference) takes the assemblies below n_tar as targets.  Two runs per size:

  "resident"  Index.marker_locs + Markers.reps from the resident kept index (Index.filter_kmers(f, subgraphs)) and the resident
              subgraphs to the rep table on the host, with n_tar = the clade's size.  The pairs, rows and items are the real
              ones and so are the count and row phases; the vote is over the first n_tar assemblies, NOT over the clade.
  "clade"     the kept index exported, its assemblies permuted on the host so that the clade comes first (records renumbered,
              every node's occurrences re-sorted), and Markers.from_arrays + Markers.reps on that: the clade's own vote.  Its
              wall time includes the host-side checks and the upload of the arrays; its phases are device time.

The phases are the library's HIP events (Markers.stats).  The host restatement (tests/tools/markers_host.py) runs on a SAMPLE of
the subgraphs of the "clade" arrays; its time is extrapolated linearly to all subgraphs and labelled "extrapolated", and the
sample's results are compared with the device's.  The reference's own _create_ck is not timed: its tree does not exist where the
device is.
"""
from __future__ import annotations

import argparse
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import markers_host as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, nargs="+", default=[2048, 15000])
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from seqwin_amd.device import Batch, Markers, set_device
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
        ro = b.record_offsets()
        n_sg = sg.sizes()[0]
        row = dict(genomes=G, n_tar=n_tar, subgraphs=n_sg, kept_occurrences=kept.sizes()[0])

        def timed(call):
            walls, st, res = [], None, None
            for r in range(a.reps + 1):   # the first call is a warm-up (code objects, pool)
                t0 = time.perf_counter()
                m = call()
                res = m.reps()
                t1 = time.perf_counter()
                if r:
                    walls.append((t1 - t0) * 1e3)
                st = m.stats()
                m.close()
            return dict(wall_ms=min(walls), wall_ms_all=walls, **st), res

        row["resident"], _ = timed(lambda: kept.marker_locs(sg, ro, n_tar, 21, 200))
        row["resident"]["targets"] = "the first n_tar assemblies, not the clade: the vote is not the workload's"
        # the clade first: assemblies permuted on the host, records renumbered, every node's occurrences re-sorted
        kk, kn, _ = kept.export()
        sizes = np.diff(ro.astype(np.int64))
        order = np.argsort(~np.asarray(tar), kind="stable")          # new assembly j is old assembly order[j]
        new_ro = np.concatenate([[0], np.cumsum(sizes[order])])
        new_of = np.empty(G, np.int64)
        new_of[order] = np.arange(G)
        asm = np.searchsorted(ro.astype(np.int64), kk["record_idx"].astype(np.int64), side="right") - 1
        rec = new_ro[new_of[asm]] + (kk["record_idx"].astype(np.int64) - ro.astype(np.int64)[asm])
        node = np.repeat(np.arange(len(kn)), (kn["stop"] - kn["start"]).astype(np.int64))
        o = np.lexsort((kk["pos"], rec, node))
        pk = np.empty(len(kk), kk.dtype)
        pk["record_idx"], pk["pos"] = rec[o], kk["pos"][o]
        offs, hashes = sg.csr()
        sg_nodes = np.searchsorted(kn["hash"], hashes).astype(np.uint64)
        pro = new_ro.astype(np.uint32)
        try:
            row["clade"], res = timed(lambda: Markers.from_arrays(pk, kn, offs, sg_nodes, pro, n_tar, 21, 200))
            row["clade"]["targets"] = "the clade (assemblies permuted on the host); wall includes host checks and upload"
        except ValueError as e:
            row["clade"], res = dict(error=str(e)), None
        if a.host_sample and res is not None:
            take = np.random.default_rng(a.seed).choice(n_sg, min(a.host_sample, n_sg), replace=False)
            ob = offs.astype(np.int64)
            s_off = np.concatenate([[0], np.cumsum(ob[take + 1] - ob[take])]).astype(np.uint64)
            s_nodes = np.concatenate([sg_nodes[ob[i]:ob[i + 1]] for i in take]).astype(np.uint64)
            t0 = time.perf_counter()
            want = M.tables(M.markers(pk, kn, s_off, s_nodes, pro, n_tar, 21, 200))
            dt = time.perf_counter() - t0
            ro2 = res[1].astype(np.int64)
            ok = all(np.array_equal(res[0][i], want["reps"][j]) and
                     np.array_equal(res[2][ro2[i]:ro2[i + 1]], want["rep_hashes"][int(want["rep_offsets"][j]):int(want["rep_offsets"][j + 1])])
                     for j, i in enumerate(take))
            row.update(host_restatement_sample=len(take), host_restatement_sample_s=dt,
                       host_restatement_s_extrapolated=dt * n_sg / len(take), equal_on_sample=bool(ok))
        print(json.dumps(row), flush=True)
        out.append(row)
        for x in (kept, sg, f, ix, b):
            x.close()
    if a.json:
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
