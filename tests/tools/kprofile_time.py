#!/usr/bin/env python3
"""Time the k-mer profile (csrc/screen.hip) on synthetic bacteria15k genomes.

    python tests/tools/kprofile_time.py --genomes 15000 [--kmerlen 21] [--reps 1] [--json profiles/kprofile_time.json]

The batch, the index (k=21, w=200), the walk and the marker step are those of tests/tools/screen_time.py; the queries are the
representatives of all subgraphs (4 085 at 15 000 genomes), the groups targets (0) and non-targets (1).  Four calls in one process,
each behind a warm-up call of its own (code objects, pool), the best of --reps kept:

    screen            Batch.screen(queries, k)                                       the plain screen
    best_hits         Batch.best_hits(queries, k, pileup=groups, window_lengths=(20,))   for scale: what the windows cost
    profile           Batch.screen(queries, k, profile=groups)
    profile_copies    Batch.screen(queries, k, profile=groups, copies=True)

Timed, as the library's HIP events report them (Screen.stats, KmerProfile.stats): table build, probe, reduce, the transposed
reduction k_scr_profile, the gather; on the host clock: the whole call.  Derived: bitmap bytes the transposed reduction read (rows x
words x 4 over all chunks) and its rate.
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
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-best-hits", action="store_true", help="leave the best_hits call out")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "kprofile_time.json"))
    a = ap.parse_args()
    import numpy as np

    from seqwin_amd.device import Batch, set_device
    set_device(0)
    out = []
    for G in a.genomes:
        b = Batch.synthetic(G, 50, 100_000, n_ancestors=30, snp_ppm=10_000, seed=a.seed)
        tar = [g % 30 < 1 for g in range(G)]
        n_tar = sum(tar)
        groups = np.array([0 if t else 1 for t in tar], np.uint8)
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

        def screen_call(**kw):
            best = None
            for r in range(a.reps + 1):        # the first call is a warm-up
                t0 = time.perf_counter()
                s = b.screen(queries, a.kmerlen, **kw)
                t1 = time.perf_counter()
                st = dict(s.stats(), call_wall_ms=(t1 - t0) * 1e3)
                st.pop("chunk_probe_ms"), st.pop("chunk_reduce_ms")
                if kw:
                    p = s.profile()
                    st.update(p.stats())
                    t2 = time.perf_counter()
                    _, present, cop = p.table()
                    st["download_ms"] = (time.perf_counter() - t2) * 1e3
                    window = present[:, 0] != p.NO_WINDOW
                    st.update(rows=int(present.shape[0]), window_rows=int(window.sum()), group_sizes=p.group_sizes().tolist(),
                              present_sum=[int(x) for x in present[window].sum(axis=0, dtype=np.int64)])
                    if cop is not None:
                        st["copies_sum"] = [int(x) for x in cop[window].sum(axis=0, dtype=np.uint64)]
                    words = (st["distinct_kmers"] + 31) // 32
                    kept_rows = int((groups != 255).sum())
                    st["bitmap_bytes_read"] = kept_rows * words * 4
                    st["profile_gb_per_s"] = st["bitmap_bytes_read"] / st["profile_ms"] / 1e6 if st["profile_ms"] else None
                s.close()
                print(json.dumps(dict(call="screen " + " ".join(sorted(kw)), run=r, call_wall_ms=st["call_wall_ms"])), flush=True)
                if r and (best is None or st["call_wall_ms"] < best["call_wall_ms"]):
                    best = st
            return best

        row["screen"] = screen_call()
        if not a.no_best_hits:
            best = None
            for r in range(a.reps + 1):
                t0 = time.perf_counter()
                h = b.best_hits(queries, a.kmerlen, pileup=groups, window_lengths=(20,))
                wall = (time.perf_counter() - t0) * 1e3
                h.close()
                print(json.dumps(dict(call="best_hits", run=r, call_wall_ms=wall)), flush=True)
                if r and (best is None or wall < best):
                    best = wall
            row["best_hits_pileup_windows20"] = dict(call_wall_ms=best)
        row["profile"] = screen_call(profile=groups)
        row["profile_copies"] = screen_call(profile=groups, copies=True)
        row["profile_over_screen_wall"] = row["profile"]["call_wall_ms"] / row["screen"]["call_wall_ms"]
        row["profile_copies_over_screen_wall"] = row["profile_copies"]["call_wall_ms"] / row["screen"]["call_wall_ms"]
        print(json.dumps(row), flush=True)
        out.append(row)
        b.close()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
