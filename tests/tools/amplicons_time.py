#!/usr/bin/env python3
"""Time the amplicon stage (csrc/amplicons.hip) against the host route it replaces, on synthetic bacteria15k genomes.

    python tests/tools/amplicons_time.py [--genomes 2048] [--pairs 2048] [--mismatch 3] [--max-edits N --oligos 128] [--host-limit-s 600]
                                         [--json profiles/amplicons_time.json]

The batch and the oligos are those of tests/tools/oligo_time.py (the first and the reverse-complemented last 20 bases of the subgraph
representatives as primer pairs); the default is its recorded run: 4 096 oligos as 2 048 pairs on 2 048 genomes, max_mismatch 3,
2.8 M sites.  --max-edits N --oligos 128 --genomes 15000 is the second run.  In one process, each call behind its own warm-up:

    device   OligoHits.amplicons(pairs, 60, 3000), products=True and products=False: the call's wall time and its three event times
    host     the route of the parent: o.sites() (the export of the list) and seqwin_amd.oligos.amplicons on it, wall time each

The host route runs in a child process that is ended after --host-limit-s seconds; then that is recorded and the device time stands
alone.  Where both finish, the count matrices are compared.  The yardstick for the time is the host route, never this code."""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _host(sites, lengths, pairs, lo, hi, na, q):
    from seqwin_amd import oligos as O
    t0 = time.perf_counter()
    _, n_amp = O.amplicons(sites, lengths, pairs, lo, hi, n_assemblies=na)
    q.put((time.perf_counter() - t0, n_amp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=2048)
    ap.add_argument("--pairs", type=int, default=2048)
    ap.add_argument("--oligos", type=int, default=None, help="use only the first N oligos (N / 2 pairs)")
    ap.add_argument("--mismatch", type=int, default=3)
    ap.add_argument("--max-edits", type=int, default=None)
    ap.add_argument("--min-len", type=int, default=60)
    ap.add_argument("--max-len", type=int, default=3000)
    ap.add_argument("--penalty-th", type=float, default=0.2)
    ap.add_argument("--host-limit-s", type=float, default=600.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "amplicons_time.json"))
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
    o64 = offs.astype("int64")
    reps = [blob[o64[i]:o64[i + 1]] for i in range(len(o64) - 1)]
    for x in (m, kept, sg, f, ix):
        x.close()
    usable = [t for t in reps if len(t) >= 40 and b"N" not in t][:a.pairs]
    oligos = [x for t in usable for x in (t[:20], t[-20:].translate(COMP)[::-1])]
    if a.oligos:
        oligos = oligos[:a.oligos - a.oligos % 2]
    pairs = np.arange(len(oligos), dtype=np.uint32).reshape(-1, 2)
    if a.max_edits is None:
        o = b.oligo_hits(oligos, a.mismatch, 0, sites=True)
    else:
        o = b.oligo_hits(oligos, sites=True, max_edits=a.max_edits)
    row = dict(genomes=G, oligos=len(oligos), pairs=len(pairs), max_mismatch=None if a.max_edits is not None else a.mismatch, max_edits=a.max_edits,
               min_len=a.min_len, max_len=a.max_len, sites=o.stats()["hits"], total_bp=b.info()["total_bp"])
    print(json.dumps(row), flush=True)
    o.amplicons(pairs[:1], a.min_len, a.max_len).close()             # the warm-up (code objects, pool)
    n_dev = None
    for products in (True, False):
        t0 = time.perf_counter()
        am = o.amplicons(pairs, a.min_len, a.max_len, products=products)
        wall = (time.perf_counter() - t0) * 1e3
        st = am.stats()
        st["call_wall_ms"] = wall
        st["wave_item_share"] = st["wave_items"] / max(st["items"], 1)
        st["partners_per_product"] = st["partners"] / max(st["products"], 1)
        n_dev = am.n_amplicons()
        am.close()
        row["device_products" if products else "device_counts"] = st
        print(json.dumps(st), flush=True)
    o.sites()                                                        # the warm-up of the export
    t0 = time.perf_counter()
    S = o.sites()
    row["host_sites_export_ms"] = (time.perf_counter() - t0) * 1e3
    q = mp.get_context("spawn").Queue()
    child = mp.get_context("spawn").Process(target=_host, args=(S, o.lengths, pairs, a.min_len, a.max_len, o.sizes()[1], q))
    child.start()
    try:
        secs, n_host = q.get(timeout=a.host_limit_s)
        row["host_amplicons_ms"] = secs * 1e3
        row["host_finished"] = True
        row["counts_equal"] = bool(np.array_equal(n_host, n_dev))
    except Exception:
        row["host_finished"] = False
        row["host_limit_s"] = a.host_limit_s
    finally:
        child.terminate()
        child.join()
    print(json.dumps({k: row[k] for k in row if k.startswith("host") or k == "counts_equal"}), flush=True)
    o.close()
    b.close()
    p = Path(a.json)
    p.parent.mkdir(parents=True, exist_ok=True)
    old = json.loads(p.read_text()) if p.exists() else []
    p.write_text(json.dumps(old + [row], indent=1) + "\n")


if __name__ == "__main__":
    main()
