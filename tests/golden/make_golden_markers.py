#!/usr/bin/env python3
"""Generate the marker goldens under tests/golden/markers/ by running the REAL reference's markers._create_ck.

Run in the dev container only (needs the reference checkout, its compiled extension, pandas and networkx):
    make -C oracle ref && python tests/golden/make_golden_markers.py [/path/to/reference]

Inputs: four graphs of tests/golden/subgraphs/manifest.json (smoke_k17_w10, pan_a_k15_w20, pan_b_k21_w10, synth_pan_k15_w20) and,
of each, the walks recorded there at the reference's own penalty threshold that kept a subgraph (the last recorded walk that
kept one where none did).  Every graph is built and scored
by the oracle, filtered and walked by the reference (kmers._filter_edges_and_nodes, kmers._get_subgraphs), the kept occurrences
come from the oracle's filter_kmers, and every subgraph goes through markers._create_ck with the reference's
ConnectedKmers.__get_loc and __get_rep_order wrapped so that what they return is recorded.
Stored per case (markers/<graph>_c<case>.npz), subgraphs in the reference's final order, all values as integers:
rows / row_offsets / kmer_offsets / row_hashes (the `loc` tables), reps (the `rep` row, n_rep, flags bit 0 single, bit 1 dup),
rep_offsets / rep_hashes (rep_order).  Only recorded results are stored; no reference source text is copied.
"""
from __future__ import annotations

import json
import logging
import random
import sys
from pathlib import Path

import numpy as np

logging.disable(logging.CRITICAL)
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "markers"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oracle  # noqa: E402
import markers_host as M  # noqa: E402

REF = Path(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
sys.path.insert(0, str(REF / "src"))
_core = oracle.load_ref()
if _core is None:
    raise SystemExit("build the reference extension first: make -C oracle ref")
sys.modules["seqwin.graph._core"] = _core
from seqwin.kmers import _filter_edges_and_nodes, _get_subgraphs  # noqa: E402
from seqwin import markers as ref_markers  # noqa: E402

GRAPHS = ("smoke_k17_w10", "pan_a_k15_w20", "pan_b_k21_w10", "synth_pan_k15_w20")
CK = ref_markers.ConnectedKmers
_seen = {}
_get_loc = CK._ConnectedKmers__get_loc
_get_rep = CK._ConnectedKmers__get_rep_order


def _loc(kmers, kmerlen, windowsize):
    _seen["loc"] = _get_loc(kmers, kmerlen, windowsize)
    return _seen["loc"]


def _rep(loc, warnings):
    _seen["rep"] = _get_rep(loc, warnings)
    return _seen["rep"]


CK._ConnectedKmers__get_loc = staticmethod(_loc)
CK._ConnectedKmers__get_rep_order = staticmethod(_rep)


def one_subgraph(nxg, sg, kmers, node_of, offs, n_tar, k, w):
    arg_nodes = tuple(sg)
    arg_kmers = tuple(kmers[node_of[h]["start"]:node_of[h]["stop"]] for h in arg_nodes)
    ck = ref_markers._create_ck(nxg.subgraph(sg).copy(), arg_nodes, arg_kmers, offs, n_tar, k, w)
    loc, (order, n_rep) = _seen["loc"], _seen["rep"]
    rows = np.zeros(len(loc), M.ROW_DTYPE)
    for f in M.ROW_DTYPE.names:
        rows[f] = loc[f].to_numpy().astype(np.int64)
    seqs = [tuple(int(x) for x in t) for t in loc["kmers"]]
    rep = np.zeros((), M.REP_DTYPE)
    for f in M.ROW_DTYPE.names:
        rep[f] = int(ck.rep[f])
    assert int(ck.len) == int(ck.rep["len"]) == (int(ck.rep["stop"]) - int(ck.rep["start"])) % (1 << 32)
    rep["n_rep"] = n_rep
    rep["flags"] = (M.SINGLE if "single" in ck.warnings else 0) | (M.DUP if "dup" in ck.warnings else 0)
    assert tuple(int(x) for x in ck.rep["kmers"]) == tuple(int(x) for x in order)
    return dict(rows=rows, seqs=seqs, rep=rep, order=tuple(int(x) for x in order))


def main():
    OUT.mkdir(exist_ok=True)
    sub = json.loads((HERE / "subgraphs" / "manifest.json").read_text())
    manifest = {"cases": []}
    for g in sub["graphs"]:
        if g["name"] not in GRAPHS:
            continue
        kmers, nodes, edges, offs, _ = oracle.build([HERE / p for p in g["paths"]], g["k"], g["w"])
        oracle.get_penalty(kmers, nodes, offs, g["is_targets"])
        n_tar = sum(g["is_targets"])
        assert all(g["is_targets"][:n_tar])
        fn, fe, nxg = _filter_edges_and_nodes(nodes, edges, g["edge_weight_th"])
        ok = [ci for ci, c in enumerate(g["cases"]) if c["error"] is None]
        take = [ci for ci in ok if g["cases"][ci]["penalty_th"] == g["penalty_th_ref"]] or ok[-1:]   # (no walk kept anything there: the last that did)
        for ci in take:
            case = g["cases"][ci]
            sgs, used = _get_subgraphs(nxg, case["penalty_th"], case["min_nodes"], case["max_nodes"], random.Random(case["seed"]))
            kk, kn = oracle.filter_kmers(kmers, fn, np.array(sorted(int(x) for x in used), np.uint64))
            node_of = {n["hash"]: n for n in kn}
            try:
                res = [one_subgraph(nxg, sg, kk, node_of, offs, n_tar, g["k"], g["w"]) for sg in sgs]
            except ValueError as e:
                manifest["cases"].append(dict(graph=g["name"], case=ci, error="ValueError", n_subgraphs=len(sgs)))
                print(g["name"], ci, "ValueError:", e)
                continue
            np.savez_compressed(OUT / f"{g['name']}_c{ci}.npz", **M.tables(res))
            manifest["cases"].append(dict(graph=g["name"], case=ci, error=None, n_subgraphs=len(sgs), n_tar=n_tar,
                                          n_rows=int(sum(len(r["rows"]) for r in res))))
            print(g["name"], ci, len(sgs), "subgraphs,", manifest["cases"][-1]["n_rows"], "rows")
    (OUT / "manifest.json").write_text(json.dumps(manifest, indent=1) + "\n")


if __name__ == "__main__":
    main()
