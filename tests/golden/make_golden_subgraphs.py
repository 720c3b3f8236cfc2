#!/usr/bin/env python3
"""Generate the subgraph-walk goldens under tests/golden/subgraphs/ by running the REAL reference's kmers._get_subgraphs.

Run in the dev container only (needs the reference checkout and its compiled extension):
    make -C oracle ref && python tests/golden/make_golden_subgraphs.py [/path/to/reference]

Graphs: the committed smoke and synth FASTA files and two seeded pan-genome sets written here (subgraphs/pan_a_*.fa.gz,
subgraphs/pan_b_*.fa.gz).  Each is built (oracle.build + oracle.get_penalty, both pinned to the reference by
tests/golden/manifest.json), filtered by the reference's kmers._filter_edges_and_nodes at the reference's edge-weight threshold,
and walked by the reference's kmers._get_subgraphs for a grid of (penalty_th, min_nodes, max_nodes, rng seed).
Stored: the filtered inputs (graph_<name>.npz: node hashes, penalties, edges), the parameters and the rng state after the call
(manifest.json: rng.random() drawn afterwards; the error text when nothing was kept) and the expected subgraphs as CSR in the
reference's final order (cases_<name>.npz).  Nodes are stored by rank in the graph's ascending hashes (edges too) to keep the
fixtures small; tests/tools/subgraphs_host.py: load_golden rebuilds the arrays.  Only inputs and outputs are stored; no reference source text is copied.
"""
from __future__ import annotations

import gzip
import json
import random
import sys
from pathlib import Path

import logging

import numpy as np

logging.disable(logging.CRITICAL)
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "subgraphs"
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402

REF = Path(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
sys.path.insert(0, str(REF / "src"))
_core = oracle.load_ref()
if _core is None:
    raise SystemExit("build the reference extension first: make -C oracle ref")
sys.modules["seqwin.graph._core"] = _core
from seqwin.kmers import _filter_edges_and_nodes, _get_subgraphs  # noqa: E402

SMOKE = ["smoke/targets/target-1.fasta", "smoke/targets/target-2.fasta", "smoke/non-targets/non-target-1.fasta",
         "smoke/non-targets/non-target-2.fasta"]


def pan_set(tag: str, n_genomes: int, n_anc: int, length: int, snp: float, seed: int) -> list[str]:
    rng = np.random.default_rng(seed)
    B = np.array(list("ACGT"))
    anc = [B[rng.integers(0, 4, length)] for _ in range(n_anc)]
    paths = []
    for g in range(n_genomes):
        a = anc[g % n_anc].copy()
        hit = rng.random(length) < snp
        a[hit] = B[rng.integers(0, 4, int(hit.sum()))]
        s = "".join(a)
        cut = int(rng.integers(length // 3, 2 * length // 3))
        text = f">{tag}{g}_c1\n" + "\n".join(s[i:i + 80] for i in range(0, cut, 80)) + "\n"
        text += f">{tag}{g}_c2\n" + "\n".join(s[i:i + 80] for i in range(cut, length, 80)) + "\n"
        p = OUT / f"{tag}_{g}.fa.gz"
        with gzip.GzipFile(p, "wb", mtime=0) as f:
            f.write(text.encode())
        paths.append(str(p.relative_to(HERE)))
    return paths


def thresholds(nodes, n_tar: int, n_neg: int, stringency: int = 5, edge_w_th_mul: float = 0.3, cap: float = 0.2):
    """penalty_th from minimizer sketches and edge_weight_th, as kmers.filter_graph computes them (kmers.py:426-453)."""
    nt = nodes["n_tar"]
    e_abs = 1 - np.sum((nt / n_tar) * nt) / np.sum(nt)
    e_pre = np.sum((nodes["n_neg"] / n_neg) * nt) / np.sum(nt)
    th = (1 - stringency / 10) * (e_abs * e_pre) ** 0.5
    th = min(float(th), cap)
    return th, edge_w_th_mul * (1 - th) * n_tar


def main():
    OUT.mkdir(exist_ok=True)
    graphs = [
        ("smoke_k17_w10", SMOKE, 17, 10, [True, True, False, False]),
        ("smoke_k7_w10", SMOKE, 7, 10, [True, True, False, False]),
        ("synth_pan_k15_w20", [f"synth/pan_{i}.fa" for i in range(6)], 15, 20, [True, True, True, False, False, False]),
        ("synth_long_k19_w33", [f"synth/long_{i}.fa" for i in range(3)], 19, 33, [True, True, False]),
        ("pan_a_k15_w20", pan_set("pan_a", 12, 3, 16000, 0.01, 11), 15, 20, [i < 7 for i in range(12)]),
        ("pan_b_k21_w10", pan_set("pan_b", 10, 1, 7000, 0.03, 12), 21, 10, [i < 5 for i in range(10)]),
    ]
    manifest = {"graphs": []}
    for gi, (name, paths, k, w, tar) in enumerate(graphs):
        kmers, nodes, edges, offs, _ = oracle.build([HERE / p for p in paths], k, w)
        oracle.get_penalty(kmers, nodes, offs, tar)
        n_tar = sum(tar)
        pth, ewt = thresholds(nodes, n_tar, len(tar) - n_tar)
        fn, fe, nxg = _filter_edges_and_nodes(nodes, edges, ewt)
        rank_t = np.uint16 if len(fn) < 1 << 16 else np.uint32
        h = fn["hash"]
        np.savez_compressed(OUT / f"graph_{name}.npz", hash=h, penalty=fn["penalty"],
                            first=np.searchsorted(h, fe["first"]).astype(rank_t), second=np.searchsorted(h, fe["second"]).astype(rank_t),
                            weight=fe["weight"].astype(np.uint32))
        pens = np.sort(fn["penalty"])
        ths = [0.0, pth, float(pens[len(pens) // 2]) if len(pens) else 0.5, float(pens[-1]) + 1.0 if len(pens) else 2.0]
        cases, arrays = [], {}
        i = 0
        for ti, th in enumerate(ths):
            for mi, mx in enumerate([None, 1, 3, 100]):
                mn = [1, 3, 5][(ti + mi + gi) % 3]
                seed = 1000 * gi + 10 * ti + mi
                rng = random.Random(seed)
                case = dict(penalty_th=th, min_nodes=mn, max_nodes=mx, seed=seed)
                try:
                    sgs, used = _get_subgraphs(nxg, th, mn, mx, rng)
                    lens = [len(s) for s in sgs]
                    arrays[f"c{i}_offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
                    hs = np.array([x for s in sgs for x in sorted(int(y) for y in s)], np.uint64)
                    arrays[f"c{i}_ranks"] = np.searchsorted(h, hs).astype(rank_t)   # node ranks, ascending inside a subgraph
                    case.update(error=None, n_subgraphs=len(sgs), n_used=len(used))
                    assert len(used) == sum(lens)
                except RuntimeError as e:
                    case.update(error=str(e), n_subgraphs=0, n_used=0)
                case["rng_after"] = rng.random()
                cases.append(case)
                i += 1
        np.savez_compressed(OUT / f"cases_{name}.npz", **arrays)
        manifest["graphs"].append(dict(name=name, paths=paths, k=k, w=w, is_targets=tar, penalty_th_ref=pth, edge_weight_th=ewt,
                                       n_nodes=len(fn), n_edges=len(fe), cases=cases))
        print(name, len(nodes), "nodes ->", len(fn), "filtered,", len(fe), "edges; subgraphs per case:",
              [c["n_subgraphs"] for c in cases])
    (OUT / "manifest.json").write_text(json.dumps(manifest, indent=1) + "\n")


if __name__ == "__main__":
    main()
