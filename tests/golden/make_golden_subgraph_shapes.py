#!/usr/bin/env python3
"""Record the subgraph walk on the adversarial graphs of tests/tools/sg_shapes.py by running the REAL reference.

Run in the dev container only (needs the reference checkout and its compiled extension):
    make -C oracle ref && python tests/golden/make_golden_subgraph_shapes.py [/path/to/reference]

Every graph of sg_shapes.cases() is generated, passed through the reference's kmers._filter_edges_and_nodes(nodes, edges, 0) and
walked by its kmers._get_subgraphs for each of the graph's (penalty_th, min_nodes, max_nodes, rng seed).  Stored in
subgraphs/shapes.json: the sha256 of the generated arrays (generator drift fails loudly), the parameters, the rng state after the
call (rng.random() drawn afterwards), the error text when nothing was kept, the counts and the sha256 of the canonical CSR
(sg_shapes.canonical_csr: the subgraphs in the reference's final order, hashes ascending inside each).  Cases with at most
SMALL_USED nodes in their subgraphs also store that CSR, as node ranks in the generated nodes, in subgraphs/shapes_cases.npz.
Only inputs and outputs are stored; no reference source text is copied.
"""
from __future__ import annotations

import json
import logging
import random
import sys
import time
from pathlib import Path

import numpy as np

logging.disable(logging.CRITICAL)
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "subgraphs"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oracle  # noqa: E402
import sg_shapes as S  # noqa: E402

REF = Path(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
sys.path.insert(0, str(REF / "src"))
_core = oracle.load_ref()
if _core is None:
    raise SystemExit("build the reference extension first: make -C oracle ref")
sys.modules["seqwin.graph._core"] = _core
from seqwin.kmers import _filter_edges_and_nodes, _get_subgraphs  # noqa: E402

SMALL_USED = 6000


def main():
    graphs, arrays = [], {}
    for gid, family, params, seed, cases in S.cases():
        t0 = time.time()
        nodes, edges = S.make(family, params, seed)
        fn, fe, nxg = _filter_edges_and_nodes(nodes, edges, 0)
        h = nodes["hash"]
        out = []
        for c in cases:
            rng = random.Random(c["seed"])
            case = dict(c)
            try:
                sgs, used = _get_subgraphs(nxg, c["penalty_th"], c["min_nodes"], c["max_nodes"], rng)
                offs, hashes = S.canonical_csr(sgs)
                assert len(used) == len(hashes)
                case.update(error=None, n_subgraphs=len(sgs), n_used=len(used), max_size=max(len(s) for s in sgs),
                            csr_sha256=S.csr_digest(offs, hashes))
                if len(hashes) <= SMALL_USED:
                    key = f"{gid}__{c['seed']}"
                    arrays[key + "__offsets"] = offs.astype(np.uint32)
                    arrays[key + "__ranks"] = np.searchsorted(h, hashes).astype(np.uint16 if len(h) < 1 << 16 else np.uint32)
                    case["stored"] = key
            except RuntimeError as e:
                case.update(error=str(e), n_subgraphs=0, n_used=0)
            case["rng_after"] = rng.random()
            out.append(case)
        graphs.append(dict(id=gid, family=family, params=params, seed=seed, sha256=S.digest(nodes, edges), n_nodes=len(nodes),
                           n_edges=len(edges), n_filtered_nodes=len(fn), n_filtered_edges=len(fe), cases=out))
        print(gid, len(nodes), "nodes,", len(edges), "edges; subgraphs per case:", [c["n_subgraphs"] for c in out],
              f"{time.time() - t0:.1f} s", flush=True)
    np.savez_compressed(OUT / "shapes_cases.npz", **arrays)
    (OUT / "shapes.json").write_text(json.dumps(dict(graphs=graphs), indent=1) + "\n")


if __name__ == "__main__":
    main()
