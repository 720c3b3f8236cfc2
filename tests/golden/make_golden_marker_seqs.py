#!/usr/bin/env python3
"""Record the representative sequences of the marker goldens by running the REAL reference's Assemblies.fetch_seq.

Run in the dev container only (needs the reference checkout, its compiled extension and pandas):
    make -C oracle ref && python tests/golden/make_golden_marker_seqs.py [/path/to/reference]

For every case of tests/golden/markers/manifest.json the representative rows (`reps` of markers/<graph>_c<case>.npz: assembly_idx,
record_idx, start, stop) go through Assemblies.fetch_seq (src/seqwin/assemblies.py:101-141), as markers._fetch_cks_seq calls it with
rep_only=True (markers.py:443-465), over the graph's FASTA files.  Stored per case (markers/<graph>_c<case>_seqs.npz): rep_seq_offsets
and rep_seq_blob (the strings back to back, ASCII).  Only recorded results are stored; no reference source text is copied.
"""
from __future__ import annotations

import json
import logging
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

logging.disable(logging.CRITICAL)
HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
OUT = HERE / "markers"
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402

REF = Path(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
sys.path.insert(0, str(REF / "src"))
_core = oracle.load_ref()
if _core is None:
    raise SystemExit("build the reference extension first: make -C oracle ref")
sys.modules["seqwin.graph._core"] = _core
import pandas as pd  # noqa: E402
from seqwin.assemblies import Assemblies  # noqa: E402


def main():
    cases = json.loads((OUT / "manifest.json").read_text())["cases"]
    graphs = {g["name"]: g for g in json.loads((HERE / "subgraphs" / "manifest.json").read_text())["graphs"]}
    for c in cases:
        if c["error"] is not None:
            continue
        g = graphs[c["graph"]]
        reps = np.load(OUT / f"{c['graph']}_c{c['case']}.npz")["reps"]
        loc = pd.DataFrame({f: reps[f].astype(np.int64) for f in ("assembly_idx", "record_idx", "start", "stop")})
        holder = SimpleNamespace(path=pd.Series([HERE / p for p in g["paths"]]))
        seqs = Assemblies.fetch_seq(holder, loc, 1).to_list()
        assert len(seqs) == len(reps) and all(len(s) == int(r["stop"]) - int(r["start"]) for s, r in zip(seqs, reps))
        offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
        blob = np.frombuffer("".join(seqs).encode("ascii"), np.uint8)
        np.savez_compressed(OUT / f"{c['graph']}_c{c['case']}_seqs.npz", rep_seq_offsets=offs, rep_seq_blob=blob)
        print(c["graph"], c["case"], len(seqs), "representatives,", len(blob), "bases")


if __name__ == "__main__":
    main()
