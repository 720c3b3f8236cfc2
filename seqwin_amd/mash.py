"""``Assemblies.mash`` without the Mash binary: the n x n Jaccard matrix from device-resident MinHash sketches.

``jaccard_matrix`` returns what ``Assemblies.mash`` (src/seqwin/assemblies.py:76-99) returns -- ``mash sketch -k kmerlen -s
sketchsize`` over every assembly, ``mash dist`` over all pairs, ``shared / total`` of every output line -- computed by
csrc/minhash.hip.  INTEGRATION.md shows the lines that bind it into an unmodified Seqwin checkout.
"""
from __future__ import annotations

import numpy as np

from .device import Batch


def jaccard_matrix(batch_or_paths, kmerlen: int, sketchsize: int, n_cpu: int = 1) -> np.ndarray:
    """float64[n, n] Jaccard indices of all assembly pairs.  ``batch_or_paths``: a resident :class:`Batch`, or FASTA paths
    (read and packed on ``n_cpu`` host threads, as the build does)."""
    own = not isinstance(batch_or_paths, Batch)
    batch = Batch.from_fasta(list(batch_or_paths), n_cpu=n_cpu) if own else batch_or_paths
    try:
        mh = batch.minhash(kmerlen, sketchsize)
        try:
            return mh.jaccard()
        finally:
            mh.close()
    finally:
        if own:
            batch.close()
