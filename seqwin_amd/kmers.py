"""Drop-in for the subgraph step of Seqwin's kmers.filter_graph, on the device.

``get_subgraphs`` takes the filtered ``nodes`` / ``edges`` arrays that ``kmers._filter_edges_and_nodes`` returns
(src/seqwin/kmers.py:132-173) instead of the networkx graph, and returns what ``kmers._get_subgraphs`` (kmers.py:176-312)
returns -- the same tuple of frozensets of np.uint64, the same frozenset of used hashes, the same RuntimeError when nothing is
kept -- leaving ``rng`` in the state the reference leaves it.  A caller that has the arrays skips networkx for this step.
"""
from __future__ import annotations

from .device import NO_SUBGRAPH_MSG, Index, Subgraphs  # noqa: F401


def get_subgraphs(nodes, edges, penalty_th: float, min_nodes: int, max_nodes, rng):
    """kmers._get_subgraphs on the filtered arrays: (tuple[frozenset[np.uint64], ...], frozenset[np.uint64])."""
    ix = Index.from_arrays(nodes, edges)
    try:
        sg = ix.subgraphs(penalty_th, min_nodes, max_nodes, rng)
        try:
            return sg.as_reference()
        finally:
            sg.close()
    finally:
        ix.close()
