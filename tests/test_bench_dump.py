"""bench.py --dump-outputs on a stand-in index (no GPU): float64 files only, exact 64-bit hashes, a fixed sample of long arrays
within the size limit, the same files from run to run."""
import numpy as np

from bench import DUMP_ROWS, dump_outputs   # (the repository root is on sys.path: tests/conftest.py)
from seqwin_amd import EDGE_DTYPE, KMER_DTYPE, NODE_DTYPE


class _Index:
    def __init__(self, n_kmers, n_nodes, n_edges):
        rng = np.random.default_rng(7)
        self.kmers = np.zeros(n_kmers, KMER_DTYPE)
        self.kmers["pos"] = rng.integers(0, 2**32, n_kmers, dtype=np.uint32)
        self.kmers["record_idx"] = rng.integers(0, 2**32, n_kmers, dtype=np.uint32)
        self.nodes = np.zeros(n_nodes, NODE_DTYPE)
        self.nodes["hash"] = rng.integers(0, 2**64, n_nodes, dtype=np.uint64)
        self.nodes["start"] = np.arange(n_nodes)
        self.nodes["stop"] = np.arange(n_nodes) + 1
        self.nodes["n_tar"] = rng.integers(0, 2**32, n_nodes, dtype=np.uint32)
        self.nodes["penalty"] = rng.standard_normal(n_nodes)
        self.edges = np.zeros(n_edges, EDGE_DTYPE)
        self.edges["first"] = rng.integers(0, 2**64, n_edges, dtype=np.uint64)
        self.edges["second"] = rng.integers(0, 2**64, n_edges, dtype=np.uint64)
        self.edges["weight"] = rng.integers(1, 1000, n_edges)

    def export(self):
        return self.kmers, self.nodes, self.edges


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.iterdir())}


def test_dump_outputs_small_arrays_whole_and_exact(tmp_path):
    ix = _Index(1000, 300, 500)
    dump_outputs(ix, tmp_path)
    f = _load(tmp_path)
    assert all(v.dtype == np.float64 for v in f.values()) and not any(k.endswith("_index") for k in f)
    assert f["counts"].tolist() == [1000, 300, 500]
    assert np.array_equal(f["kmers_pos"], ix.kmers["pos"].astype(np.float64))
    h = (f["nodes_hash_hi"].astype(np.uint64) << np.uint64(32)) | f["nodes_hash_lo"].astype(np.uint64)
    assert np.array_equal(h, ix.nodes["hash"]) and np.array_equal(f["nodes_penalty"], ix.nodes["penalty"])
    e = (f["edges_second_hi"].astype(np.uint64) << np.uint64(32)) | f["edges_second_lo"].astype(np.uint64)
    assert np.array_equal(e, ix.edges["second"])


def test_dump_outputs_samples_long_arrays_at_fixed_positions(tmp_path):
    n = {name: rows + 12345 for name, rows in DUMP_ROWS.items()}
    ix = _Index(n["kmers"], n["nodes"], n["edges"])
    dump_outputs(ix, tmp_path / "a")
    dump_outputs(ix, tmp_path / "b")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum((tmp_path / "a" / f"{k}.npy").stat().st_size for k in a) <= 64 << 20
    for name, arr in (("kmers", ix.kmers), ("nodes", ix.nodes), ("edges", ix.edges)):
        idx = a[f"{name}_index"].astype(np.int64)
        assert len(idx) == DUMP_ROWS[name] and np.all(np.diff(idx) > 0) and idx[-1] < n[name]
    assert np.array_equal(a["kmers_record_idx"], ix.kmers["record_idx"][a["kmers_index"].astype(np.int64)].astype(np.float64))
    idx = a["edges_index"].astype(np.int64)
    assert np.array_equal(a["edges_weight"], ix.edges["weight"][idx].astype(np.float64))
