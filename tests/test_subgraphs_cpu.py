"""The subgraph walk without a GPU: the host restatement (tests/tools/subgraphs_host.py) against goldens recorded from the
reference's kmers._get_subgraphs (tests/golden/make_golden_subgraphs.py), the permutation trick behind the device walk's
rng handling, and the new C-ABI entries."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import subgraphs_host as H  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
GRAPHS = H.load_golden(GOLDEN)


def test_goldens_cover_the_grid():
    cases = [c for _, _, _, cs in GRAPHS for c, _ in cs]
    assert len(GRAPHS) >= 6 and len(cases) >= 90
    assert {c["max_nodes"] for c in cases} == {None, 1, 3, 100}
    assert {c["min_nodes"] for c in cases} == {1, 3, 5}
    assert any(c["penalty_th"] == 0.0 for c in cases)
    assert sum(c["error"] is None for c in cases) >= 40 and any(c["error"] for c in cases)
    assert sum(p.stat().st_size for p in (GOLDEN / "subgraphs").iterdir()) < 700_000


@pytest.mark.parametrize("gi", range(len(GRAPHS)), ids=[g["name"] for g, _, _, _ in GRAPHS])
def test_restatement_reproduces_the_reference(gi):
    g, nodes, edges, cases = GRAPHS[gi]
    assert len(nodes) == g["n_nodes"] and len(edges) == g["n_edges"]
    for case, exp in cases:
        rng = random.Random(case["seed"])
        if exp is None:
            with pytest.raises(RuntimeError) as ei:
                H.get_subgraphs(nodes, edges, case["penalty_th"], case["min_nodes"], case["max_nodes"], rng)
            assert str(ei.value) == case["error"] == H.NO_SUBGRAPH_MSG
        else:
            sgs, used, _ = H.get_subgraphs(nodes, edges, case["penalty_th"], case["min_nodes"], case["max_nodes"], rng)
            want = H.csr_to_sets(*exp)
            assert sgs == want, case
            assert used == frozenset().union(*want) and len(used) == case["n_used"]
        assert rng.random() == case["rng_after"], case


def test_shuffle_depends_only_on_the_length():
    """rng.shuffle(seeds) == [seeds[i] for i in shuffled(range(n))], and both leave the rng in the same state."""
    for n in range(0, 2001):
        a, b = random.Random(n * 7 + 1), random.Random(n * 7 + 1)
        items = [np.uint64(x) for x in np.random.default_rng(n).integers(0, 1 << 63, n, dtype=np.uint64)]
        ref = list(items)
        a.shuffle(ref)
        perm = list(range(n))
        b.shuffle(perm)
        assert ref == [items[i] for i in perm]
        assert a.random() == b.random()


def test_restatement_edge_cases():
    from seqwin_amd._core import EDGE_DTYPE, NODE_DTYPE
    nodes = np.zeros(4, NODE_DTYPE)
    nodes["hash"] = [10, 20, 30, 40]
    nodes["penalty"] = [0.0, 0.5, 0.1, 0.0]
    edges = np.zeros(3, EDGE_DTYPE)
    edges["first"] = [10, 20, 30]
    edges["second"] = [20, 30, 30]    # a self-loop puts 30 in the graph; 40 is not in it
    rng = random.Random(1)
    st = rng.getstate()
    with pytest.raises(RuntimeError):
        H.get_subgraphs(nodes, edges, -1.0, 1, None, rng)   # no seed: rng untouched
    assert rng.getstate() == st
    sgs, used, _ = H.get_subgraphs(nodes, edges, 0.2, 1, 0, random.Random(2))   # max_nodes=0: single seeds
    assert sorted(len(s) for s in sgs) == [1, 1] and used == {10, 30}
    sgs, used, _ = H.get_subgraphs(nodes, edges, 0.2, 1, None, random.Random(3))
    assert used == {10, 30} and len(sgs) == 2   # 20 (0.5) lifts either mean above 0.2


def test_subgraph_entries_are_in_the_abi_table():
    from seqwin_amd._abi import PROTOTYPES
    for name in ("sw_index_from_arrays", "sw_index_subgraph_seeds", "sw_index_subgraphs", "sw_subgraphs_sizes", "sw_subgraphs_export",
                 "sw_subgraphs_stats", "sw_subgraphs_free", "sw_index_filter_kmers_sg"):
        assert name in PROTOTYPES, name
    from ctypes import c_double
    assert PROTOTYPES["sw_index_subgraphs"][1][1] is c_double and PROTOTYPES["sw_index_subgraph_seeds"][1][1] is c_double


def test_subgraph_hooks_are_test_only():
    rel, tst = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    assert rel.exists() and tst.exists()
    blob_rel, blob_tst = rel.read_bytes(), tst.read_bytes()
    for h in (b"SEQWIN_AMD_SG_WINDOW\0", b"SEQWIN_AMD_SG_LDS_CAP\0"):
        assert h not in blob_rel and h in blob_tst, h


def test_subgraph_calls_need_a_device_or_fail_cleanly():
    """Without a GPU the upload fails with the library's device error (no CPU fallback); with one, bad input is a ValueError."""
    from seqwin_amd._core import EDGE_DTYPE, NODE_DTYPE
    from seqwin_amd.device import Index
    nodes = np.zeros(2, NODE_DTYPE)
    nodes["hash"] = [5, 3]   # not ascending
    with pytest.raises(ValueError):
        Index.from_arrays(nodes, np.zeros(0, EDGE_DTYPE))


# ---- adversarial shapes (tests/tools/sg_shapes.py, goldens from tests/golden/make_golden_subgraph_shapes.py) ----------------------
import sg_shapes as S  # noqa: E402

SHAPES = S.load_golden(GOLDEN)


def _shape_result(fn, nodes, edges, case, **kw):
    """(canonical CSR digest or the error text, rng.random() afterwards) of one walk."""
    rng = random.Random(case["seed"])
    try:
        sgs = fn(nodes, edges, case["penalty_th"], case["min_nodes"], case["max_nodes"], rng, **kw)[0]
        got = S.csr_digest(*S.canonical_csr(sgs))
    except RuntimeError as e:
        got = str(e)
    return got, rng.random()


def test_shape_generator_reproduces_the_recorded_digests():
    ids = [g["id"] for g, _, _, _ in SHAPES]
    assert ids == [gid for gid, _, _, _, _ in S.cases()] and len(set(ids)) == len(ids)
    for g, nodes, edges, _ in SHAPES:
        assert S.digest(nodes, edges) == g["sha256"], g["id"]
        assert len(nodes) == g["n_nodes"] and len(edges) == g["n_edges"]
        assert np.all(nodes["hash"][1:] > nodes["hash"][:-1]) and np.all(edges["weight"] >= 1)
        assert np.all(nodes["penalty"] >= 0.0)   # -0.0 included: what from_arrays accepts


def test_shape_goldens_reach_the_bounds():
    by = {}
    for g, nodes, edges, cases in SHAPES:
        by.setdefault(g["family"], []).append((g, nodes, edges, [c for c, _ in cases]))
    assert {g["params"]["deg"] for g, *_ in by["star"]} >= {1023, 1024, 1025, 1087, 2048}
    assert {g["params"].get("deg2", 0) for g, *_ in by["star"]} >= {25, 26}
    (lg, _, _, lcases), = by["long"]
    assert {c["max_nodes"] for c in lcases} >= {None, 128, 129, 1000}
    assert max(c["max_size"] for c in lcases if c["max_nodes"] is None) == 130
    (mg, _, _, mcases), = by["many_seeds"]
    assert mcases[0]["n_subgraphs"] >= 100_000
    (dg, _, _, _), = by["dense"]
    assert dg["n_nodes"] >= 200_000
    (tg, tnodes, tedges, _), = by["ties"]
    h = tnodes["hash"]
    assert h[0] == 0 and h[-1] == S.U64_MAX and np.sum(h >= np.uint64(1 << 63)) > 100
    p = tnodes["penalty"]
    zero = p == 0.0
    assert np.any(np.signbit(p) & zero) and np.any(~np.signbit(p) & zero)
    (eg, _, _, ecases), = by["rounding_edge"]
    assert any(c["penalty_th"] < 0 and c["error"] for c in ecases)
    (pg, pnodes, pedges, _), = by["dropin"]
    assert np.any(pedges["first"] > pedges["second"]) and np.any(pedges["first"] == pedges["second"])
    pairs = np.sort(np.stack([pedges["first"], pedges["second"]], 1), 1)
    assert len(np.unique(pairs, axis=0)) < len(pedges)
    assert len(np.setdiff1d(pnodes["hash"], np.concatenate([pedges["first"], pedges["second"]]))) > 0
    assert sum(p.stat().st_size for p in (GOLDEN / "subgraphs").glob("shapes*")) <= 150_000


@pytest.mark.parametrize("gi", range(len(SHAPES)), ids=[g["id"] for g, _, _, _ in SHAPES])
def test_restatement_reproduces_the_shape_goldens(gi):
    g, nodes, edges, cases = SHAPES[gi]
    for case, exp in cases:
        got, after = _shape_result(lambda *a: H.get_subgraphs(*a)[:2], nodes, edges, case)
        assert got == (case["error"] or case["csr_sha256"]), case
        assert after == case["rng_after"], case
        if exp is not None:
            rng = random.Random(case["seed"])
            sgs, used, _ = H.get_subgraphs(nodes, edges, case["penalty_th"], case["min_nodes"], case["max_nodes"], rng)
            assert sgs == H.csr_to_sets(*exp) and len(used) == case["n_used"]


@pytest.mark.parametrize("gi", [i for i, (g, _, _, _) in enumerate(SHAPES) if g["n_nodes"] <= 20_000],
                         ids=[g["id"] for g, _, _, _ in SHAPES if g["n_nodes"] <= 20_000])
def test_heap_restatement_agrees_on_the_smaller_shapes(gi):
    """A second restatement (heap, goes on after a rejection, ties by hash) gives the recorded result too."""
    g, nodes, edges, cases = SHAPES[gi]
    for case, _ in cases:
        got, after = _shape_result(S.walk_heap, nodes, edges, case)
        assert got == (case["csr_sha256"] if case["error"] is None else "No low-penalty subgraph was found."), case
        assert after == case["rng_after"], case


def test_rounding_cases_are_sensitive():
    """Every rounding case changes its result under at least one wrong arithmetic, and each wrong arithmetic is caught somewhere."""
    caught = set()
    for g, nodes, edges, cases in SHAPES:
        if g["family"] != "rounding":
            continue
        for case, _ in cases:
            want = _shape_result(S.walk_heap, nodes, edges, case)
            assert want[0] == case["csr_sha256"]
            diff = {w for w in S.WRONG if _shape_result(S.walk_heap, nodes, edges, case, arith=w) != want}
            assert diff, (g["id"], case)
            caught |= diff
    assert caught == set(S.WRONG)
