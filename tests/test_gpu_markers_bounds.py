"""The marker step on the device at the sizes where its kernels change behaviour (tests/tools/marker_cases.py: bounds(), pinned
by tests/test_markers_bounds_cpu.py): a second chunk of 64 items in k_loc's run cut and gather, the LDS bound of 384 items, a
second row per thread in k_vote, its LDS bound of 1 536 target rows, the 32-bit edges of positions, window and record indices,
and empty shapes.  Every table is compared exactly with the host restatement (tests/tools/markers_host.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import marker_cases as C  # noqa: E402
import markers_host as M  # noqa: E402
from test_gpu_markers import CASES, HOOKS, _args, _equal, _resident, _tables  # noqa: E402

pytestmark = pytest.mark.gpu
BOUNDS = C.bounds()
NAMES = [c["name"] for c in BOUNDS]
EMPTY = ("no_subgraphs", "no_occurrences")
WANT, COUNTS = {}, {}
# the lowered bounds: the chunk of k_loc and the block of k_vote as LDS bounds, and one above; narrowed fingerprints
LOWERED = ({"SEQWIN_AMD_LOC_LDS_CAP": "64", "SEQWIN_AMD_LOC_VOTE_CAP": "256"}, {"SEQWIN_AMD_LOC_LDS_CAP": "65", "SEQWIN_AMD_LOC_VOTE_CAP": "257"},
           {"SEQWIN_AMD_LOC_FP_BITS": "0"}, {"SEQWIN_AMD_LOC_FP_BITS": "1"}, {"SEQWIN_AMD_LOC_FP_BITS": "3"})
SWEEP_LOWERED = {"SEQWIN_AMD_LOC_LDS_CAP": "8", "SEQWIN_AMD_LOC_VOTE_CAP": "3", "SEQWIN_AMD_LOC_FP_BITS": "2"}


def _want(case):
    if case["name"] not in WANT:
        WANT[case["name"]] = M.tables(M.markers(**_args(case)))
        COUNTS[case["name"]] = C.pair_counts(case)
    return WANT[case["name"]]


def _want_stats(case, env):
    """The counters of a call, counted from the case: non-empty pairs, pairs above the LDS bound, the largest pair, subgraphs
    with more target rows than the vote's bound."""
    _want(case)
    cnt = COUNTS[case["name"]]
    loc_cap = int(env.get("SEQWIN_AMD_LOC_LDS_CAP", C.LOC_CAP))
    vote_cap = int(env.get("SEQWIN_AMD_LOC_VOTE_CAP", C.VOTE_CAP))
    return dict(pairs=int((cnt > 0).sum()), spilled=int((cnt > loc_cap).sum()), largest_pair=int(cnt.max()) if cnt.size else 0,
                vote_spilled=int(((cnt[:, :case["n_tar"]] > 0).sum(axis=1) > vote_cap).sum()))


def _run(case, env, monkeypatch):
    from seqwin_amd.device import Markers
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = Markers.from_arrays(**_args(case), keep_rows=True)
    try:
        _equal(_tables(m), _want(case))
        st = m.stats()
        assert {k: st[k] for k in ("pairs", "spilled", "largest_pair", "vote_spilled")} == _want_stats(case, env), (case["name"], env)
    finally:
        m.close()


@pytest.mark.parametrize("ci", range(len(BOUNDS)), ids=NAMES)
def test_bounds_at_the_default_bounds(ci, monkeypatch):
    case = BOUNDS[ci]
    _run(case, {}, monkeypatch)
    want = _want_stats(case, {})
    spills = {"pair_n385": (2, 0), "pair_n1000": (2, 0), "three_subgraphs_mixed": (4, 0), "vote_T1537": (0, 1), "vote_all_equal_1537": (0, 1),
              "vote_non_targets_after_1537": (0, 1), "two_votes_mixed": (0, 2)}
    assert (want["spilled"], want["vote_spilled"]) == spills.get(case["name"], (0, 0))   # 384 items and 1 536 rows stay in LDS


@pytest.mark.parametrize("ci", range(len(BOUNDS)), ids=NAMES)
def test_bounds_with_the_bounds_lowered_and_the_fingerprint_narrowed(ci, monkeypatch):
    """The same tables with k_loc's chunk and k_vote's block as the LDS bounds (64 / 256), one above them (65 / 257), and with
    fingerprints of 0, 1 and 3 bits.  Cases of more than 600 rows take the first setting only: with a narrow fingerprint the
    leader search is quadratic in the rows of one fingerprint class."""
    case = BOUNDS[ci]
    rows = len(_want(case)["rows"])
    for env in LOWERED if rows <= 600 else LOWERED[:1]:
        _run(case, env, monkeypatch)


@pytest.mark.parametrize("name", EMPTY)
def test_empty_shapes_return_empty_tables(name, monkeypatch):
    from seqwin_amd.device import MARKER_REP_DTYPE, MARKER_ROW_DTYPE, Markers
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    case = BOUNDS[NAMES.index(name)]
    for keep in (True, False):
        m = Markers.from_arrays(**_args(case), keep_rows=keep)
        assert m.sizes() == (0, 0, 0, 0)
        reps, offs, hashes = m.reps()
        assert reps.dtype == MARKER_REP_DTYPE and reps.shape == (0,)
        assert offs.dtype == np.uint64 and offs.tolist() == [0] and hashes.dtype == np.uint64 and hashes.shape == (0,)
        assert m.candidates(0).shape == (0,)
        if keep:
            assert m.rows() == []
            t = _tables(m)
            assert t["rows"].dtype == MARKER_ROW_DTYPE and t["rows"].shape == (0,) and t["row_offsets"].tolist() == [0]
        st = m.stats()
        assert (st["pairs"], st["spilled"], st["largest_pair"], st["vote_spilled"]) == (0, 0, 0, 0)
        m.close()


def test_a_node_without_occurrences_is_skipped(monkeypatch):
    from seqwin_amd.device import Markers
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    case = BOUNDS[NAMES.index("node_without_occurrences")]
    m = Markers.from_arrays(**_args(case), keep_rows=True)
    t = _tables(m)
    _equal(t, _want(case))
    assert t["rows"]["n_kmers"].tolist() == [2, 2] and t["reps"]["n_rep"].tolist() == [2]
    m.close()


def test_the_golden_with_the_large_pair_under_other_votes():
    """The kept index and the subgraphs of pan_a_k15_w20 (the one fixture with a pair of about a hundred items), exported from the
    resident route, through the direct route with 1, 7 and all 12 assemblies as targets -- votes the golden does not record."""
    from seqwin_amd.device import Markers
    c = next(x for x in CASES if x["graph"] == "pan_a_k15_w20")
    g, b, sg, kept = _resident(c)
    kmers, nodes, _ = kept.export()
    sg_off, sg_hashes = sg.csr()
    sg_nodes = np.searchsorted(nodes["hash"], sg_hashes).astype(np.uint64)
    assert np.array_equal(nodes["hash"][sg_nodes.astype(np.int64)], sg_hashes)
    ro = b.record_offsets()
    assert len(ro) - 1 == 12 and len(sg_off) - 1 == c["n_subgraphs"]
    for n_tar in (1, 7, 12):
        res = M.markers(kmers, nodes, sg_off, sg_nodes, ro, n_tar, g["k"], g["w"])
        has = [i for i, r in enumerate(res) if int(r["rep"]["flags"]) != M.NO_TARGET]
        off, nd = sg_off, sg_nodes
        if len(has) < len(res):   # a subgraph that lies in no target is a ValueError, as in the reference: the others are compared
            with pytest.raises(ValueError, match="no target"):
                Markers.from_arrays(kmers, nodes, sg_off, sg_nodes, ro, n_tar, g["k"], g["w"])
            o = sg_off.astype(np.int64)
            nd = np.concatenate([sg_nodes[o[i]:o[i + 1]] for i in has])
            off = np.concatenate([[0], np.cumsum([o[i + 1] - o[i] for i in has])]).astype(np.uint64)
        assert (len(has) == len(res)) == (n_tar >= 7) and len(has) > 20
        m = Markers.from_arrays(kmers, nodes, off, nd, ro, n_tar, g["k"], g["w"], keep_rows=True)
        want = M.tables([res[i] for i in has])
        _equal(_tables(m), want)
        assert m.stats()["pairs"] == len(want["rows"])
        if n_tar == c["n_tar"]:
            _equal(_tables(m), np.load(ROOT / "tests" / "golden" / "markers" / f"{c['graph']}_c{c['case']}.npz"))
        m.close()


@pytest.mark.parametrize("seed", C.SWEEP_SEEDS)
def test_seeded_sweep(seed, monkeypatch):
    """Small random kept indexes (marker_cases.sweep) at the default bounds and with every bound lowered."""
    case = C.sweep(seed)
    for env in ({}, SWEEP_LOWERED):
        _run(case, env, monkeypatch)
