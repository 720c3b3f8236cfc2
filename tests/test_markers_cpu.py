"""The marker step without a GPU: the host restatement (tests/tools/markers_host.py) against goldens recorded from the
reference's markers._create_ck (tests/golden/make_golden_markers.py) and, where the reference tree is present, against the live
reference on the crafted cases (tests/tools/marker_cases.py); the new C-ABI entries."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import marker_cases as C  # noqa: E402
import markers_host as M  # noqa: E402
import subgraphs_host as H  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
CASES = json.loads((GOLDEN / "markers" / "manifest.json").read_text())["cases"]
GRAPHS = {g["name"]: (g, fnodes, cases) for g, fnodes, _, cases in H.load_golden(GOLDEN)}
CRAFTED = C.cases()
TABLES = ("reps", "rep_offsets", "rep_hashes", "row_offsets", "rows", "kmer_offsets", "row_hashes")


def assert_tables_equal(got, want):
    for name in TABLES:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape, name
        if a.dtype.names:
            for f in a.dtype.names:
                assert np.array_equal(a[f].astype(np.int64), b[f].astype(np.int64)), (name, f)
        else:
            assert np.array_equal(a.astype(np.uint64), b.astype(np.uint64)), name


def test_goldens_cover_the_four_fixtures():
    assert {c["graph"] for c in CASES} == {"smoke_k17_w10", "pan_a_k15_w20", "pan_b_k21_w10", "synth_pan_k15_w20"}
    assert all(c["error"] is None for c in CASES)
    assert sum(p.stat().st_size for p in (GOLDEN / "markers").iterdir()) < 200_000


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[f"{c['graph']}_c{c['case']}" for c in CASES])
def test_restatement_reproduces_the_reference(ci):
    import oracle
    c = CASES[ci]
    g, fnodes, cases = GRAPHS[c["graph"]]
    _, (sg_off, sg_hashes) = cases[c["case"]]
    kmers, nodes, _, offs, _ = oracle.build([GOLDEN / p for p in g["paths"]], g["k"], g["w"])
    kk, kn, sg_nodes = M.resident_inputs(kmers, nodes, fnodes, sg_off, sg_hashes)
    res = M.markers(kk, kn, sg_off, sg_nodes, offs, c["n_tar"], g["k"], g["w"])
    assert len(res) == c["n_subgraphs"]
    assert_tables_equal(M.tables(res), np.load(GOLDEN / "markers" / f"{c['graph']}_c{c['case']}.npz"))


def _reference():
    """The reference's markers module, or None where its tree or its compiled extension is not around."""
    import oracle
    ref = Path("/root/reference/src")
    core = oracle.load_ref() if ref.is_dir() else None
    if core is None:
        return None
    sys.modules.setdefault("seqwin.graph._core", core)
    if str(ref) not in sys.path:
        sys.path.insert(0, str(ref))
    import logging
    logging.disable(logging.CRITICAL)
    from seqwin import markers
    return markers


def _by_reference(ref, case):
    import networkx as nx
    CK = ref.ConnectedKmers
    seen = {}
    loc0, rep0 = CK._ConnectedKmers__get_loc, CK._ConnectedKmers__get_rep_order
    CK._ConnectedKmers__get_loc = staticmethod(lambda *a: seen.__setitem__("loc", loc0(*a)) or seen["loc"])
    CK._ConnectedKmers__get_rep_order = staticmethod(lambda *a: seen.__setitem__("rep", rep0(*a)) or seen["rep"])
    try:
        out = []
        so = case["sg_offsets"].astype(np.int64)
        for s in range(len(so) - 1):
            nd = case["nodes"][case["sg_nodes"][so[s]:so[s + 1]].astype(np.int64)]
            ck = ref._create_ck(nx.Graph(), tuple(nd["hash"]), tuple(case["kmers"][int(n["start"]):int(n["stop"])] for n in nd),
                                case["record_offsets"], case["n_tar"], case["kmerlen"], case["windowsize"])
            loc, (order, n_rep) = seen["loc"], seen["rep"]
            rows = np.zeros(len(loc), M.ROW_DTYPE)
            for f in M.ROW_DTYPE.names:
                rows[f] = loc[f].to_numpy().astype(np.int64)
            rep = np.zeros((), M.REP_DTYPE)
            for f in M.ROW_DTYPE.names:
                rep[f] = int(ck.rep[f])
            rep["n_rep"] = n_rep
            rep["flags"] = (M.SINGLE if "single" in ck.warnings else 0) | (M.DUP if "dup" in ck.warnings else 0)
            out.append(dict(rows=rows, seqs=[tuple(int(x) for x in t) for t in loc["kmers"]], rep=rep, order=tuple(int(x) for x in order)))
        return out
    finally:
        CK._ConnectedKmers__get_loc, CK._ConnectedKmers__get_rep_order = staticmethod(loc0), staticmethod(rep0)


@pytest.mark.parametrize("ci", range(len(CRAFTED)), ids=[c["name"] for c in CRAFTED])
def test_restatement_equals_the_live_reference_on_the_crafted_cases(ci):
    ref = _reference()
    if ref is None:
        pytest.skip("the reference tree is not present")
    case = CRAFTED[ci]
    args = {k: v for k, v in case.items() if k != "name"}
    assert_tables_equal(M.tables(M.markers(**args)), M.tables(_by_reference(ref, case)))


def test_no_target_row_is_a_value_error_in_the_reference_and_a_flag_here():
    case = C.no_target_case()
    res = M.markers(**{k: v for k, v in case.items() if k != "name"})
    assert int(res[0]["rep"]["flags"]) == M.NO_TARGET and int(res[0]["rep"]["n_rep"]) == 0 and len(res[0]["rows"]) == 2
    ref = _reference()
    if ref is not None:
        with pytest.raises(ValueError):
            _by_reference(ref, case)


def test_crafted_cases_reach_their_branches():
    by = {c["name"]: M.markers(**{k: v for k, v in c.items() if k != "name"}) for c in CRAFTED}
    row = lambda n, s=0, i=0: by[n][s]["rows"][i]   # noqa: E731
    assert (row("gap_even_w10")["n_kmers"], row("gap_even_w10")["n_repeats"]) == (2, 2)
    assert (row("gap_odd_w11")["n_kmers"], row("gap_odd_w11")["n_repeats"]) == (2, 2)
    assert (row("gap_w1")["n_kmers"], row("gap_w1")["start"], row("gap_w1")["n_repeats"]) == (3, 3, 2)
    assert row("gap_w_huge")["n_repeats"] == 1 and row("gap_w_huge")["stop"] == (1 << 31) + 10
    assert [int(x) for x in by["records"][0]["rows"]["record_idx"]] == [0, 1, 1] and row("records")["n_repeats"] == 4
    r = by["repeats"][0]["rows"]
    assert [int(x) for x in r["assembly_idx"]] == [0, 1, 3, 4] and [int(x) for x in r["start"]] == [0, 400, 0, 9]
    assert [int(x) for x in r["n_repeats"]] == [2, 3, 1, 1]
    assert {len(by[n][0]["rows"]) > 40 for n in ("asm63", "asm64", "asm65")} == {True}
    flags = lambda n: int(by[n][0]["rep"]["flags"])   # noqa: E731
    assert flags("dup") & M.DUP and flags("single") == M.SINGLE and flags("palindrome") & M.DUP
    assert int(by["rep_row_is_a_later_target"][0]["rep"]["assembly_idx"]) == 2
    assert int(by["big_pair"][0]["rows"]["n_kmers"][0]) == 11


def test_marker_entries_are_in_the_abi_table():
    from seqwin_amd._abi import PROTOTYPES
    for name in ("sw_index_marker_locs", "sw_marker_locs_from_arrays", "sw_markers_sizes", "sw_markers_export", "sw_markers_export_rows",
                 "sw_markers_stats", "sw_markers_free"):
        assert name in PROTOTYPES, name
    from seqwin_amd.device import MARKER_REP_DTYPE, MARKER_ROW_DTYPE
    assert MARKER_ROW_DTYPE.itemsize == 24 and MARKER_REP_DTYPE.itemsize == 32
    assert MARKER_ROW_DTYPE == M.ROW_DTYPE and MARKER_REP_DTYPE == M.REP_DTYPE


def test_marker_hooks_are_test_only():
    rel, tst = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    assert rel.exists() and tst.exists()
    blob_rel, blob_tst = rel.read_bytes(), tst.read_bytes()
    for h in (b"SEQWIN_AMD_LOC_LDS_CAP\0", b"SEQWIN_AMD_LOC_VOTE_CAP\0", b"SEQWIN_AMD_LOC_FP_BITS\0"):
        assert h not in blob_rel and h in blob_tst, h


def test_arguments_are_checked_before_a_device_is_touched():
    from seqwin_amd.device import Markers
    c = {k: v for k, v in CRAFTED[0].items() if k != "name"}
    with pytest.raises(ValueError, match="n_tar"):
        Markers.from_arrays(**{**c, "n_tar": 2})
    with pytest.raises(ValueError, match="windowsize"):
        Markers.from_arrays(**{**c, "windowsize": 0})
    with pytest.raises(ValueError, match="non-decreasing"):
        Markers.from_arrays(**{**c, "record_offsets": np.array([1, 0], np.uint32)})
