"""The marker step on the device (csrc/markers.hip: Index.marker_locs, Markers.from_arrays, markers.get_cks) against the goldens
recorded from the reference's markers._create_ck (tests/golden/markers/) through the resident route, and against the host
restatement (tests/tools/markers_host.py) through the direct route on the crafted cases (tests/tools/marker_cases.py)."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import marker_cases as C  # noqa: E402
import markers_host as M  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
CASES = json.loads((GOLDEN / "markers" / "manifest.json").read_text())["cases"]
SUB = {g["name"]: g for g in json.loads((GOLDEN / "subgraphs" / "manifest.json").read_text())["graphs"]}
CRAFTED = C.cases()
WANT = {}
HOOKS = ("SEQWIN_AMD_LOC_LDS_CAP", "SEQWIN_AMD_LOC_VOTE_CAP", "SEQWIN_AMD_LOC_FP_BITS")


def _args(case):
    return {k: v for k, v in case.items() if k != "name"}


def _want(case):
    """The restatement's tables of a crafted case, computed once."""
    if case["name"] not in WANT:
        WANT[case["name"]] = M.tables(M.markers(**_args(case)))
    return WANT[case["name"]]


def _tables(m, rows=True):
    reps, ro, rh = m.reps()
    out = dict(reps=reps, rep_offsets=ro, rep_hashes=rh)
    if rows:
        per = m.rows()
        out["rows"] = np.concatenate([r for r, _, _ in per]) if per else np.zeros(0, M.ROW_DTYPE)
        out["row_offsets"] = np.concatenate([[0], np.cumsum([len(r) for r, _, _ in per])]).astype(np.uint64)
        out["row_hashes"] = np.concatenate([h for _, _, h in per]) if per else np.zeros(0, np.uint64)
        lens = [np.diff(o.astype(np.int64)) for _, o, _ in per]
        out["kmer_offsets"] = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.uint64) if per else np.zeros(1, np.uint64)
    return out


def _equal(got, want):
    for name, a in got.items():
        b = np.asarray(want[name])
        assert a.shape == b.shape, name
        if a.dtype.names:
            for f in a.dtype.names:
                assert np.array_equal(a[f].astype(np.int64), b[f].astype(np.int64)), (name, f, a[f], b[f])
        else:
            assert np.array_equal(a.astype(np.uint64), b.astype(np.uint64)), name


def _resident(c):
    from seqwin_amd.device import Batch
    g = SUB[c["graph"]]
    case = g["cases"][c["case"]]
    b = Batch.from_fasta([GOLDEN / p for p in g["paths"]])
    ix = b.build_index(g["k"], g["w"], g["is_targets"])
    f = ix.filter_graph(g["edge_weight_th"])
    sg = f.subgraphs(case["penalty_th"], case["min_nodes"], case["max_nodes"], random.Random(case["seed"]))
    return g, b, sg, ix.filter_kmers(f, sg)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[f"{c['graph']}_c{c['case']}" for c in CASES])
def test_golden_through_the_resident_route(ci):
    c = CASES[ci]
    g, b, sg, kept = _resident(c)
    m = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"], keep_rows=True)
    assert m.sizes()[0] == c["n_subgraphs"] and m.sizes()[2] == c["n_rows"] == m.stats()["pairs"]
    _equal(_tables(m), np.load(GOLDEN / "markers" / f"{c['graph']}_c{c['case']}.npz"))
    m.close()


@pytest.mark.parametrize("ci", range(len(CRAFTED)), ids=[c["name"] for c in CRAFTED])
def test_crafted_through_the_direct_route(ci, monkeypatch):
    """Every crafted case with the default bounds, and with the LDS bounds and the fingerprint narrowed so that the same small
    input sorts its pairs and votes in the HBM scratch and meets fingerprint collisions: the same tables every time."""
    from seqwin_amd.device import Markers
    case = CRAFTED[ci]
    for env in ({}, {"SEQWIN_AMD_LOC_LDS_CAP": "1", "SEQWIN_AMD_LOC_VOTE_CAP": "1", "SEQWIN_AMD_LOC_FP_BITS": "1"},
                {"SEQWIN_AMD_LOC_LDS_CAP": "8", "SEQWIN_AMD_LOC_VOTE_CAP": "3", "SEQWIN_AMD_LOC_FP_BITS": "0"}):
        for k in HOOKS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        m = Markers.from_arrays(**_args(case), keep_rows=True)
        _equal(_tables(m), _want(case))
        st = m.stats()
        assert st["pairs"] == len(_want(case)["rows"])
        if not env:
            assert st["spilled"] == 0 and st["vote_spilled"] == 0
        m.close()


def test_a_pair_above_the_lds_bound_takes_the_spill(monkeypatch):
    from seqwin_amd.device import Markers
    case = next(c for c in CRAFTED if c["name"] == "big_pair")
    monkeypatch.setenv("SEQWIN_AMD_LOC_LDS_CAP", "8")
    m = Markers.from_arrays(**_args(case), keep_rows=True)
    _equal(_tables(m), _want(case))
    st = m.stats()
    assert st["spilled"] == 1 and st["largest_pair"] == 22, st   # the pair of 22 items; the one of 3 stays in LDS
    monkeypatch.delenv("SEQWIN_AMD_LOC_LDS_CAP")
    m2 = Markers.from_arrays(**_args(case), keep_rows=True)
    _equal(_tables(m2), _want(case))
    assert m2.stats()["spilled"] == 0


def test_no_target_row_raises_value_error():
    from seqwin_amd.device import Markers
    with pytest.raises(ValueError, match="no target"):
        Markers.from_arrays(**_args(C.no_target_case()))
    two = C.build("mixed", [C.at([0, 1], 0), C.at([0, 1], 1)], [0, 1, 2], 1)   # the second subgraph lies in the non-target only
    with pytest.raises(ValueError, match="subgraph 1"):
        Markers.from_arrays(**_args(two))


def test_the_final_order_is_applied_to_every_table():
    from seqwin_amd.device import Markers
    case = C.many_assemblies(9, 7)
    extra = C.build("x", [C.at([0, 1, 2], 0), C.at([0, 1], 1) + C.at([1, 0], 2), C.at([0], 0, 900) + C.at([0], 3)], [0, 1, 2, 3, 4], 4)
    for case, order in ((case, [1, 0]), (extra, [2, 0, 1])):
        res = M.markers(**_args(case))
        want = M.tables([res[i] for i in order])
        m = Markers.from_arrays(**_args(case), keep_rows=True, order=order)
        _equal(_tables(m), want)
        assert not np.array_equal(want["reps"], M.tables(res)["reps"])
        with pytest.raises(ValueError):
            Markers.from_arrays(**_args(case), order=order[:-1])


def test_rows_are_opt_in():
    from seqwin_amd.device import Markers
    case = CRAFTED[-1]
    m = Markers.from_arrays(**_args(case))
    with pytest.raises(ValueError, match="keep_rows"):
        m.rows()
    _equal(_tables(m, rows=False), {k: _want(case)[k] for k in ("reps", "rep_offsets", "rep_hashes")})
    assert m.sizes()[3] == 0 and m.sizes()[2] == len(_want(case)["rows"])


def test_argument_checks():
    from seqwin_amd.device import Markers
    c = _args(CRAFTED[4])   # "records": three assemblies, eight records
    for bad in (dict(n_tar=4), dict(windowsize=0), dict(record_offsets=np.array([0, 6, 4, 8], np.uint32)),
                dict(record_offsets=np.array([0, 4, 6, 7], np.uint32)),    # record 7 is not covered
                dict(record_offsets=np.array([1, 4, 6, 8], np.uint32)),    # record 0 is not covered
                dict(sg_nodes=c["sg_nodes"] + np.uint64(1)),               # no such node
                dict(sg_offsets=np.array([0, 3, 2, len(c["sg_nodes"])], np.uint64)),
                dict(kmers=c["kmers"][::-1].copy())):                      # occurrences of a node not ascending
        with pytest.raises(ValueError):
            Markers.from_arrays(**{**c, **bad})
    nodes = c["nodes"].copy()
    nodes["stop"][-1] += 1
    with pytest.raises(ValueError):
        Markers.from_arrays(**{**c, "nodes": nodes})
    nodes = c["nodes"][::-1].copy()
    with pytest.raises(ValueError):
        Markers.from_arrays(**{**c, "nodes": nodes})


def test_argument_checks_of_the_resident_route():
    c = CASES[0]
    g, b, sg, kept = _resident(c)
    ro = b.record_offsets()
    args = (c["n_tar"], g["k"], g["w"])
    hi = int(kept.export()[0]["record_idx"].max())   # the last record that holds a kept occurrence
    for bad_ro in (ro[:0], ro[ro <= hi], np.concatenate([[1], ro[1:]]).astype(np.uint32), ro[::-1].copy()):
        with pytest.raises(ValueError):   # empty / that record not covered / record 0 not covered / decreasing
            kept.marker_locs(sg, bad_ro, 1, g["k"], g["w"])
    with pytest.raises(ValueError, match="n_tar"):
        kept.marker_locs(sg, ro, len(ro), g["k"], g["w"])
    with pytest.raises(ValueError, match="windowsize"):
        kept.marker_locs(sg, ro, c["n_tar"], g["k"], 0)
    ix = b.build_index(g["k"], g["w"], g["is_targets"])
    fewer = ix.filter_kmers(ix, sg.used_hashes()[1:])   # an index that lacks one subgraph node
    with pytest.raises(ValueError, match="not among"):
        fewer.marker_locs(sg, ro, *args)
    kept.marker_locs(sg, ro, *args).close()   # and the call itself is fine


def test_get_cks_returns_the_candidates_with_the_reference_fields():
    import pandas as pd
    from seqwin_amd import markers
    c = next(x for x in CASES if x["graph"] == "pan_a_k15_w20")
    g, b, sg, kept = _resident(c)
    z = np.load(GOLDEN / "markers" / f"{c['graph']}_c{c['case']}.npz")
    reps = z["reps"]
    length = (reps["stop"] - reps["start"]).astype(np.uint32)
    min_len = int(np.median(length))
    keep = np.flatnonzero((length >= min_len) & ((reps["flags"] & 3) == 0))
    cks = markers.get_cks(kept, sg, b.record_offsets(), c["n_tar"], g["k"], g["w"], min_len)
    assert 0 < len(cks) == len(keep) < len(reps)
    o = z["rep_offsets"].astype(np.int64)
    for ck, i in zip(cks, keep):
        assert isinstance(ck.rep, pd.Series)
        assert list(ck.rep.index) == ["assembly_idx", "record_idx", "start", "stop", "n_kmers", "kmers", "is_target", "n_repeats", "len", "seq"]
        assert ck.rep["kmers"] == tuple(z["rep_hashes"][o[i]:o[i + 1]]) and all(type(x) is np.uint64 for x in ck.rep["kmers"])
        assert int(ck.len) == int(length[i]) and ck.n_rep == int(reps["n_rep"][i]) and ck.rep_ratio == ck.n_rep / c["n_tar"]
        assert ck.rep["seq"] is None and ck.blast is None and ck.path is None and not ck.is_bad and ck.rep["is_target"]
        assert ck.metrics.conservation is None and ck.metrics.avg_pident_neg is None and ck.warnings == set()
        assert ck.graph is None and ck.kmers is None and ck.loc is None
        assert set(vars(ck)) == {"graph", "kmers", "loc", "path", "rep", "len", "n_rep", "blast", "metrics", "rep_ratio", "warnings", "is_bad"}
    m = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"])
    assert np.array_equal(m.candidates(min_len), keep)
