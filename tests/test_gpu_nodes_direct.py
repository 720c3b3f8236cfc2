"""GPU (-m gpu): the node stage (csrc/index.hip: group_occurrences = the pair sort, k_nodes<BITS, REP, SCAT>, one of five unsort
routes, k_finish_nodes<BITS>) driven directly through sw_slice_build on crafted rows, against a plain NumPy restatement.

tests/tools/nodes_host.py builds every case layout-first -- runs of equal hashes placed on k_nodes' lane (2 occurrences), wave row
(128), bitmap word (64), row (2048), tile (8192) and look-back (64 tiles) bounds, with the assembly of every occurrence chosen --
and tests/test_nodes_host_cpu.py checks those layouts and the restatement (against the oracle) on the host.  Here every case
compares ALL of kmers, the six node fields (the penalty bit for bit) and every rank word (bit 31, the repeat mark, included) by
equality, asserts the route and a silent order guard from the [nodes] line, and that the ranks are marked."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import nodes_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

# switches that choose a path of the stage: none of them may leak in from the caller's environment
HOOKS = ("SEQWIN_AMD_UNSORT_DIRECT", "SEQWIN_AMD_UNSORT_FUSED", "SEQWIN_AMD_SORT", "SEQWIN_AMD_PAIR_SORT", "SEQWIN_AMD_CHECK_ORDER",
         "SEQWIN_AMD_ORDER", "SEQWIN_AMD_SORT_KEYBITS", "SEQWIN_AMD_ADJ_SEPARATE", "SEQWIN_AMD_FAULT_INJECT", "SEQWIN_AMD_RADIX_RANK")
ROUTES = {   # name -> (the route the [nodes] line must name, the switches that lead there at the case's size)
    "direct": ("direct", {}),
    "one_bucket": ("one bucket", {"SEQWIN_AMD_UNSORT_DIRECT": "0"}),
    "sort_rocprim": ("sort", {"SEQWIN_AMD_SORT": "rocprim", "SEQWIN_AMD_PAIR_SORT": "rocprim", "SEQWIN_AMD_UNSORT_DIRECT": "0"}),
    "sort_own": ("sort", {"SEQWIN_AMD_SORT": "own", "SEQWIN_AMD_PAIR_SORT": "own", "SEQWIN_AMD_UNSORT_DIRECT": "0"}),
    "two_passes": ("two passes", {"SEQWIN_AMD_SORT": "own", "SEQWIN_AMD_UNSORT_DIRECT": "0", "SEQWIN_AMD_UNSORT_FUSED": "0"}),
    "fused": ("fused", {"SEQWIN_AMD_SORT": "own", "SEQWIN_AMD_UNSORT_DIRECT": "0", "SEQWIN_AMD_UNSORT_FUSED": "1"}),
}
_REF = {}


def _ref(name):
    """reference() of a case, computed once per process."""
    if name not in _REF:
        c = H.case(name)
        _REF[name] = H.reference(c.rows, c.kmer_base, c.record_offsets, c.is_targets)
    return _REF[name]


def _engine():
    import seqwin_amd.dist as swdist
    return swdist.HipEngine()


def _check(name, route, monkeypatch, capfd, eng=None):
    import torch
    c = H.case(name)
    want_k, want_n, want_r = _ref(name)
    want_route, env = ROUTES[route]
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SEQWIN_AMD_DEBUG_NODES", "1")
    eng = eng or _engine()
    assert c.n == 0 or int(c.rows[:, 1].max() >> np.uint64(32)) < int(c.record_offsets[-1])   # (every record is in the table)
    rows = torch.from_numpy(np.array(c.rows).view(np.int64)).to(eng.gpu)
    capfd.readouterr()
    ix, ranks = eng.slice_build(rows, c.kmer_base, c.record_offsets, c.is_targets)
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[nodes]")]
    try:
        if c.n == 0:
            assert lines == []
        else:
            assert len(lines) == 1, lines
            ln = lines[0]
            assert ln.split("unsort route ")[1].split(",")[0] == want_route, ln
            assert ln.startswith(f"[nodes] {c.n} occurrences ") and "attempt 0:" in ln and ln.endswith(", order guard 0"), ln
            assert f", {len(want_n)} nodes," in ln, ln
        K, N, E = eng.export(ix)
        got = ranks.cpu().numpy().view(np.uint32)
        assert len(E) == 0 and ix.sizes() == (c.n, len(want_n), 0)
        assert K.dtype == want_k.dtype and K.shape == want_k.shape
        assert np.array_equal(K["pos"], want_k["pos"]) and np.array_equal(K["record_idx"], want_k["record_idx"])
        assert N.dtype == want_n.dtype and N.shape == want_n.shape
        for f in ("hash", "start", "stop", "n_tar", "n_neg"):
            assert np.array_equal(N[f], want_n[f]), (name, route, f, _first_diff(N[f], want_n[f]))
        assert np.array_equal(N["penalty"].view(np.uint64), want_n["penalty"].view(np.uint64)), (name, route, "penalty")
        assert got.shape == want_r.shape
        assert np.array_equal(got & np.uint32(0x7FFFFFFF), want_r & np.uint32(0x7FFFFFFF)), (name, route, "node of a row",
                                                                                              _first_diff(got & np.uint32(0x7FFFFFFF), want_r & np.uint32(0x7FFFFFFF)))
        assert np.array_equal(got, want_r), (name, route, "repeat marks", _first_diff(got, want_r))
        assert eng.ranks_marked(ix)
    finally:
        ix.close()
    return want_n, want_r


def _first_diff(a, b):
    d = np.flatnonzero(a != b)
    return (len(d), int(d[0]), int(a[d[0]]), int(b[d[0]])) if len(d) else None


@pytest.mark.parametrize("n", (0,) + H.SIZES)
def test_sizes(n, monkeypatch, capfd):
    """Every n around a lane, a wave row, a row and a tile, odd and even (an odd n ends in a lane with one occurrence), and none."""
    _check(f"sizes_{n}", "direct", monkeypatch, capfd)


@pytest.mark.parametrize("variant", H.BOUNDARY_VARIANTS)
def test_run_boundaries(variant, monkeypatch, capfd):
    """Heads at, one before and one behind p = 64, 128, 2048, 8192, 2 x 8192, 4 x 8192 -- where the predecessor of an occurrence
    comes from another lane, by a reload, from another row or another tile --, each differing from its predecessor in the low
    half of the hash only; the hashes 0 and 2^64 - 1."""
    want_n, _ = _check(f"boundaries_{variant}", "direct", monkeypatch, capfd)
    assert int(want_n["hash"][0]) == 0 and int(want_n["hash"][-1]) == 2**64 - 1


@pytest.mark.parametrize("form", ("plain_even", "mirror_odd"))
def test_assembly_changes_on_the_reloaded_lanes(form, monkeypatch, capfd):
    """Inside long runs the assembly changes exactly at the multiples of 128 (lane 0 reloads the predecessor's record, lane 63 the
    successor's) -- or, mirrored, ONLY the pair across such a place is of one assembly: its two repeat marks and the missing
    first-of-assembly bit then come from the reloaded neighbour alone.  The last run ends at n - 1: s + 2 == n, s + 1 == n."""
    want_n, want_r = _check(f"asm_{form}", "direct", monkeypatch, capfd)
    assert (want_r >> np.uint32(31)).any() and not (want_r >> np.uint32(31)).all() and int(want_n["n_tar"].max()) >= 3


@pytest.mark.parametrize("tail", H.BITMAP_TAILS)
def test_bitmap_words(tail, monkeypatch, capfd):
    """Nodes that are whole bitmap words, the last bit of one, the last and the first of two, all but the outer bits of three
    (popc_range's masks), 1000 occurrences of 9 assemblies; n mod 128 = 63, 64, 65: the last wave row's second word."""
    want_n, _ = _check(f"bitmap_tail{tail}", "direct", monkeypatch, capfd)
    assert int((want_n["n_tar"] + want_n["n_neg"]).max()) == 9


@pytest.mark.parametrize("name", ("headless_tiles", "all_equal", "all_equal_hash0", "all_distinct", "long_look_back"))
def test_tiles_without_heads_and_the_look_back(name, monkeypatch, capfd):
    """Tiles that publish 0 heads, one node in all (once with the hash 0), a node per occurrence, and 130 tiles + 1 occurrence
    around a node of 70 tiles: a look-back of three steps, one of them over more than 64 tiles without a head, and the number of
    nodes from a last tile of one occurrence."""
    want_n, _ = _check(name, "direct", monkeypatch, capfd)
    if name.startswith("all_equal"):
        assert len(want_n) == 1 and (int(want_n["hash"][0]) == 0) == name.endswith("hash0")
    if name == "all_distinct":
        assert len(want_n) == H.case(name).n


def test_base_above_two_to_the_32(monkeypatch, capfd):
    want_n, _ = _check("base_offset", "direct", monkeypatch, capfd)
    assert int(want_n["start"][0]) == 2**32 - 5 and int(want_n["stop"][-1]) == 2**32 - 5 + 20_000


def test_without_targets(monkeypatch, capfd):
    """is_targets=None with a record table: counts and penalty are zero, the ranks are still marked."""
    want_n, want_r = _check("without_targets", "direct", monkeypatch, capfd)
    assert not want_n["n_tar"].any() and not want_n["n_neg"].any() and not want_n["penalty"].view(np.uint64).any()
    assert (want_r >> np.uint32(31)).any()


SMALL_ROUTED = [(r, c) for r in ("one_bucket", "sort_rocprim", "sort_own")
                for c in [f"boundaries_{v}" for v in H.BOUNDARY_VARIANTS] + ["asm_plain", "asm_mirror"]]


@pytest.mark.parametrize("route,what", SMALL_ROUTED, ids=[f"{r}-{c}" for r, c in SMALL_ROUTED])
def test_the_small_unsort_routes(route, what, monkeypatch, capfd):
    """The run-boundary and assembly-change layouts behind each unsort route, at the size that leads to it (2^14 rows hold the
    boundaries up to p = 8192): the rank words, marks included, are the same on every route."""
    _check(f"routed_{'one_bucket' if route == 'one_bucket' else 'sort'}_{what}", route, monkeypatch, capfd)


@pytest.fixture(scope="module")
def large():
    """The rows and the reference of the input above 2^22 rows, once for both routes that need that size."""
    _ref("large")
    return "large"


@pytest.mark.parametrize("route", ("two_passes", "fused"))
def test_the_large_unsort_routes(route, large, monkeypatch, capfd):
    """2^22 + 3 x 8192 + 1 rows: every boundary layout, both forms of the assembly changes, and a node of 20 000 occurrences of
    one assembly (whole tiles of marked words in one digit)."""
    _, want_r = _check(large, route, monkeypatch, capfd)
    assert int((want_r >> np.uint32(31)).sum()) > 20_000


def test_four_builds_alternating_two_sizes_on_the_fused_route(large, monkeypatch, capfd):
    """Tickets, tile states and cursors are per build."""
    eng = _engine()
    for i in range(4):
        _check((large, "second_large")[i % 2], "fused", monkeypatch, capfd, eng)
