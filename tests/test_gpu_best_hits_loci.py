"""GPU: Batch.best_hits(loci=True) / Markers.best_hits(loci=True) -- every seeded locus of every (query, assembly) pair (the loci
mode of csrc/hits.hip) against the host restatement tests/tools/loci_host.py: the hand-made cases of
tests/test_loci_cpu.py, and one seeded random case run plain and with the hit buffer split and doubled, one probe workgroup, several
rounds of the traceback scratch, one workgroup per list launch and the striped route, for min_seeds 1, 2 and 3.  The nine matrix
fields stay what align=True gives."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import hits_host as H  # noqa: E402
import loci_cases as C  # noqa: E402
import loci_host as L  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
MATRIX = ("seeds", "record", "strand", "end", "dist", "start", "nident", "mismatch", "gaps")


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d some text\n" % (name.encode(), i))
            r = bytes(r)
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def _batch(d, assemblies, tag="a"):
    from seqwin_amd.device import Batch
    return Batch.from_fasta([_write(d, f"{tag}{i}.fa", recs) for i, recs in enumerate(assemblies)], n_cpu=2)


def _got(h):
    got = h.loci()
    got["n_loci"], got["sum_nident"] = h.n_loci(), h.sum_nident()
    return got


def _same(got, want, what=""):
    for f in L.LIST_FIELDS + ("cell_offsets", "n_loci", "sum_nident"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f, got[f].dtype, got[f].shape, want[f].shape)
        assert np.array_equal(got[f], want[f]), (what, f, got[f].tolist(), want[f].tolist())


def _check(batch, queries, want, min_seeds=1, what=""):
    """loci=True against the restatement; returns (the arrays, stats, loci_stats, the nine matrix fields)."""
    h = batch.best_hits(queries, C.K, loci=True, min_seeds=min_seeds)
    try:
        got = _got(h)
        _same(got, want, what)
        ls = h.loci_stats()
        assert ls["loci"] == len(want["query"]) == ls["pairs_aligned"] and ls["duplicates"] == int(want["dup"].sum())
        assert ls["max_loci_per_cell"] == int(want["n_loci"].max(initial=0))
        return got, h.stats(), ls, {f: getattr(h, f)() for f in MATRIX}
    finally:
        h.close()


@pytest.mark.parametrize("name", sorted(C.hand_made()))
def test_hand_made_cases(name, tmp_path):
    queries, asms, rows = C.hand_made()[name]
    b = _batch(tmp_path, asms)
    try:
        for ms in (1, 2):
            want = L.best_hits_loci(queries, asms, C.K, ms)
            got, _, _, matrix = _check(b, queries, want, ms, name)
            aligned = A.best_hits_aligned(queries, asms, C.K)
            for f in MATRIX:
                assert np.array_equal(matrix[f], aligned[f]), (name, ms, f)
        if name == "single_seed":
            assert got["n_loci"].tolist() == [[1, 0]] and matrix["seeds"].tolist() == [[50, 1]]
    finally:
        b.close()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """The seeded random case, its restatement for min_seeds 1, 2, 3 (computed once) and the matrix fields of align=True."""
    queries, asms = C.random_large()
    want = {ms: L.best_hits_loci(queries, asms, C.K, ms) for ms in (1, 2, 3)}
    aligned = A.best_hits_aligned(queries, asms, C.K)
    # what the case is there for, before a device is touched
    w1 = want[1]
    records = [r for recs in asms for r in recs]
    assert w1["n_loci"].max() >= 3, "no cell with three loci"
    assert int(w1["n_candidates"]) > len(w1["query"]), "no suppressed neighbour"
    assert w1["dup"].any(), "no duplicate"
    assert any(int(w1["band"][j]) >= (len(records[w1["record"][j]]) - C.K) >> 6 for j in range(len(w1["query"]))), "no locus in a record's last band"
    below = (aligned["seeds"] > 0) & (aligned["seeds"] < 3)
    assert below.any() and (want[3]["n_loci"][below] == 0).all(), "no cell whose winner is below min_seeds"
    assert max(len(q) for q in queries) > 64 * 64
    b = _batch(tmp_path_factory.mktemp("loci"), asms, "l")
    yield b, queries, asms, want, aligned
    b.close()


@pytest.mark.parametrize("min_seeds", (1, 2, 3))
def test_random_case(big, min_seeds):
    """The restatement, and the nine matrix fields of align=True whatever min_seeds is."""
    b, queries, asms, want, aligned = big
    _, st, ls, matrix = _check(b, queries, want[min_seeds], min_seeds)
    assert st["chunks"] == 1 and st["chunk_splits"] == 0 and st["buffer_doublings"] == 0 and ls["rounds"] == 1
    h = b.best_hits(queries, C.K, align=True)
    try:
        for f in MATRIX:
            assert np.array_equal(matrix[f], getattr(h, f)()) and np.array_equal(matrix[f], aligned[f]), f
        assert np.array_equal(h.n_seeds(), aligned["n_seeds"])
    finally:
        h.close()


def test_random_case_under_the_hooks(big, monkeypatch):
    """Chunks, splits and one doubling of the hit buffer; one probe workgroup per launch; several rounds of the traceback's scratch;
    one workgroup per launch of the list kernels; the striped route for everything above one block: every array as without a hook."""
    b, queries, asms, want, aligned = big
    plain = {ms: _check(b, queries, want[ms], ms) for ms in (1, 2, 3)}
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")
    h = b.best_hits(queries, C.K)
    per_assembly = h.stats()["chunk_hits"]               # (64 keys: every chunk is one assembly)
    h.close()
    assert len(per_assembly) == len(asms)
    kb = (max(per_assembly) // 2 + 63) // 64            # the largest assembly does not fit, twice the buffer holds it
    assert kb * 64 < max(per_assembly) <= 2 * kb * 64
    runs = (("buffer", {"SEQWIN_AMD_HIT_BUFFER_KB": str(kb)}), ("probe", {"SEQWIN_AMD_HIT_MAX_BLOCKS": "1"}),
            ("scratch", {"SEQWIN_AMD_ALN_SCRATCH_KB": "64"}), ("lists", {"SEQWIN_AMD_SEQ_MAX_BLOCKS": "1"}),
            ("striped", {"SEQWIN_AMD_DIST_LDS_CAP": "1"}))
    for what, env in runs:
        monkeypatch.delenv("SEQWIN_AMD_HIT_BUFFER_KB", raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        for ms in (1, 2, 3):
            got, st, ls, matrix = _check(b, queries, want[ms], ms, what)
            _same(got, plain[ms][0], what)
            for f in MATRIX:
                assert np.array_equal(matrix[f], plain[ms][3][f]), (what, f)
        if what == "buffer":
            assert st["chunk_splits"] > 0 and st["buffer_doublings"] == 1 and st["chunks"] > 1
        elif what == "probe":
            assert st["launches"] > plain[3][1]["launches"]
        elif what == "scratch":
            assert ls["rounds"] > 1
        elif what == "striped":
            assert st["striped_pairs"] > plain[3][1]["striped_pairs"] > 0
        for name in env:
            monkeypatch.delenv(name)


def test_loci_fetch_and_replay(big):
    """loci_intervals() hands Batch.fetch the located copies; the script of every locus that is no duplicate, traced again on its
    window, replays to that text."""
    b, queries, asms, want, _ = big
    w = want[1]
    h = b.best_hits(queries, C.K, loci=True)
    try:
        iv = h.loci_intervals()
    finally:
        h.close()
    keep = np.flatnonzero(w["dup"] == 0)
    assert len(iv) == len(keep) and np.array_equal(iv["record"], w["record"][keep])
    assert np.array_equal(iv["start"], w["start"][keep]) and np.array_equal(iv["stop"], w["end"][keep])
    offs, blob, _ = b.fetch(iv)
    o = offs.astype(np.int64)
    pairs = [(int(w["query"][j]), int(w["strand"][j]), int(w["record"][j]), int(w["lo"][j]), int(w["hi"][j])) for j in keep]
    res = b.infix_alignments(queries, pairs, ops=True)
    so = res[6].astype(np.int64)
    for x, j in enumerate(keep):
        assert (res[0][x], res[1][x], res[2][x], res[3][x]) == (w["dist"][j], w["end"][j], w["start"][j], w["nident"][j])
        pat = H._text(queries[w["query"][j]])
        assert A.replay_matches(H._rc(pat) if w["strand"][j] else pat, res[7][so[x]:so[x + 1]], H._text(blob[o[x]:o[x + 1]])), j


def test_accessors_need_loci(big):
    b, queries, _, want, _ = big
    for kw in ({}, {"align": True}):
        h = b.best_hits(queries, C.K, **kw)
        try:
            for f in ("n_loci", "sum_nident", "loci", "loci_stats", "loci_intervals"):
                with pytest.raises(ValueError, match="loci"):
                    getattr(h, f)()
            from seqwin_amd._lib import c_u64, lib
            out = np.zeros(1, np.uint32)
            n = c_u64()
            assert lib.sw_hits_loci_block(h._h, c_u64(0), c_u64(0), c_u64(1), c_u64(0), c_u64(1), out.ctypes.data) == 2   # SW_ERR_VALUE
            assert lib.sw_hits_loci_sizes(h._h, __import__("ctypes").byref(n), None) == 2
            assert lib.sw_hits_loci_stats(h._h, None, None) == 2 and lib.sw_hits_loci(h._h, *([None] * 14)) == 2
        finally:
            h.close()
    with pytest.raises(ValueError, match="min_seeds"):
        b.best_hits(queries, C.K, loci=True, min_seeds=0)
    from seqwin_amd._lib import c_u64, c_vp, lib
    hh = c_vp()
    offs = np.zeros(1, np.uint64)
    assert lib.sw_batch_best_hits_loci(b._h, offs.ctypes.data, b"", c_u64(0), c_u64(C.K), c_u64(0), __import__("ctypes").byref(hh)) == 2
    assert b"min_seeds" in lib.sw_last_error()
    h = b.best_hits(queries, C.K, loci=True, min_seeds=2)
    try:
        assert np.array_equal(h.n_loci((1, 4), (2, 4)), want[2]["n_loci"][1:4, 2:4]) and h.sum_nident((2, 2), (0, 4)).shape == (0, 4)
        with pytest.raises(ValueError, match="outside"):
            h.n_loci((0, 99), (0, 1))
        assert np.array_equal(h.nident(), b.best_hits(queries, C.K, align=True).nident())
    finally:
        h.close()


def test_repeat_summary(big):
    from seqwin_amd.markers import repeat_summary
    b, queries, _, want, _ = big
    w = want[1]
    lengths = [len(q) for q in queries]
    n_tar = 2
    h = b.best_hits(queries, C.K, loci=True)
    try:
        s = repeat_summary(h, lengths, n_tar)
        with pytest.raises(ValueError):
            repeat_summary(h, lengths[:-1], n_tar)
    finally:
        h.close()
    for q, m in enumerate(lengths):
        for loci_name, ident_name, cols in (("loci_tar", "identity_all_tar", range(0, n_tar)), ("loci_neg", "identity_all_neg", range(n_tar, 5))):
            cells = [a for a in cols if w["n_loci"][q, a] > 0]
            if not cells:
                assert s[loci_name][q] == 0.0 and s[ident_name][q] == 0.0
                continue
            assert s[loci_name][q] == np.mean([float(w["n_loci"][q, a]) for a in cells])
            assert np.isclose(s[ident_name][q], np.mean([w["sum_nident"][q, a] / w["n_loci"][q, a] for a in cells]) / m, rtol=1e-12, atol=0)
    assert s["loci_tar"].max() >= 2 and 0 < s["identity_all_tar"][0] <= 1


def test_markers_best_hits_loci():
    """The marker golden of tests/test_gpu_best_hits_aligned.py::test_markers_best_hits_aligned through Markers.best_hits(loci=True)."""
    from seqwin_amd.device import Batch
    sub = {g["name"]: g for g in json.loads((GOLDEN / "subgraphs" / "manifest.json").read_text())["graphs"]}
    c = next(c for c in json.loads((GOLDEN / "markers" / "manifest.json").read_text())["cases"]
             if c["graph"] == "smoke_k17_w10" and c["case"] == 6 and c["error"] is None)
    g = sub[c["graph"]]
    case = g["cases"][c["case"]]
    b = Batch.from_fasta([GOLDEN / p for p in g["paths"]])
    ix = b.build_index(g["k"], g["w"], g["is_targets"])
    f = ix.filter_graph(g["edge_weight_th"])
    sg = f.subgraphs(case["penalty_th"], case["min_nodes"], case["max_nodes"], random.Random(case["seed"]))
    kept = ix.filter_kmers(f, sg)
    m = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"])
    try:
        offs, blob, _ = m.sequences(b, "reps")
        o = offs.astype(np.int64)
        texts = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        ro = b.record_offsets()
        asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
        want = L.best_hits_loci(texts, asms, g["k"], 2)
        h = m.best_hits(b, g["k"], loci=True, min_seeds=2)
        ha = m.best_hits(b, g["k"], align=True)
        try:
            _same(_got(h), want)
            for fld in MATRIX:
                assert np.array_equal(getattr(h, fld)(), getattr(ha, fld)()), fld
            assert want["n_loci"].any()
        finally:
            h.close()
            ha.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
