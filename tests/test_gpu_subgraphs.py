"""The subgraph walk on the device (csrc/subgraph.hip: Index.subgraphs, kmers.get_subgraphs) against the reference's
kmers._get_subgraphs (goldens under tests/golden/subgraphs/) and the host restatement (tests/tools/subgraphs_host.py)."""
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import subgraphs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
GRAPHS = H.load_golden(GOLDEN)


def _np_sets(sgs):
    return tuple(frozenset(int(x) for x in s) for s in sgs)


def _check_types(sgs, used):
    assert isinstance(sgs, tuple) and all(isinstance(s, frozenset) for s in sgs) and isinstance(used, frozenset)
    assert all(type(x) is np.uint64 for s in sgs[:3] for x in s) and all(type(x) is np.uint64 for x in list(used)[:3])


def _induced_ok(sg, nodes, edges):
    """Subgraphs.induced_edges() == the restatement's, subgraph by subgraph."""
    offs, hashes = sg.csr()
    h = np.asarray(nodes["hash"], np.uint64)
    o = offs.astype(np.int64)
    rank_sgs = [np.searchsorted(h, hashes[o[i]:o[i + 1]]) for i in range(len(o) - 1)]
    want = H.induced_edges(edges, h, rank_sgs)
    got = sg.induced_edges()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("gi", range(len(GRAPHS)), ids=[g["name"] for g, _, _, _ in GRAPHS])
def test_golden_pipeline_and_dropin(gi):
    from seqwin_amd import kmers
    from seqwin_amd.device import Batch, Subgraphs
    g, nodes, edges, cases = GRAPHS[gi]
    b = Batch.from_fasta([GOLDEN / p for p in g["paths"]])
    ix = b.build_index(g["k"], g["w"], g["is_targets"])
    f = ix.filter_graph(g["edge_weight_th"])
    _, fn, fe = f.export()
    assert np.array_equal(fn["hash"], nodes["hash"]) and np.array_equal(fn["penalty"].view(np.uint64), nodes["penalty"].view(np.uint64))
    assert np.array_equal(fe, edges)
    for case, exp in cases:
        args = (case["penalty_th"], case["min_nodes"], case["max_nodes"])
        for route in ("index", "dropin"):
            rng = random.Random(case["seed"])
            if exp is None:
                with pytest.raises(RuntimeError) as ei:
                    if route == "index":
                        f.subgraphs(*args, rng)
                    else:
                        kmers.get_subgraphs(nodes, edges, *args, rng)
                assert str(ei.value) == case["error"]
            else:
                want = H.csr_to_sets(*exp)
                if route == "index":
                    sg = f.subgraphs(*args, rng)
                    assert isinstance(sg, Subgraphs)
                    sgs, used = sg.as_reference()
                    _induced_ok(sg, nodes, edges)
                    assert sg.stats()["kept"] == len(want)
                    sg.close()
                else:
                    sgs, used = kmers.get_subgraphs(nodes, edges, *args, rng)
                _check_types(sgs, used)
                assert _np_sets(sgs) == want, (route, case)
                assert used == frozenset().union(*want)
            assert rng.random() == case["rng_after"], (route, case)


def test_filter_kmers_with_the_device_used_mask():
    import oracle
    from seqwin_amd.device import Batch
    for g, nodes, edges, cases in GRAPHS:
        case, exp = next((c, e) for c, e in reversed(cases) if e is not None)
        b = Batch.from_fasta([GOLDEN / p for p in g["paths"]])
        ix = b.build_index(g["k"], g["w"], g["is_targets"])
        f = ix.filter_graph(g["edge_weight_th"])
        sg = f.subgraphs(case["penalty_th"], case["min_nodes"], case["max_nodes"], random.Random(case["seed"]))
        got = ix.filter_kmers(f, sg)
        k_all, _, _ = ix.export()
        _, fnodes, _ = f.export()
        gk, gn, _ = got.export()
        ek, en = oracle.filter_kmers(k_all, fnodes, exp[1])
        assert len(en) == len(exp[1])
        assert np.array_equal(gk, ek) and np.array_equal(gn, en), g["name"]
        assert np.array_equal(sg.used_hashes(), np.sort(exp[1]))
        assert sg.used_mask().sum() == len(exp[1])


def _synthetic(n_genomes, n_anc, snp_ppm, seed, penalty_th=None, k=21, w=10):
    """Batch.synthetic with a target clade (the genomes of ancestor 0) and the reference's thresholds: computed from the sketches
    (kmers.py:426-440) when penalty_th is None, else given as --penalty-th gives it (edge_weight_th follows, kmers.py:453).  The
    generator's ancestors share no k-mers, so the computed penalty_th is ~0 and leaves no seed: the walks with work are given one."""
    from seqwin_amd.device import Batch
    b = Batch.synthetic(n_genomes, 2, 20000, n_ancestors=n_anc, snp_ppm=snp_ppm, seed=seed)
    tar = [i % n_anc == 0 for i in range(n_genomes)]
    n_tar = sum(tar)
    ix = b.build_index(k, w, tar)
    _, nodes, _ = ix.export()
    pth, ewt = H.thresholds(nodes, n_tar, n_genomes - n_tar)
    if penalty_th is not None:
        pth, ewt = penalty_th, 0.3 * (1 - penalty_th) * n_tar
    f = ix.filter_graph(ewt)
    _, fn, fe = f.export()
    return b, ix, f, fn, fe, pth


@pytest.mark.parametrize("n_genomes,n_anc,snp_ppm,seed", [(256, 2, 5000, 3), (300, 4, 8000, 4), (200, 3, 3000, 5)])
def test_synthetic_batches_against_the_restatement(n_genomes, n_anc, snp_ppm, seed, monkeypatch):
    invalidated, walks = 0, 0
    for given in (None, 0.2, 0.1, 0.4):
        b, ix, f, fn, fe, pth = _synthetic(n_genomes, n_anc, snp_ppm, seed, given)
        for th, mn, mx in ((pth, 3, 100), (pth, 1, None), (pth, 5, 3)):
            rs = random.Random(seed)
            try:
                want = H.get_subgraphs(fn, fe, th, mn, mx, rs)[:2]
            except RuntimeError:
                want = None
            after = rs.random()
            frontier = 0
            for env in ({}, {"SEQWIN_AMD_SG_WINDOW": "1"}, {"SEQWIN_AMD_SG_WINDOW": "7"}, {"SEQWIN_AMD_SG_LDS_CAP": "1"}):
                for k in ("SEQWIN_AMD_SG_WINDOW", "SEQWIN_AMD_SG_LDS_CAP"):
                    monkeypatch.delenv(k, raising=False)
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                rng = random.Random(seed)
                if want is None:
                    with pytest.raises(RuntimeError):
                        f.subgraphs(th, mn, mx, rng)
                else:
                    sg = f.subgraphs(th, mn, mx, rng)
                    got = sg.as_reference()
                    st = sg.stats()
                    assert _np_sets(got[0]) == want[0] and got[1] == want[1], (th, mn, mx, env)
                    if env == {"SEQWIN_AMD_SG_WINDOW": "1"}:
                        assert st["invalidated"] == 0 and st["expansions"] == st["kept"] + st["discarded"] <= st["rounds"]
                    if "SEQWIN_AMD_SG_LDS_CAP" in env and frontier > 1:
                        assert st["spilled"] > 0, st   # every frontier of two or more entries took the spill path
                    if not env:
                        invalidated += st["invalidated"]
                        walks += 1
                        frontier = st["max_frontier"]
                    assert st["kept"] + st["discarded"] + st["skipped_used"] == st["seeds"], st
                    sg.close()
                assert rng.random() == after
    assert walks >= 3 and invalidated > 0   # walks with work ran, and the conflict path with them


def test_no_seed_and_nothing_kept():
    b, ix, f, fn, fe, pth = _synthetic(64, 2, 5000, 9, 0.2)
    rng = random.Random(5)
    st = rng.getstate()
    with pytest.raises(RuntimeError, match="No low-penalty subgraph was found"):
        f.subgraphs(-1.0, 1, None, rng)
    assert rng.getstate() == st   # no seed: shuffle of an empty list
    n_seeds = f.subgraph_seeds(pth)
    assert n_seeds > 0
    rng = random.Random(5)
    with pytest.raises(RuntimeError, match="No low-penalty subgraph was found"):
        f.subgraphs(pth, 101, 100, rng)   # seeds, none kept
    ref = random.Random(5)
    ref.shuffle(list(range(n_seeds)))
    assert rng.random() == ref.random()


def test_max_nodes_zero_and_one_and_empty_graph():
    b, ix, f, fn, fe, pth = _synthetic(64, 2, 5000, 10, 0.2)
    for mx in (0, 1):
        rs = random.Random(mx)
        want = H.get_subgraphs(fn, fe, pth, 1, mx, rs)[:2]
        rng = random.Random(mx)
        sg = f.subgraphs(pth, 1, mx, rng)
        got = sg.as_reference()
        assert all(len(s) == 1 for s in got[0]) and _np_sets(got[0]) == want[0] and got[1] == want[1]
        assert len(got[0]) == f.subgraph_seeds(pth)
        assert rng.random() == rs.random()
    empty = ix.filter_graph(1e9)
    assert empty.sizes()[1:] == (0, 0) and empty.subgraph_seeds(1.0) == 0
    rng = random.Random(1)
    with pytest.raises(RuntimeError):
        empty.subgraphs(1.0, 1, None, rng)


def test_hub_node_beyond_the_lds_frontier():
    """A hub of degree 5000 (> the 1024 frontier entries a wave keeps in LDS) and max_nodes=None: the spill path."""
    from seqwin_amd._core import EDGE_DTYPE, NODE_DTYPE
    from seqwin_amd import kmers
    from seqwin_amd.device import Index
    r = np.random.default_rng(7)
    n = 6000
    nodes = np.zeros(n, NODE_DTYPE)
    nodes["hash"] = np.sort(r.choice(1 << 60, n, replace=False)).astype(np.uint64)
    nodes["penalty"] = r.choice([0.0, 0.05, 0.1, 0.3, 0.7], n)
    hub = 17
    nodes["penalty"][hub] = 0.0
    spokes = np.setdiff1d(np.arange(5001), [hub])
    extra = r.integers(0, n, (3000, 2))
    a = np.concatenate([np.full(len(spokes), hub), extra[:, 0]])
    c = np.concatenate([spokes, extra[:, 1]])
    lo, hi = np.minimum(a, c), np.maximum(a, c)
    pairs = np.unique(np.stack([lo, hi], 1), axis=0)
    edges = np.zeros(len(pairs), EDGE_DTYPE)
    edges["first"] = nodes["hash"][pairs[:, 0]]
    edges["second"] = nodes["hash"][pairs[:, 1]]
    edges["weight"] = 1
    for th, mn, mx in ((0.1, 1, None), (0.2, 3, 100), (0.05, 2, None)):
        rs = random.Random(11)
        want = H.get_subgraphs(nodes, edges, th, mn, mx, rs)
        ix = Index.from_arrays(nodes, edges)
        rng = random.Random(11)
        sg = ix.subgraphs(th, mn, mx, rng)
        got = sg.as_reference()
        assert _np_sets(got[0]) == want[0] and got[1] == want[1]
        assert rng.random() == rs.random()
        st = sg.stats()
        if mx is None and th >= 0.1:
            assert st["spilled"] > 0 and st["max_frontier"] > 1024, st
        _induced_ok(sg, nodes, edges)
        rng = random.Random(11)
        assert kmers.get_subgraphs(nodes, edges, th, mn, mx, rng) == got
    with pytest.raises(ValueError):   # an edge endpoint that is no node
        bad = edges.copy()
        bad["second"][0] = 3
        Index.from_arrays(nodes, bad).subgraphs(0.1, 1, None, random.Random(1))


def test_release_library_walk():
    """The release library (test hooks compiled out) through the drop-in, on two golden cases."""
    code = (
        "import random, sys, numpy as np\n"
        "sys.path.insert(0, 'tests/tools')\n"
        "import subgraphs_host as H\n"
        "from seqwin_amd._lib import LIB_PATH\n"
        "from seqwin_amd import kmers\n"
        "assert str(LIB_PATH).endswith('libseqwin_hip.so'), LIB_PATH\n"
        "n = 0\n"
        "for g, nodes, edges, cases in H.load_golden('tests/golden'):\n"
        "    for case, exp in cases:\n"
        "        if exp is None or n >= 8: continue\n"
        "        rng = random.Random(case['seed'])\n"
        "        sgs, used = kmers.get_subgraphs(nodes, edges, case['penalty_th'], case['min_nodes'], case['max_nodes'], rng)\n"
        "        assert tuple(frozenset(int(x) for x in s) for s in sgs) == H.csr_to_sets(*exp)\n"
        "        assert rng.random() == case['rng_after']\n"
        "        n += 1\n"
        "print('release ok', n)\n")
    env = {k: v for k, v in os.environ.items() if k != "SEQWIN_AMD_LIB"}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "release ok 8" in r.stdout, r.stdout


# ---- adversarial shapes (tests/tools/sg_shapes.py) against goldens recorded from the reference ---------------------------------
import sg_shapes as S  # noqa: E402

SHAPES = S.load_golden(GOLDEN)
SG_HOOKS = ("SEQWIN_AMD_SG_WINDOW", "SEQWIN_AMD_SG_LDS_CAP")


def _hooks(monkeypatch, **env):
    for k in SG_HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(f"SEQWIN_AMD_SG_{k}", str(v))


def _run_shape(ix, case):
    """(Subgraphs or the error text, rng.random() afterwards) of Index.subgraphs."""
    rng = random.Random(case["seed"])
    try:
        sg = ix.subgraphs(case["penalty_th"], case["min_nodes"], case["max_nodes"], rng)
    except RuntimeError as e:
        return str(e), rng.random()
    return sg, rng.random()


def _digest(sg):
    return S.csr_digest(*sg.csr())


def _induced_grouped_ok(sg, nodes, edges):
    """Subgraphs.induced_edges() == H.induced_edges, computed in one pass (a stable sort by subgraph) for walks with many subgraphs."""
    offs, hashes = sg.csr()
    h = np.asarray(nodes["hash"], np.uint64)
    sg_of = np.full(len(h), -1, np.int64)
    sg_of[np.searchsorted(h, hashes)] = np.repeat(np.arange(len(offs) - 1), np.diff(offs.astype(np.int64)))
    a = sg_of[np.searchsorted(h, edges["first"])]
    b = sg_of[np.searchsorted(h, edges["second"])]
    hit = np.flatnonzero((a >= 0) & (a == b))
    hit = hit[np.argsort(a[hit], kind="stable")]
    got = sg.induced_edges()
    assert len(got) == len(offs) - 1
    assert np.array_equal(np.array([len(x) for x in got], np.int64), np.bincount(a[hit], minlength=len(offs) - 1))
    assert np.array_equal(np.concatenate(got) if got else edges[:0], edges[hit])


def _shape_paths(g, case, st):
    """The kernel paths each family is built to reach."""
    fam, p = g["family"], g["params"]
    assert st["kept"] + st["discarded"] + st["skipped_used"] == st["seeds"], st
    assert st["kept"] == case["n_subgraphs"], st
    if fam == "star":
        nf = p["deg"] + max(p.get("deg2", 0) - 1, 0)   # the first accepted leaf leaves the frontier before its neighbours enter
        if nf <= 1024:
            assert st["max_frontier"] == nf and st["spilled"] == 0, st
        else:
            assert st["spilled"] >= 1, st
    if fam == "many_seeds":
        assert st["window"] == 4096 and st["invalidated"] == 0, st
    if fam == "dense":
        assert st["invalidated"] > 0, st
    if fam == "multi_spill" and case["max_nodes"] is None:
        assert st["spilled"] >= p["hubs"], st


@pytest.mark.parametrize("gi", range(len(SHAPES)), ids=[g["id"] for g, _, _, _ in SHAPES])
def test_shapes_against_the_reference(gi, monkeypatch):
    """Index.from_arrays(...).subgraphs and the drop-in kmers.get_subgraphs on every shape case: subgraphs in final order, used,
    element types, rng state, induced edges and used hashes against the goldens, and the kernel paths reached."""
    from seqwin_amd import kmers
    from seqwin_amd.device import Index
    _hooks(monkeypatch)
    g, nodes, edges, cases = SHAPES[gi]
    ix = Index.from_arrays(nodes, edges)
    for case, exp in cases:
        want = case["error"] or case["csr_sha256"]
        sg, after = _run_shape(ix, case)
        assert after == case["rng_after"], case
        if case["error"]:
            assert sg == case["error"]
        else:
            sgs, used = sg.as_reference()
            _check_types(sgs, used)
            assert _digest(sg) == want, case
            if exp is not None:
                assert _np_sets(sgs) == H.csr_to_sets(*exp), case
            offs, hashes = sg.csr()
            assert len(used) == case["n_used"] == len(hashes) and frozenset(int(x) for x in used) == frozenset(hashes.tolist())
            assert np.array_equal(sg.used_hashes(), np.sort(hashes))
            assert sg.used_mask().sum() == case["n_used"]
            _induced_grouped_ok(sg, nodes, edges)
            if case["n_subgraphs"] <= 300:
                _induced_ok(sg, nodes, edges)
            _shape_paths(g, case, sg.stats())
            sg.close()
        rng = random.Random(case["seed"])
        try:
            got = kmers.get_subgraphs(nodes, edges, case["penalty_th"], case["min_nodes"], case["max_nodes"], rng)
            _check_types(*got)
            got = S.csr_digest(*S.canonical_csr(got[0]))
        except RuntimeError as e:
            got = str(e)
        assert got == want and rng.random() == case["rng_after"], ("dropin", case)
    ix.close()


def _shape(family, **params):
    return next(s for s in SHAPES if s[0]["family"] == family and all(s[0]["params"].get(k) == v for k, v in params.items()))


@pytest.mark.parametrize("family", ["many_seeds", "dense"])
def test_window_sizes_give_one_result(family, monkeypatch):
    from seqwin_amd.device import Index
    g, nodes, edges, cases = _shape(family)
    case = cases[0][0]
    ix = Index.from_arrays(nodes, edges)
    for w in (1, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 10000):
        _hooks(monkeypatch, WINDOW=w)
        sg, after = _run_shape(ix, case)
        assert _digest(sg) == case["csr_sha256"] and after == case["rng_after"], w
        st = sg.stats()
        assert st["window"] == min(w, 4096) and st["kept"] + st["discarded"] + st["skipped_used"] == st["seeds"], (w, st)
        if w == 1:
            # one expansion per round; a last round may find only used seeds left and expand nothing
            assert st["invalidated"] == 0 and st["expansions"] <= st["rounds"] <= st["expansions"] + 1, st
        sg.close()
    ix.close()


@pytest.mark.parametrize("deg", [1024, 1025, 2048])
def test_lds_frontier_caps_give_one_result(deg, monkeypatch):
    from seqwin_amd.device import Index
    g, nodes, edges, cases = _shape("star", deg=deg)
    ix = Index.from_arrays(nodes, edges)
    for cap in (1, 63, 64, 65, 1023):
        _hooks(monkeypatch, LDS_CAP=cap)
        for case, _ in cases:
            sg, after = _run_shape(ix, case)
            assert _digest(sg) == case["csr_sha256"] and after == case["rng_after"], (cap, case)
            assert sg.stats()["spilled"] >= 1
            sg.close()
    ix.close()


def test_long_components_spill_once_each(monkeypatch):
    """Window 1: exactly one spill per component that an expansion takes beyond the 128 LDS subgraph entries."""
    from seqwin_amd.device import Index
    g, nodes, edges, cases = _shape("long")
    big = 3 * sum(s >= 129 for s in g["params"]["sizes"])
    ix = Index.from_arrays(nodes, edges)
    _hooks(monkeypatch, WINDOW=1)
    for case, _ in cases:
        sg, after = _run_shape(ix, case)
        assert _digest(sg) == case["csr_sha256"] and after == case["rng_after"], case
        mx = case["max_nodes"]
        st = sg.stats()
        assert st["spilled"] == (big if mx is None or mx > 128 else 0), (case, st)
        sg.close()
    _hooks(monkeypatch, WINDOW=1, LDS_CAP=64)   # the cliques' frontiers spill too, the paths' do not
    sg, _ = _run_shape(ix, cases[0][0])
    assert _digest(sg) == cases[0][0]["csr_sha256"]
    ix.close()


def test_multiple_spills_with_invalidation(monkeypatch):
    from seqwin_amd.device import Index
    g, nodes, edges, cases = _shape("multi_spill")
    ix = Index.from_arrays(nodes, edges)
    for env in ({}, {"WINDOW": 1}, {"WINDOW": 4096}):
        _hooks(monkeypatch, **env)
        for case, _ in cases:
            sg, after = _run_shape(ix, case)
            st = sg.stats()
            assert _digest(sg) == case["csr_sha256"] and after == case["rng_after"], (env, case)
            assert st["spilled"] >= g["params"]["hubs"], (env, st)
            if env.get("WINDOW") == 4096:
                assert st["invalidated"] > 0, st
            sg.close()
    ix.close()


def test_filter_chain_at_scale():
    """filter_graph, subgraphs and filter_kmers on the bench generator's graph (512 genomes, 30 ancestors, penalty_th 0.2)
    against the numpy expressions of kmers._filter_edges_and_nodes, the host restatement and the oracle's filter_kmers."""
    import oracle
    from seqwin_amd.device import Batch
    G, th = 512, 0.2
    b = Batch.synthetic(G, 50, 100_000, n_ancestors=30, snp_ppm=10_000, seed=1)
    tar = [g % 30 == 0 for g in range(G)]
    n_tar = sum(tar)
    ix = b.build_index(21, 200, tar)
    ewt = 0.3 * (1 - th) * n_tar
    k_all, nodes, edges = ix.export()
    e_want = edges[edges["weight"] > np.uintp(ewt)]
    keep = np.unique(e_want.view(np.uint64).reshape(-1, 3)[:, :2])
    n_want = nodes[np.searchsorted(nodes["hash"], keep)]
    f = ix.filter_graph(ewt)
    _, fn, fe = f.export()
    assert len(fn) > 1_000_000 and np.array_equal(fn, n_want) and np.array_equal(fe, e_want)
    rs = random.Random(1)
    want = H.get_subgraphs(fn, fe, th, 3, 100, rs)
    rng = random.Random(1)
    sg = f.subgraphs(th, 3, 100, rng)
    got = sg.as_reference()
    assert _np_sets(got[0]) == want[0] and got[1] == want[1] and rng.random() == rs.random()
    st = sg.stats()
    assert st["kept"] == len(want[0]) > 1000 and st["kept"] + st["discarded"] + st["skipped_used"] == st["seeds"]
    gk, gn, _ = ix.filter_kmers(f, sg).export()
    ek, en = oracle.filter_kmers(k_all, fn, sg.used_hashes())
    assert np.array_equal(gk, ek) and np.array_equal(gn, en) and len(en) == len(want[1])
    sg.close()


def test_release_library_shapes():
    """The release library (test hooks compiled out) through the drop-in on the many-seeds and rounding shapes."""
    code = (
        "import random, sys\n"
        "sys.path.insert(0, 'tests/tools')\n"
        "import sg_shapes as S\n"
        "from seqwin_amd._lib import LIB_PATH\n"
        "from seqwin_amd import kmers\n"
        "assert str(LIB_PATH).endswith('libseqwin_hip.so'), LIB_PATH\n"
        "n = 0\n"
        "for g, nodes, edges, cases in S.load_golden('tests/golden', families=('many_seeds', 'rounding')):\n"
        "    for case, _ in cases:\n"
        "        rng = random.Random(case['seed'])\n"
        "        sgs, used = kmers.get_subgraphs(nodes, edges, case['penalty_th'], case['min_nodes'], case['max_nodes'], rng)\n"
        "        assert S.csr_digest(*S.canonical_csr(sgs)) == case['csr_sha256'], (g['id'], case)\n"
        "        assert rng.random() == case['rng_after']\n"
        "        n += 1\n"
        "print('release ok', n)\n")
    env = {k: v for k, v in os.environ.items() if k not in ("SEQWIN_AMD_LIB",) + SG_HOOKS}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    n = sum(len(cs) for g, _, _, cs in SHAPES if g["family"] in ("many_seeds", "rounding"))
    assert f"release ok {n}" in r.stdout, r.stdout
