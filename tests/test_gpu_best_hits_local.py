"""GPU: Batch.best_hits(local=True) / Markers.best_hits(local=True) -- the local alignment with affine gap scores (csrc/local.hip,
DESIGN.md section 3.2i) of every winner, and with loci=True of every locus, on the window of section 3.2e, against the host
restatement tests/tools/local_host.py; every field the call had before equals the same call with local=False bit for bit."""
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
import local_host as L  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
K = 15
BLASTN = (2, -3, 5, 2)
PLAIN = ("seeds", "record", "strand", "end", "dist")
ALIGNED = ("start", "nident", "mismatch", "gaps")
LOCAL = {"score": "score", "qstart": "qstart", "qend": "qend", "sstart": "sstart", "send": "send", "nident": "local_nident",
         "mismatch": "local_mismatch", "gapopen": "local_gapopen", "gaps": "local_gaps"}
NONE = np.uint32(0xFFFFFFFF)


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d\n" % (name.encode(), i))
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def _mutated(rng, seq, every):
    out = bytearray(seq)
    for at in range(every // 2, len(out), every):
        out[at:at + 1] = bytes([rng.choice([c for c in b"ACGT" if c != out[at]])])
    return bytes(out)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Queries: 0 a stretch of 300; 1 a stretch of 400 whose second half assembly 1 lacks (its contig ends inside the copy); 2 and 3
    the same 150 bases (seeds only with seed_copies=2); 4 a stretch with two deletions.  Assemblies: 0 the ancestor; 1 a contig that
    ends in the middle of query 1; 2 the reverse complement of a diverged ancestor; 3 two copies of query 2 in one record."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    rng = random.Random(29)
    anc = _rand(rng, 2000)
    gapped = bytearray(anc[1300:1600])
    del gapped[200:203]
    del gapped[90:91]
    queries = [anc[100:400], anc[500:900], anc[1000:1150], anc[1000:1150], bytes(gapped)]
    asms = [[anc],
            [_rand(rng, 120) + anc[50:700]],
            [_rand(rng, 40), H.revcomp(_mutated(rng, anc[80:1700], 37)) + _rand(rng, 70)],
            [_rand(rng, 200) + anc[1000:1150] + _rand(rng, 500) + anc[1000:1150] + _rand(rng, 100), anc[1250:1650]]]
    b = Batch.from_fasta([_write(tmp_path_factory.mktemp("bhl"), f"a{i}.fa", recs) for i, recs in enumerate(asms)], n_cpu=2)
    yield b, queries, asms
    b.close()


def _matrix(h, local=True):
    out = {f: getattr(h, f)() for f in PLAIN}
    if h._aligned:
        out.update({f: getattr(h, f)() for f in ALIGNED})
    if h._loci:
        out.update(n_loci=h.n_loci(), sum_nident=h.sum_nident())
        out.update({"loci_" + f: a for f, a in h.loci().items() if not f.startswith("local_")})
    out["n_seeds"] = h.n_seeds()
    return out


@pytest.mark.parametrize("scoring", [BLASTN, (1, -2, 0, 1)])
def test_winners_against_the_restatement(case, scoring):
    b, queries, asms = case
    records = [r for recs in asms for r in recs]
    want = A.best_hits_aligned(queries, asms, K)
    h = b.best_hits(queries, K, local=True, scoring=scoring)
    try:
        hit = want["seeds"] > 0
        assert hit.sum() >= 8 and np.array_equal(h.seeds(), want["seeds"])
        qs, cs = np.nonzero(hit)
        pairs = [(int(q), int(want["strand"][q, c]), int(want["record"][q, c]), int(want["lo"][q, c]), int(want["hi"][q, c])) for q, c in zip(qs, cs)]
        ref = L.alignments(queries, records, pairs, scoring)
        got = {f: getattr(h, m)() for f, m in LOCAL.items()}
        for f in L.FIELDS:
            assert got[f].dtype == np.uint32 and got[f].shape == hit.shape
            assert (got[f][~hit] == NONE).all(), f
            assert np.array_equal(got[f][qs, cs], ref[f]), (f, got[f][qs, cs].tolist(), ref[f].tolist())
        L.check({f: got[f][qs, cs] for f in L.FIELDS}, scoring, queries, records, pairs)
        st = h.local_stats()
        assert st["pairs"] == int(hit.sum()) and st["cells"] == sum(len(queries[p[0]]) * (p[4] - p[3]) for p in pairs) and st["local_ms"] >= 0
        with pytest.raises(ValueError):
            h.start()
    finally:
        h.close()


def test_loci_columns_against_the_restatement(case):
    b, queries, asms = case
    records = [r for recs in asms for r in recs]
    h = b.best_hits(queries, K, loci=True, local=True, seed_copies=2)
    try:
        lc = h.loci()
        n = len(lc["query"])
        assert n > int((h.seeds() > 0).sum())                                   # more loci than winners: the two copies of assembly 3
        m = np.array([len(queries[q]) for q in lc["query"]], np.int64)
        s0 = lc["band"].astype(np.int64) * 64 - (m - K)
        lo = np.maximum(s0 - 64, 0)
        hi = np.minimum(s0 + 192 + m, np.array([len(records[r]) for r in lc["record"]], np.int64))
        pairs = [(int(lc["query"][j]), int(lc["strand"][j]), int(lc["record"][j]), int(lo[j]), int(hi[j])) for j in range(n)]
        ref = L.alignments(queries, records, pairs)
        for f in L.FIELDS:
            assert lc["local_" + f].dtype == np.uint32 and np.array_equal(lc["local_" + f], ref[f]), f
        L.check({f: lc["local_" + f] for f in L.FIELDS}, BLASTN, queries, records, pairs)
        # the winner's cell fields are those of one of its cell's loci
        score, offs = h.score(), lc["cell_offsets"].astype(np.int64)
        for q, c in zip(*np.nonzero(h.seeds() > 0)):
            cell = q * score.shape[1] + c
            assert score[q, c] in lc["local_score"][offs[cell]:offs[cell + 1]]
        assert h.local_stats()["pairs"] == n + int((h.seeds() > 0).sum())
    finally:
        h.close()


@pytest.mark.parametrize("seed_copies", [None, 2])
@pytest.mark.parametrize("mode", ["plain", "align", "loci"])
def test_every_earlier_field_is_bit_for_bit_the_call_without_local(case, monkeypatch, mode, seed_copies):
    b, queries, _ = case
    kw = dict(align=mode == "align", loci=mode == "loci", min_seeds=2 if mode == "loci" else 1, seed_copies=seed_copies)

    def run(local):
        h = b.best_hits(queries, K, local=local, **kw)
        try:
            out = _matrix(h)
            if local:
                out.update({"local_" + f: getattr(h, m)() for f, m in LOCAL.items()})
                if mode == "loci":
                    out.update({"loci_" + f: a for f, a in h.loci().items() if f.startswith("local_")})
            else:
                for m in LOCAL.values():
                    with pytest.raises(ValueError):
                        getattr(h, m)()
                with pytest.raises(ValueError):
                    h.local_stats()
            return out, h.stats()
        finally:
            h.close()

    base, _ = run(False)
    with_local, st = run(True)
    assert st["chunks"] == 1
    for f, a in base.items():
        assert a.dtype == with_local[f].dtype and np.array_equal(a, with_local[f]), (mode, seed_copies, f)
    if seed_copies == 2:
        assert (base["seeds"][2] > 0).any() and np.array_equal(with_local["local_score"][2], with_local["local_score"][3])
    else:
        assert not base["seeds"][2].any() and (with_local["local_score"][2] == NONE).all()
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")                        # several chunks: a chunk's results do not depend on the others
    chunked, st = run(True)
    assert st["chunks"] > 1
    for f, a in with_local.items():
        assert np.array_equal(a, chunked[f]), (mode, seed_copies, f)


def test_half_a_copy_reads_as_a_clean_local_hit_and_local_summary(case):
    from seqwin_amd import markers
    b, queries, _ = case
    h = b.best_hits(queries, K, align=True, loci=True, local=True)
    try:
        m = len(queries[1])
        assert h.dist()[1, 1] >= m // 2 - 8                                     # the whole query against half a copy
        assert h.local_mismatch()[1, 1] + h.local_gaps()[1, 1] == 0
        assert h.qend()[1, 1] - h.qstart()[1, 1] == m // 2 and h.score()[1, 1] == 2 * (m // 2) and h.local_nident()[1, 1] == m // 2
        lengths = [len(q) for q in queries]
        n_tar = 2
        for best in (False, True):
            s = markers.local_summary(h, lengths, n_tar, best_locus=best)
            assert s.dtype == markers.LOCAL_SUMMARY_DTYPE and s.shape == (len(queries),)
            assert s["coverage_tar"][1] == (1.0 + 0.5) / 2 and s["identity_local_tar"][1] == (1.0 + 0.5) / 2 and s["f_tar"][1] == 1.0
            assert s["coverage_tar"][0] == 1.0 and s["f_tar"][0] == 1.0
            assert s["f_tar"][2] == 0.0 and s["coverage_tar"][2] == 0.0 and s["f_neg"][2] == 0.0   # a duplicated query has no unique seed
        hit = h.score() != NONE
        span = np.where(hit, h.qend().astype(np.float64) - h.qstart(), 0.0)
        edits = np.where(hit, h.local_mismatch().astype(np.float64) + h.local_gaps(), 0.0)
        s = markers.local_summary(h, lengths, n_tar)
        ln = np.array(lengths, np.float64)
        assert np.array_equal(s["coverage_tar"], span[:, :2].sum(axis=1) / ln / 2)
        assert np.array_equal(s["distance_local_neg"], edits[:, 2:].sum(axis=1) / ln / 2)
        assert np.array_equal(s["f_neg"], hit[:, 2:].sum(axis=1) / 2)
        assert s["distance_local_neg"][0] > 0                                  # the diverged reverse complement of assembly 2
        with pytest.raises(ValueError):
            markers.local_summary(h, lengths[:-1], n_tar)
    finally:
        h.close()
    h = b.best_hits(queries, K, local=True)
    try:
        with pytest.raises(ValueError):
            markers.local_summary(h, [len(q) for q in queries], 2, best_locus=True)
    finally:
        h.close()


def test_malformed_calls_raise(case):
    b, queries, _ = case
    for bad in ((0, -3, 5, 2), (2, 1, 5, 2), (2, -3, 256, 2), (2, -3, 5, 0)):
        with pytest.raises(ValueError):
            b.best_hits(queries, K, local=True, scoring=bad)
    with pytest.raises(ValueError):
        b.best_hits([b"A" * 65280], K, local=True)
    with pytest.raises(ValueError):
        b.best_hits(queries, K, local=True, seed_copies=257)
    with pytest.raises(ValueError):
        b.best_hits(queries, K, local=True, loci=True, min_seeds=0)
    h = b.best_hits([b"A" * 65279], K, local=True)
    h.close()


def test_markers_best_hits_local():
    """One marker golden through Markers.best_hits(local=True): a representative is cut from a target row, so in the assembly it
    was taken from every representative whose row lies in one valid run scores r * len over the whole query."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
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
        offs, _, inexact = m.sequences(b, "reps")
        lens = np.diff(offs.astype(np.int64))
        h = m.best_hits(b, g["k"], local=True)
        plain = m.best_hits(b, g["k"])
        try:
            for fld in PLAIN:
                assert np.array_equal(getattr(h, fld)(), getattr(plain, fld)()), fld
            reps = m.reps()[0]
            rows = np.flatnonzero(~inexact)
            assert len(rows) > 0
            own = reps["assembly_idx"].astype(np.int64)[rows]
            assert np.array_equal(h.score()[rows, own], 2 * lens[rows])
            assert not h.qstart()[rows, own].any() and np.array_equal(h.qend()[rows, own], lens[rows])
            assert np.array_equal(h.sstart()[rows, own], reps["start"][rows]) and np.array_equal(h.send()[rows, own], reps["stop"][rows])
            got = {fld: getattr(h, meth)() for fld, meth in LOCAL.items()}
            L.check(got, BLASTN)
        finally:
            h.close()
            plain.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
