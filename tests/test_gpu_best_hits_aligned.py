"""GPU: Batch.best_hits(align=True) / Markers.best_hits(align=True) -- the traceback of every chunk's winners (csrc/align.hip) behind
the seed vote and the infix distance of csrc/hits.hip.  The five fields of best_hits stay what they are without align; start, nident,
mismatch and gaps equal the host restatement (tests/tools/align_host.py) run on the window of DESIGN.md section 3.2e, also when the hit
buffer is chunked and split (SEQWIN_AMD_HIT_BUFFER_KB) and the scratch takes several rounds (SEQWIN_AMD_ALN_SCRATCH_KB)."""
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

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
NONE = 0xFFFFFFFF
NEW = ("start", "nident", "mismatch", "gaps")


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


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


def _fields(h):
    got = dict(seeds=h.seeds(), record=h.record(), strand=h.strand(), end=h.end(), dist=h.dist(), n_seeds=h.n_seeds())
    got.update(start=h.start(), nident=h.nident(), mismatch=h.mismatch(), gaps=h.gaps())
    return got


def _check(batch, queries, want, k=21):
    """align=True against the restatement, and its five old fields against align=False; returns (fields, align_stats)."""
    plain = batch.best_hits(queries, k)
    h = batch.best_hits(queries, k, align=True)
    try:
        got = _fields(h)
        for f in ("n_seeds",) + H.FIELDS:
            assert np.array_equal(got[f], getattr(plain, f)()), f
            assert got[f].dtype == want[f].dtype and np.array_equal(got[f], want[f]), f
        for f in NEW:
            assert got[f].dtype == np.uint32 and got[f].shape == want[f].shape, f
            assert np.array_equal(got[f], want[f]), (f, got[f].tolist(), want[f].tolist())
        assert h.sizes() == plain.sizes() and h.stats()["pairs_aligned"] == plain.stats()["pairs_aligned"]
        st = h.align_stats()
        assert st["pairs"] == int((want["seeds"] > 0).sum())
        hit = want["seeds"] > 0
        assert np.all(got["mismatch"][hit] + got["gaps"][hit] == got["dist"][hit])
        for f in NEW:
            assert np.all(got[f][~hit] == NONE), f
        return got, st
    finally:
        plain.close()
        h.close()


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """tests/test_gpu_best_hits.py's `four` with edits of every kind: 4 assemblies of two records over one ancestor, each with a few
    substitutions, insertions and deletions; 7 queries (one reverse-complemented, one random, one shorter than k)."""
    rng = random.Random(9)
    anc = _rand(rng, 6000)
    asms = []
    for g in range(4):
        seq = bytearray(anc)
        for _ in range(30 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        for _ in range(6 * g):
            at = rng.randrange(len(seq))
            if rng.random() < 0.5:
                del seq[at]
            else:
                seq[at:at] = _rand(rng, rng.randint(1, 3))
        asms.append([bytes(seq[:3500]), bytes(seq[3500:]) + _rand(rng, 200)])
    queries = [anc[i * 1000 + 50:i * 1000 + 650] for i in range(4)] + [H.revcomp(anc[4500:5300]), _rand(rng, 300), anc[10:20]]
    b = _batch(tmp_path_factory.mktemp("aln4"), asms, "n")
    want = A.best_hits_aligned(queries, asms, 21)
    yield b, queries, asms, want
    b.close()


def test_aligned_fields(four):
    b, queries, asms, want = four
    got, st = _check(b, queries, want)
    assert st["rounds"] == 1 and st["striped_pairs"] == 0 and (got["gaps"][want["seeds"] > 0] > 0).any()
    assert np.all(got["seeds"][5] == 0) and np.all(got["start"][5:] == NONE)


def test_votes_aligned(tmp_path):
    """The vote cases of tests/test_gpu_best_hits.py::test_votes: copies at a record's start and end, split by an N run, clipped,
    records shorter than the query, no hit."""
    rng = random.Random(77)
    k = 21
    q = _rand(rng, 300)
    q2 = _rand(rng, 150)
    indel = q[:150] + b"ACG" + q[150:]
    lead = 64 * 5 + 63 - (300 - k)
    asms = [
        [_rand(rng, lead) + indel + _rand(rng, 200)],
        [_rand(rng, 90) + q + _rand(rng, 40), _rand(rng, 10) + H.revcomp(q) + _rand(rng, 70)],
        [_rand(rng, 500) + q[:140] + b"N" * 20 + q[160:] + _rand(rng, 300)],
        [q + _rand(rng, 400)],
        [_rand(rng, 400) + q],
        [q[40:200], _rand(rng, 30)],
        [_rand(rng, 1000)],
        [_rand(rng, 300) + H.revcomp(q)[:250], q[100:] + _rand(rng, 5), q2[10:]],
    ]
    want = A.best_hits_aligned([q, q2], asms, k)
    b = _batch(tmp_path, asms)
    try:
        got, _ = _check(b, [q, q2], want, k)
    finally:
        b.close()
    assert (got["start"][0, 0], got["nident"][0, 0], got["mismatch"][0, 0], got["gaps"][0, 0]) == (lead, 300, 0, 3)
    assert (got["start"][0, 1], got["nident"][0, 1]) == (90, 300)
    assert (got["nident"][0, 2], got["mismatch"][0, 2], got["gaps"][0, 2]) == (280, 20, 0)
    assert got["start"][0, 3] == 0 and got["start"][0, 4] == 400 and got["end"][0, 4] == 700
    assert (got["nident"][0, 5], got["gaps"][0, 5], got["start"][0, 5], got["end"][0, 5]) == (160, 140, 0, 160)
    assert got["start"][0, 6] == NONE and got["gaps"][0, 6] == NONE


def test_chunks_splits_and_rounds(four, monkeypatch):
    b, queries, asms, want = four
    h = b.best_hits(queries, 21)
    per = h.stats()["hits"] // 4
    h.close()
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(max(1, (per * 16 * 5 // 4) // 1024)))   # holds one assembly, not two
    _, st = _check(b, queries, want)
    assert st["rounds"] == 4
    monkeypatch.setenv("SEQWIN_AMD_ALN_SCRATCH_KB", "64")
    _, st = _check(b, queries, want)
    assert st["rounds"] > 4
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", "4")
    _, st = _check(b, queries, want)
    assert st["striped_pairs"] > 0


def test_accessors_need_align(four):
    b, queries, _, want = four
    h = b.best_hits(queries, 21)
    try:
        for f in NEW + ("intervals", "align_stats"):
            with pytest.raises(ValueError, match="align"):
                getattr(h, f)()
        from seqwin_amd._lib import c_u64, lib
        out = np.zeros(1, np.uint32)
        assert lib.sw_hits_align_block(h._h, c_u64(0), c_u64(0), c_u64(1), c_u64(0), c_u64(1), out.ctypes.data) == 2   # SW_ERR_VALUE
        assert np.array_equal(h.dist(), want["dist"])
    finally:
        h.close()
    h = b.best_hits(queries, 21, align=True)
    try:
        assert np.array_equal(h.start((1, 4), (2, 4)), want["start"][1:4, 2:4]) and h.gaps((2, 2), (0, 4)).shape == (0, 4)
        with pytest.raises(ValueError, match="outside"):
            h.nident((0, 9), (0, 1))
    finally:
        h.close()


def test_intervals_fetch_and_replay(four):
    """intervals() hands Batch.fetch the located copies; the script of every hit, traced again on the window of section 3.2e,
    replays to that text."""
    b, queries, asms, want = four
    h = b.best_hits(queries, 21, align=True)
    try:
        iv, rows, cols = h.intervals()
        hit = want["seeds"] > 0
        assert len(iv) == int(hit.sum()) and np.array_equal(np.stack([rows, cols]), np.stack(np.nonzero(hit)))
        assert np.array_equal(iv["start"], want["start"][hit]) and np.array_equal(iv["stop"], want["end"][hit]) and np.array_equal(iv["record"], want["record"][hit])
        offs, blob, _ = b.fetch(iv)
        o = offs.astype(np.int64)
        pairs = [(q, int(want["strand"][q, a]), int(want["record"][q, a]), int(want["lo"][q, a]), int(want["hi"][q, a])) for q, a in zip(rows, cols)]
        res = b.infix_alignments(queries, pairs, ops=True)
        so = res[6].astype(np.int64)
        for x, (q, a) in enumerate(zip(rows.tolist(), cols.tolist())):
            ops = res[7][so[x]:so[x + 1]]
            assert np.array_equal(ops, want["scripts"][(q, a)])
            pat = H._text(queries[q])
            assert A.replay_matches(H._rc(pat) if want["strand"][q, a] else pat, ops, H._text(blob[o[x]:o[x + 1]]))
        sub_iv, r2, c2 = h.intervals((1, 3), (2, 4))
        keep = (rows >= 1) & (rows < 3) & (cols >= 2)
        assert np.array_equal(sub_iv, iv[keep]) and np.array_equal(r2, rows[keep]) and np.array_equal(c2, cols[keep])
    finally:
        h.close()


def test_alignment_summary(four):
    from seqwin_amd.markers import alignment_summary
    b, queries, _, want = four
    lengths = [len(q) for q in queries]
    h = b.best_hits(queries + [b""], 21, align=True)
    try:
        s = alignment_summary(h, lengths + [0], 2)
        ni, ed = h.nident().astype(np.float64), h.mismatch().astype(np.float64) + h.gaps().astype(np.float64)
        hit = h.nident() != NONE
        for q, m in enumerate(lengths):
            assert s["identity_tar"][q] == np.where(hit[q, :2], ni[q, :2], 0).sum() / m / 2
            assert s["distance_neg"][q] == np.where(hit[q, 2:], ed[q, 2:], 0).sum() / m / 2
            assert s["f_tar"][q] == hit[q, :2].sum() / 2 and s["f_neg"][q] == hit[q, 2:].sum() / 2
        assert all(np.isnan(s[f][-1]) for f in s.dtype.names)
        assert s["identity_tar"][0] > 0.9 and s["identity_tar"][5] == 0 and np.isnan(alignment_summary(h, lengths + [0], 0)["identity_tar"]).all()
        with pytest.raises(ValueError):
            alignment_summary(h, lengths, 2)
    finally:
        h.close()


def test_markers_best_hits_aligned():
    """One marker golden through Markers.best_hits(align=True).  A representative is cut from a target row: in the assembly it was
    taken from, every representative whose row lies in one valid run is found whole -- nident == len, no mismatch, no gap, and
    [start, end) the row's interval.  Everything else equals the restatement."""
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
        offs, blob, inexact = m.sequences(b, "reps")
        o = offs.astype(np.int64)
        texts = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        ro = b.record_offsets()
        asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
        want = A.best_hits_aligned(texts, asms, g["k"])
        h = m.best_hits(b, g["k"], align=True)
        try:
            got = _fields(h)
            for fld in H.FIELDS + NEW:
                assert np.array_equal(got[fld], want[fld]), fld
            reps = m.reps()[0]
            rows = np.flatnonzero(~inexact)
            assert len(rows) > 0
            own = reps["assembly_idx"].astype(np.int64)[rows]
            assert np.all(own < c["n_tar"])
            lens = np.array([len(t) for t in texts])[rows]
            assert np.array_equal(got["nident"][rows, own], lens) and not got["gaps"][rows, own].any() and not got["mismatch"][rows, own].any()
            assert np.array_equal(got["start"][rows, own], reps["start"][rows]) and np.array_equal(got["end"][rows, own], reps["stop"][rows])
            assert np.array_equal(got["record"][rows, own], ro[own] + reps["record_idx"][rows])
        finally:
            h.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
