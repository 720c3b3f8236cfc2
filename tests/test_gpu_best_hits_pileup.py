"""GPU: Batch.best_hits(pileup=groups) / Markers.best_hits(pileup=groups) -- the winners of csrc/hits.hip piled by the pile walk of
csrc/align.hip, labelled by their assembly -- against tests/tools/pileup_host.py: best_hits_pileup.  Every
field of the hits equals the same call without the pileup, also with shared seeds and with the loci; the table does not depend on
how the hit buffer chunks and splits the assemblies (SEQWIN_AMD_HIT_BUFFER_KB)."""
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
import pileup_host as P  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
FIELDS = ("seeds", "record", "strand", "end", "dist", "n_seeds", "start", "nident", "mismatch", "gaps")
GROUPS = [0, 0, 0, 1, 1, P.LEAVE_OUT, 1]


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


@pytest.fixture(scope="module")
def seven(tmp_path_factory):
    """7 assemblies over one ancestor of 3000 bases, more and more diverged (substitutions, insertions, deletions, an N); assembly 4
    holds the reverse complement, assembly 6 nothing of it.  4 queries: three stretches of the ancestor (one given as its reverse
    complement) and random text.  Groups: three targets, three non-targets, one assembly left out."""
    from seqwin_amd.device import Batch
    rng = random.Random(19)
    anc = _rand(rng, 3000)
    asms = []
    for g in range(6):
        seq = bytearray(anc)
        for _ in range(25 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGTN" if g == 3 else b"ACGT")
        for _ in range(5 * g):
            at = rng.randrange(len(seq))
            if rng.random() < 0.5:
                del seq[at:at + rng.randint(1, 2)]
            else:
                seq[at:at] = _rand(rng, rng.randint(1, 3))
        seq = bytes(seq)
        if g == 4:
            seq = H.revcomp(seq)
        asms.append([seq[:1700], seq[1700:] + _rand(rng, 100)])
    asms.append([_rand(rng, 2000)])
    queries = [anc[100:500], H.revcomp(anc[900:1500]), anc[2000:2350], _rand(rng, 300)]
    d = tmp_path_factory.mktemp("bhp")
    b = Batch.from_fasta([_write(d, f"p{i}.fa", recs) for i, recs in enumerate(asms)], n_cpu=2)
    hits = A.best_hits_aligned(queries, asms, 21)
    want = P.best_hits_pileup(queries, asms, 21, GROUPS, 2, hits=hits)
    yield b, queries, asms, want
    b.close()


def _fields(h):
    return {f: getattr(h, f)() for f in FIELDS}


def _same_hits(h, plain):
    for f in FIELDS:
        assert np.array_equal(getattr(h, f)(), getattr(plain, f)()), f


def _check_table(h, want):
    pile = h.pileup()
    offs, table = pile.table()
    assert np.array_equal(offs.astype(np.int64), want["q_offsets"]) and table.shape == want["table"].shape
    bad = np.argwhere(table != want["table"])
    assert not len(bad), (bad[:5].tolist(), table[tuple(bad[0])], want["table"][tuple(bad[0])])
    assert np.array_equal(pile.depth(), want["depth"])
    return table, pile.stats()


def test_the_batch_covers_its_ground(seven):
    _, queries, _, want = seven
    hit = want["seeds"] > 0
    assert hit[:3, :6].all() and not hit[3].any() and not hit[:, 6].any()
    assert (want["strand"][0, :4] == 0).all() and want["strand"][0, 4] == 1 and want["strand"][1, 0] == 1 and want["strand"][1, 4] == 0
    t = want["table"]
    assert t[:, :, P.DEL].any() and t[:, :, P.INS].any() and t[:, :, P.N_].any() and t[:, 0].any() and t[:, 1].any()
    assert want["depth"].tolist() == [[3, 2], [3, 2], [3, 2], [0, 0]]
    # targets are closer to the ancestor than non-targets: there are positions that tell them apart
    from seqwin_amd.pileup import diagnostic_positions, consensus
    assert len(diagnostic_positions((want["q_offsets"], t), queries, min_tar=1.0, max_neg=0.5)) > 0
    assert consensus(t[:400, 0]) == queries[0].decode()


def test_pileup_of_the_winners(seven):
    b, queries, asms, want = seven
    plain = b.best_hits(queries, 21, align=True)
    h = b.best_hits(queries, 21, pileup=GROUPS)
    try:
        got = _fields(h)
        for f in FIELDS:
            assert np.array_equal(got[f], want[f]), f
        _same_hits(h, plain)
        table, st = _check_table(h, want)
        assert st["piled"] == 15 and st["left_out_by_label"] == 3 and st["filtered_by_distance"] == 0
        assert st["adds"] == int(table[:, :, :6].sum()) + 2 * int(table[:, :, P.INS].sum()) and st["table_bytes"] == table.nbytes
        hit = want["seeds"] > 0
        k = hit & (np.array(GROUPS) != P.LEAVE_OUT)[None, :]
        n_i = sum(int((want["scripts"][(q, a)] == 2).sum()) for q, a in zip(*np.nonzero(k)))
        n_d = sum(int((want["scripts"][(q, a)] == 3).sum()) for q, a in zip(*np.nonzero(k)))
        P.invariants(table, h.pileup().depth(), want["q_offsets"], got["nident"][k].sum(), got["mismatch"][k].sum(), n_i, n_d)
        with pytest.raises(ValueError, match="pileup"):
            plain.pileup()
    finally:
        plain.close()
        h.close()


def test_the_distance_filter(seven):
    b, queries, asms, want = seven
    rel = want["dist"][:3, :5].astype(np.int64) * 1000 // np.array([len(q) for q in queries[:3]])[:, None]
    permille = int(np.sort(rel.ravel())[7])                              # some winners inside, some outside
    filtered = P.best_hits_pileup(queries, asms, 21, GROUPS, 2, permille, hits=want)
    assert 0 < filtered["depth"].sum() < want["depth"].sum()
    h = b.best_hits(queries, 21, pileup=GROUPS, max_dist_permille=permille)
    try:
        _, st = _check_table(h, filtered)
        assert st["filtered_by_distance"] == int(want["depth"].sum() - filtered["depth"].sum())
        for f in FIELDS:
            assert np.array_equal(getattr(h, f)(), want[f]), f
    finally:
        h.close()


@pytest.mark.parametrize("kw", [dict(seed_copies=2), dict(loci=True, min_seeds=2), dict(local=True), dict(n_groups=8)])
def test_every_field_equals_the_call_without_the_pileup(seven, kw):
    b, queries, asms, want = seven
    call = {k: v for k, v in kw.items() if k != "n_groups"}
    plain = b.best_hits(queries, 21, align=True, **call)
    h = b.best_hits(queries, 21, pileup=GROUPS, **kw)
    try:
        _same_hits(h, plain)
        if "n_groups" in kw:
            offs, table = h.pileup().table()
            assert table.shape[1] == 8 and np.array_equal(table[:, :2], want["table"]) and not table[:, 2:].any()
        else:
            _check_table(h, want)                                        # (two copies of a seed, loci and the local stage change no winner here)
        if "loci" in kw:
            L, Lp = h.loci(), plain.loci()
            assert all(np.array_equal(L[f], Lp[f]) for f in Lp) and np.array_equal(h.n_loci(), plain.n_loci()) and np.array_equal(h.sum_nident(), plain.sum_nident())
        if "local" in kw:
            assert np.array_equal(h.score(), plain.score()) and np.array_equal(h.sstart(), plain.sstart()) and np.array_equal(h.local_gaps(), plain.local_gaps())
    finally:
        plain.close()
        h.close()


def test_chunks_and_splits(seven, monkeypatch):
    b, queries, asms, want = seven
    h = b.best_hits(queries, 21)
    st = h.stats()
    h.close()
    assert st["chunks"] == 1
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(max(1, (st["hits"] // 6 * 16 * 5 // 4) // 1024)))   # holds one assembly, not two
    h = b.best_hits(queries, 21, pileup=GROUPS)
    try:
        _check_table(h, want)
        s = h.stats()
        assert s["chunks"] > 2 and s["chunk_splits"] > 0
    finally:
        h.close()
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")
    monkeypatch.setenv("SEQWIN_AMD_ALN_SCRATCH_KB", "64")
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    h = b.best_hits(queries, 21, pileup=GROUPS)
    try:
        _check_table(h, want)
    finally:
        h.close()


def test_malformed_calls_raise(seven):
    b, queries, _, _ = seven
    with pytest.raises(ValueError):
        b.best_hits(queries, 21, pileup=GROUPS[:-1])
    with pytest.raises(ValueError, match="group label"):
        b.best_hits(queries, 21, pileup=[0, 1, 2, 0, 0, 0, 0], n_groups=2)
    with pytest.raises(ValueError, match="1..8"):
        b.best_hits(queries, 21, pileup=GROUPS, n_groups=0)
    with pytest.raises(ValueError, match="0..1000"):
        b.best_hits(queries, 21, pileup=GROUPS, max_dist_permille=2000)
    h = b.best_hits([], 21, pileup=GROUPS)
    try:
        assert h.pileup().table()[1].shape == (0, 2, 8) and h.pileup().depth().shape == (0, 2)
    finally:
        h.close()


def test_markers_best_hits_pileup():
    """One marker golden through Markers.best_hits(pileup=targets / non-targets): the table equals the restatement, and in the group
    of the targets every representative cut from one valid run sees its own bases at least once at every position."""
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
        groups = [0 if a < c["n_tar"] else 1 for a in range(len(asms))]
        want = P.best_hits_pileup(texts, asms, g["k"], groups, 2)
        h = m.best_hits(b, g["k"], pileup=groups)
        try:
            table, _ = _check_table(h, want)
            for fld in H.FIELDS + ("start", "nident", "mismatch", "gaps"):
                assert np.array_equal(getattr(h, fld)(), want[fld]), fld
            from seqwin_amd.pileup import match_fraction
            frac = match_fraction(h.pileup(), texts)
            rows = np.flatnonzero(~inexact)
            assert len(rows) > 0
            for q in rows:
                assert (frac[o[q]:o[q + 1], 0] > 0).all(), q
        finally:
            h.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
