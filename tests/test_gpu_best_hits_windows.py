"""GPU: Batch.best_hits(pileup=groups, window_lengths=...) / Markers.best_hits(...) -- the winners of csrc/hits.hip classed window by
window by the window walk of csrc/align.hip -- against tests/tools/windows_host.py: best_hits_windows.  Every
field of the hits and the pileup equal the same call without the windows, also with shared seeds, the loci and the local stage; the
table does not depend on how the hit buffer chunks and splits the assemblies (SEQWIN_AMD_HIT_BUFFER_KB).  Where a window is FWD_OK or
REV_OK for an assembly, the exhaustive scan (Batch.oligo_hits) finds that oligo there."""
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
import windows_host as W  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
FIELDS = ("seeds", "record", "strand", "end", "dist", "n_seeds", "start", "nident", "mismatch", "gaps")
GROUPS = list(range(7))                                          # each assembly its own group
LENS, MM, C3 = (18, 20, 22, 25), 2, 3
KW = dict(pileup=GROUPS, window_lengths=LENS, window_mismatch=MM, window_three_prime=C3)


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
    """7 assemblies of ACGT only over one ancestor of 3000 bases, more and more diverged (planted substitutions, insertions,
    deletions, a cluster of five substitutions in assembly 5); assembly 4 holds the reverse complement, assembly 6 nothing of it.
    3 queries: two stretches of the ancestor (one given as its reverse complement) and random text."""
    from seqwin_amd.device import Batch
    rng = random.Random(23)
    anc = _rand(rng, 3000)
    asms = []
    for g in range(6):
        seq = bytearray(anc)
        if g == 5:                                                       # five substitutions within 8 bases of query 0: windows with 4 mismatches and more
            for at in (300, 302, 303, 305, 307):
                seq[at] = b"CGTA"[b"ACGT".index(seq[at])]
        for _ in range(25 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        for _ in range(4 * g):
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
    queries = [anc[100:500], H.revcomp(anc[900:1500]), _rand(rng, 300)]
    d = tmp_path_factory.mktemp("bhw")
    b = Batch.from_fasta([_write(d, f"w{i}.fa", recs) for i, recs in enumerate(asms)], n_cpu=2)
    hits = A.best_hits_aligned(queries, asms, 21)
    want = W.best_hits_windows(queries, asms, 21, GROUPS, 7, LENS, MM, C3, hits=hits)
    yield b, queries, asms, want
    b.close()


def _same_hits(h, plain):
    for f in FIELDS:
        assert np.array_equal(getattr(h, f)(), getattr(plain, f)()), f
    assert np.array_equal(h.pileup().table()[1], plain.pileup().table()[1]) and np.array_equal(h.pileup().depth(), plain.pileup().depth())
    s, s0 = h.pileup().stats(), plain.pileup().stats()
    assert all(s[k] == s0[k] for k in ("piled", "filtered_by_distance", "left_out_by_label", "adds", "table_bytes"))


def _check_table(h, want, lengths=LENS):
    win = h.windows()
    offs, table = win.table()
    assert win.lengths == tuple(lengths) and np.array_equal(offs.astype(np.int64), want["q_offsets"]) and table.shape == want["wtable"].shape
    bad = np.argwhere(table != want["wtable"])
    assert not len(bad), (bad[:5].tolist(), table[tuple(bad[0])], want["wtable"][tuple(bad[0])])
    assert np.array_equal(h.pileup().depth(), want["depth"])
    W.invariants(table, want["depth"], want["q_offsets"], lengths)
    return table, win.stats()


def test_the_batch_covers_its_ground(seven):
    _, queries, _, want = seven
    hit = want["seeds"] > 0
    assert hit[:2, :6].all() and not hit[2].any() and not hit[:, 6].any()
    assert want["strand"][0, 0] == 0 and want["strand"][0, 4] == 1 and want["strand"][1, 0] == 1 and want["strand"][1, 4] == 0
    t = want["wtable"]
    assert all(t[..., c].any() for c in range(8)) and want["depth"].tolist() == [[1] * 6 + [0]] * 2 + [[0] * 7]
    # the ancestor's own assembly matches every window; the most diverged one does not
    assert (t[:400 - 25 + 1, :, 0, W.MM0] == 1).all() and not (t[:400 - 25 + 1, :, 5, W.FWD_OK] == 1).all()
    # the two orientations differ somewhere, and the two host forms agree on this batch
    assert (t[..., W.FWD_OK] != t[..., W.REV_OK]).any()
    loops = W.best_hits_windows(queries, None, 21, GROUPS, 7, LENS, MM, C3, hits=want, form="loops")
    assert np.array_equal(loops["wtable"], t)


def test_windows_of_the_winners(seven):
    b, queries, asms, want = seven
    plain = b.best_hits(queries, 21, pileup=GROUPS)
    h = b.best_hits(queries, 21, **KW)
    try:
        for f in FIELDS:
            assert np.array_equal(getattr(h, f)(), want[f]), f
        _same_hits(h, plain)
        table, st = _check_table(h, want)
        m = np.array([len(q) for q in queries])
        per_query = sum(np.maximum(m - L + 1, 0) for L in LENS)
        assert st["windows"] == int((want["depth"].sum(axis=1) * per_query).sum()) and st["table_bytes"] == table.nbytes
        assert st["adds"] == int(table[..., 1:6].sum()) + int(table[..., 6:].sum()) - 2 * int(table[..., 0].sum())
        assert h.windows().sizes() == (3, int(m.sum()), 7, 4, MM, C3)
        with pytest.raises(ValueError, match="window_lengths"):
            plain.windows()
        from seqwin_amd.pileup import candidate_oligos
        cand, oligos = candidate_oligos(h.windows(), h.pileup(), queries, tar=0, neg=5, min_tar=1.0, max_neg=0.0)
        assert len(cand) and all(len(o) == int(c["length"]) for c, o in zip(cand, oligos))
    finally:
        plain.close()
        h.close()


@pytest.mark.parametrize("kw", [dict(seed_copies=2), dict(loci=True, min_seeds=2), dict(local=True), dict(max_dist_permille=25)])
def test_every_field_and_the_pileup_equal_the_call_without_windows(seven, kw):
    b, queries, asms, want = seven
    plain = b.best_hits(queries, 21, pileup=GROUPS, **kw)
    h = b.best_hits(queries, 21, **KW, **kw)
    try:
        _same_hits(h, plain)
        if "max_dist_permille" in kw:
            filtered = W.best_hits_windows(queries, asms, 21, GROUPS, 7, LENS, MM, C3, kw["max_dist_permille"], hits=want)
            assert 0 < filtered["depth"].sum() < want["depth"].sum()
            _check_table(h, filtered)
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
    h = b.best_hits(queries, 21, **KW)
    try:
        _check_table(h, want)
        s = h.stats()
        assert s["chunks"] > 2
    finally:
        h.close()
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")
    monkeypatch.setenv("SEQWIN_AMD_HIT_MAX_BLOCKS", "1")
    monkeypatch.setenv("SEQWIN_AMD_ALN_SCRATCH_KB", "64")
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    h = b.best_hits(queries, 21, **KW)
    try:
        _check_table(h, want)
        s2 = h.stats()
        # 1 KiB holds 64 hits, far fewer than one assembly's: the chunk of all assemblies is split, and a chunk of one assembly, which
        # cannot be, makes the buffer grow; no hit is lost on the way
        assert s2["chunks"] > 2 and s2["chunk_splits"] > 0 and s2["buffer_doublings"] > 0 and s2["launches"] >= s2["chunks"] and s2["hits"] == st["hits"], s2
    finally:
        h.close()


def test_the_exhaustive_scan_finds_what_the_windows_promise(seven):
    """ACGT-only text, each assembly its own group.  Wherever FWD_OK (REV_OK) of a window is 1 for an assembly, the winner's copy
    faces the window without a gap, with at most MM mismatches and none at the oligo's 3' end: the exhaustive scan of that oligo (of
    its reverse complement) with the same bounds has at least one site in that assembly.  It is an inequality, not an equation: the
    scan sees every locus of the assembly, the windows only the best one."""
    b, queries, asms, want = seven
    l, L = LENS.index(20), 20
    t, offs = want["wtable"], want["q_offsets"]
    promised = 0
    for cls, turn in ((W.FWD_OK, lambda s: s), (W.REV_OK, H.revcomp)):
        rows, oligos = [], []
        for q in (0, 1):
            for u in range(0, len(queries[q]) - L + 1):
                rows.append(int(offs[q]) + u)
                oligos.append(turn(queries[q][u:u + L]))
        o = b.oligo_hits(oligos, max_mismatch=MM, three_prime=C3)
        try:
            n_sites = o.n_sites()
        finally:
            o.close()
        ok = t[rows, l][:, :, cls] == 1                                     # [windows, assemblies]
        assert ok.shape == n_sites.shape and ok[:, :6].any(axis=0).all() and not ok.all()
        assert (n_sites[ok] > 0).all(), np.argwhere(ok & (n_sites == 0))[:5].tolist()
        promised += int(ok.sum())
    assert promised > 1000


def test_malformed_calls_raise(seven):
    b, queries, _, _ = seven
    with pytest.raises(ValueError, match="pileup"):
        b.best_hits(queries, 21, window_lengths=LENS)
    with pytest.raises(ValueError, match="pileup"):
        b.best_hits(queries, 21, align=True, window_lengths=LENS)
    for bad in (dict(window_lengths=(7,)), dict(window_lengths=(20, 20)), dict(window_lengths=()), dict(window_lengths=(20,), window_mismatch=9),
                dict(window_lengths=(8,), window_mismatch=8), dict(window_lengths=(20,), window_three_prime=9)):
        with pytest.raises(ValueError):
            b.best_hits(queries, 21, pileup=GROUPS, **bad)
    h = b.best_hits([], 21, pileup=GROUPS, window_lengths=(20,))
    try:
        assert h.windows().table()[1].shape == (0, 1, 7, 8) and h.windows().stats()["windows"] == 0
    finally:
        h.close()


def test_markers_best_hits_windows():
    """One marker golden through Markers.best_hits(pileup=targets / non-targets, window_lengths=...): the table equals the
    restatement."""
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
        lengths = (25, 18)
        want = W.best_hits_windows(texts, asms, g["k"], groups, 2, lengths, 1, 2)
        h = m.best_hits(b, g["k"], pileup=groups, window_lengths=lengths, window_mismatch=1, window_three_prime=2)
        plain = m.best_hits(b, g["k"], pileup=groups)
        try:
            table, _ = _check_table(h, want, lengths)
            assert table.any()
            for fld in H.FIELDS + ("start", "nident", "mismatch", "gaps"):
                assert np.array_equal(getattr(h, fld)(), want[fld]), fld
            assert np.array_equal(h.pileup().table()[1], plain.pileup().table()[1])
        finally:
            h.close()
            plain.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
