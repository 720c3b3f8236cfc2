"""GPU: the oligo search of csrc/oligo.hip (Batch.oligo_hits) against the host restatement of its specification
(tests/tools/oligo_host.py) on the same text: n_sites, the four best-site fields and the whole site list, exactly.  The scan gives a
lane 16 consecutive window ends and a wave 1024 (one tile), holds the last 32 bases in a 64-bit window and packs 16 bases a word;
oligo lengths, run lengths and planted sites straddle all of these.  seqwin_amd.oligos on top of it: products of primer pairs."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oligo_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
TILE = 1024
NO_HIT = 0xFFFFFFFF
FIELDS = ("n_sites", "best_mm", "best_record", "best_pos", "best_strand")
SITE_FIELDS = ("oligo", "assembly", "record", "pos", "strand", "mm")


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, seq, n):
    s = bytearray(seq)
    for i in rng.sample(range(len(s)), n):
        s[i] = ord("ACGT"["ACGT".index(chr(s[i]).upper()) ^ rng.randrange(1, 4)])
    return bytes(s)


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


def _compare(o, want, n_oligos, n_asm, sites=True):
    """every array of the result `o` against the restatement's `want`, whole; returns (sites dict or None, stats)"""
    for f in FIELDS:
        got = getattr(o, f)()
        assert got.dtype == np.uint32 and got.shape == (n_oligos, n_asm), f
        assert np.array_equal(got, want[f]), f
    st = o.stats()
    assert st["hits"] == int(want["n_sites"].sum())
    if not sites:
        return None, st
    S = o.sites()
    for f in SITE_FIELDS:
        assert S[f].dtype == np.uint32 and np.array_equal(S[f], want["sites"][f]), f
    assert S["cell_offsets"].dtype == np.uint64 and np.array_equal(S["cell_offsets"], want["sites"]["cell_offsets"])
    return S, st


def _check(batch, oligos, assemblies, max_mm, clamp=0, want=None, sites=True):
    want = want if want is not None else H.search(oligos, assemblies, max_mm, clamp)
    o = batch.oligo_hits(oligos, max_mm, clamp, sites=sites)
    try:
        assert o.sizes() == (len(oligos), len(assemblies), max_mm, clamp)
        S, st = _compare(o, want, len(oligos), len(assemblies), sites)
        return want, S, st
    finally:
        o.close()


# ---- lengths, mismatches, the clamp; lower case, U and IUPAC in the assemblies --------------------------------------------------------

@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """4 assemblies over one ancestor of 3000 bases with lower case, U and IUPAC letters in the text (run breaks), and oligos of 8, 15,
    16, 17, 31 and 32 bases cut from it: exact, with 1, 3 and more substitutions, reverse-complemented, and degenerate."""
    rng = random.Random(42)
    anc = _rand(rng, 3000)
    r0 = bytearray(anc[:1800])
    r0[300:301] = b"N"
    r0[1000:1100] = bytes(r0[1000:1100]).lower()
    r0[1500:1503] = b"RYK"
    asms = [[bytes(r0).replace(b"T", b"U", 7), anc[1800:]], [_mutate(rng, anc[500:2500], 60)], [H.revcomp(anc[:1500]), _rand(rng, 400)], [_rand(rng, 1200)]]
    oligos = []
    for i, L in enumerate((8, 15, 16, 17, 31, 32)):
        at = 350 + 190 * i
        oligos += [anc[at:at + L], H.revcomp(_mutate(rng, anc[at + 40:at + 40 + L], 1)), _mutate(rng, anc[at + 80:at + 80 + L], min(3, L // 4))]
    oligos += [b"ACGTNNRY", anc[1495:1515].lower(), anc[600:608] + b"NNNN" + anc[612:620], b"GGWCCYRA", anc[2000:2031].replace(b"A", b"R").replace(b"C", b"Y")]
    b = _batch(tmp_path_factory.mktemp("olmixed"), asms, "m")
    yield b, oligos, asms
    b.close()


@pytest.mark.parametrize("max_mm,clamp", [(0, 0), (1, 0), (1, 1), (3, 5), (3, 1), (0, 5)])
def test_lengths_mismatches_and_clamp(mixed, max_mm, clamp):
    b, oligos, asms = mixed
    assert sorted({len(o) for o in oligos[:18]}) == [8, 15, 16, 17, 31, 32]
    want, S, st = _check(b, oligos, asms, max_mm, clamp)
    assert st["passes"] == 1 and st["chunks"] == 1 and st["launches"] == 1 and st["buffer_doublings"] == 0
    assert st["comparisons"] == st["windows"] * 2 * len(oligos)
    assert want["n_sites"][0, 0] >= 1 and (want["best_mm"][::3, 0][:6] == 0).all()       # every exact oligo lies in assembly 0
    if max_mm >= 1 and clamp == 0:
        assert (want["best_mm"][1:18:3].min(axis=1) <= 1).all() and want["best_strand"][4, 0] == 1


def test_eight_mismatches(mixed):
    """max_mismatch = 8 needs oligos of 9 bases or more: 9, 15, 16, 17, 31 and 32.  Nearly every window holds the 9-mer."""
    b, oligos, asms = mixed
    rng = random.Random(8)
    long = [o for o in oligos[:18] if len(o) > 8] + [_rand(rng, 9), b"ACGTNNRYK"]
    want, S, st = _check(b, long, asms, 8, 1)
    assert want["n_sites"][-2].sum() > 1000
    with pytest.raises(ValueError, match="max_mismatch"):
        b.oligo_hits(oligos, 8)


# ---- run, tile and lane bounds -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lengths", [(8,), (32,), (17,), (8, 17, 32)])
def test_site_placement(tmp_path, lengths):
    """Valid runs of L - 1, L, L + 15, L + 16, 1024 + L - 2, 1024 + L - 1 and 1024 + L bases (L the call's longest oligo), as records and
    as the stretches between single Ns of one record.  Sites planted (the oligo is the text there, one base changed, max_mismatch 1)
    at a run's first and last window, at the last window of a tile and the first of the next, at the last window of a lane and the
    first of the next -- a tile counts window ENDS from the shortest oligo's length on, so for a longer oligo the same bounds are
    also taken at starts shifted by L - Lmin."""
    rng = random.Random(100 + sum(lengths))
    lmin, lmax = min(lengths), max(lengths)
    lens = [lmax - 1, lmax, lmax + 15, lmax + 16, TILE + lmax - 2, TILE + lmax - 1, TILE + lmax]
    runs = [_rand(rng, n) for n in lens]
    long_run = runs[-1]
    asms = [
        [r for r in runs],
        [b"N".join(runs), b"NN" + runs[2] + b"N"],
        [_rand(rng, lmin - 1), _rand(rng, 7), b"N" * 40],      # nothing of Lmin valid bases: a NO_HIT column
        [long_run[1:]],
        [H.revcomp(long_run)],
    ]
    oligos, planted = [], []
    for L in lengths:
        starts = {0, 15, 16, 17, TILE - 1, TILE, TILE + 1, len(long_run) - L, len(long_run) - L - 1}
        starts |= {s - (L - lmin) for s in (16, TILE, 2 * 16) if s - (L - lmin) >= 0}
        for s in sorted(s for s in starts if s + L <= len(long_run)):
            o = bytearray(long_run[s:s + L])
            j = rng.randrange(L)
            o[j] = ord("ACGT"["ACGT".index(chr(o[j])) ^ 1])
            planted.append(len(oligos))
            oligos.append(bytes(o))
        oligos += [runs[1][:L], runs[2][-L:], runs[3][:L], runs[4][-L:], runs[5][:L]]
    b = _batch(tmp_path, asms)
    try:
        want, S, st = _check(b, oligos, asms, 1)
        assert (want["n_sites"][:, 2] == 0).all() and (want["best_mm"][:, 2] == NO_HIT).all() and (want["best_pos"][:, 2] == NO_HIT).all()
        assert (want["n_sites"][:, 0] >= 1).all() and (want["n_sites"][:, 1] >= 1).all()
        assert (want["n_sites"][planted, 4] >= 1).all()        # (assembly 4 holds the long run's reverse complement: strand 1)
        if lmin >= 17:                                         # (an oligo this long has no chance hit)
            assert (want["best_strand"][planted, 4] == 1).all() and (want["best_mm"][planted, 0] == 1).all()
        _check(b, oligos, asms, 0, sites=False)
    finally:
        b.close()


# ---- one strand only, a palindrome, a column without a run ------------------------------------------------------------------------------

def test_strands_and_a_palindrome(tmp_path):
    rng = random.Random(5)
    x = _rand(rng, 25)
    pal = b"ACGTTGCATGCAACGT"                                   # its own reverse complement
    assert H.revcomp(pal) == pal
    asms = [[_rand(rng, 500) + H.revcomp(x) + _rand(rng, 300)], [_rand(rng, 200) + pal + _rand(rng, 100), b"ACGTAC"], [b"ACGTACG", b"NNNNNNNNNNNN"]]
    b = _batch(tmp_path, asms)
    try:
        want, S, _ = _check(b, [x, pal], asms, 0)
        assert want["n_sites"].tolist() == [[1, 0, 0], [0, 2, 0]]
        assert (want["best_strand"][0, 0], want["best_pos"][0, 0]) == (1, 500)              # a site on strand 1 only
        assert S["strand"].tolist() == [1, 0, 1] and S["pos"].tolist() == [500, 200, 200]   # the palindrome: two sites at one place
        assert (want["best_mm"][:, 2] == NO_HIT).all()
    finally:
        b.close()


# ---- the hooks: groups of oligos, the site buffer, the launch split ------------------------------------------------------------------

@pytest.fixture(scope="module")
def five(tmp_path_factory):
    """5 assemblies, one of them with a poly-A stretch of 700 bases; 7 oligos, among them AAAAAAAA (693 exact sites in that stretch)."""
    rng = random.Random(9)
    anc = _rand(rng, 2500)
    asms = [[_mutate(rng, anc, 20 * g)] for g in range(4)]
    asms.insert(2, [_rand(rng, 300) + b"A" * 700 + _rand(rng, 300), anc[:900]])
    oligos = [b"AAAAAAAA", anc[100:120], H.revcomp(anc[700:732]), _mutate(rng, anc[1500:1517], 2), b"ACGTNNRY", anc[2000:2015], anc[2400:2408]]
    b = _batch(tmp_path_factory.mktemp("ol5"), asms, "f")
    want = H.search(oligos, asms, 2, 1)
    yield b, oligos, asms, want
    b.close()


@pytest.mark.parametrize("group", [1, 3])
def test_groups_of_oligos(five, monkeypatch, group):
    b, oligos, asms, want = five
    _, _, st1 = _check(b, oligos, asms, 2, 1, want)
    assert st1["passes"] == 1
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_GROUP", str(group))
    _, _, st = _check(b, oligos, asms, 2, 1, want)
    assert st["passes"] == -(-7 // group) and st["windows"] == st["passes"] * st1["windows"] and st["comparisons"] == st1["comparisons"]
    _check(b, oligos, asms, 2, 1, want, sites=False)


def test_a_small_site_buffer_splits_and_doubles(five, monkeypatch):
    """A budget of 1 KiB holds 128 sites: the 5 assemblies together overflow it and are split into chunks -- a chunk of several
    assemblies is halved, never grown --, and every assembly alone overflows it too: the buffer doubles until it holds the largest,
    the one with the poly-A stretch (693 sites of AAAAAAAA and more).  A budget below one site holds one."""
    b, oligos, asms, want = five
    per_asm = want["n_sites"].sum(axis=0)
    assert want["n_sites"][0, 2] >= 693 and per_asm.argmax() == 2 and per_asm.min() > 128
    doublings = int(np.ceil(np.log2(per_asm.max() / 128)))
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", "1")
    _, _, st = _check(b, oligos, asms, 2, 1, want)
    assert st["chunk_splits"] >= 1 and st["buffer_doublings"] == doublings >= 2 and st["chunks"] >= 3, st
    _, _, st = _check(b, oligos, asms, 2, 1, want, sites=False)      # without the list nothing is buffered
    assert st["chunks"] == 1 and st["chunk_splits"] == 0 and st["buffer_doublings"] == 0
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_GROUP", "3")
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", "0")
    _, _, st = _check(b, oligos[:4], asms, 0, 0)
    assert st["buffer_doublings"] >= 1 and st["passes"] == 2


def test_a_launch_split(five, monkeypatch):
    b, oligos, asms, want = five
    _, _, st1 = _check(b, oligos, asms, 2, 1, want)
    assert st1["launches"] == 1
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_MAX_BLOCKS", "1")
    _, _, st = _check(b, oligos, asms, 2, 1, want)
    assert st["launches"] > 1 and st["windows"] == st1["windows"]


# ---- blocks, sites() without the list, intervals ------------------------------------------------------------------------------------------

def test_blocks_and_sites_without_the_list(five):
    b, oligos, asms, want = five
    o = b.oligo_hits(oligos, 2, 1)
    try:
        nq, na = len(oligos), len(asms)
        for rows, cols in (((0, nq), (0, na)), ((2, 5), (1, 4)), ((6, 7), (0, 1)), ((4, 4), (0, 5)), ((0, 7), (4, 5)), ((3, 6), (2, 2))):
            for f in FIELDS:
                blk = getattr(o, f)(rows, cols)
                assert blk.dtype == np.uint32 and np.array_equal(blk, want[f][rows[0]:rows[1], cols[0]:cols[1]])
        assert np.array_equal(o.n_sites(slice(1, 4), range(2, 5)), want["n_sites"][1:4, 2:5])
        for rows, cols in (((0, nq + 1), (0, 1)), ((0, 1), (0, na + 1)), ((3, 2), (0, 1))):
            with pytest.raises(ValueError, match="outside"):
                o.best_mm(rows, cols)
        with pytest.raises(ValueError, match="sites=True"):
            o.sites()
        with pytest.raises(ValueError, match="sites=True"):
            o.intervals()
    finally:
        o.close()


def test_intervals_through_fetch(five):
    """The fetched text of every hit has exactly `mm` mismatches against the oligo's sets (strand 1: against its reverse complement's)."""
    b, oligos, asms, want = five
    o = b.oligo_hits(oligos, 2, 1, sites=True)
    try:
        S, iv = o.sites(), o.intervals()
        assert len(iv) == len(S["oligo"]) > 700
        offs, blob, inexact = b.fetch(iv)
        assert not inexact.any()
        P = [H.strands(q) for q in oligos]
        for i in range(len(iv)):
            text = blob[int(offs[i]):int(offs[i + 1])].decode()
            sets = P[S["oligo"][i]][S["strand"][i]]
            assert len(text) == len(sets) and sum(c not in s for c, s in zip(text, sets)) == S["mm"][i]
    finally:
        o.close()


# ---- primer pairs -------------------------------------------------------------------------------------------------------------------

def test_amplicons_and_assay_summary(tmp_path):
    """Two targets and two non-targets.  Pair 0 (f0, r0) frames 300 bases in both targets (in target 1 on the other strand: orientation
    `-`), and in non-target 0 only r0's site exists.  Pair 1 (f1, r1) gives two products in target 0 (f1 lies there twice), none in
    target 1, one in non-target 1."""
    from seqwin_amd import oligos as O
    rng = random.Random(77)
    f0, r0, f1, r1 = (_rand(rng, 20), _rand(rng, 22), _rand(rng, 18), _rand(rng, 20))

    def locus(f, r, n):
        return f + _rand(rng, n - len(f) - len(r)) + H.revcomp(r)

    t0 = _rand(rng, 200) + locus(f0, r0, 300) + _rand(rng, 150) + f1 + _rand(rng, 30) + locus(f1, r1, 200) + _rand(rng, 100)
    t1 = _rand(rng, 100) + H.revcomp(locus(_mutate(rng, f0, 1), r0, 300)) + _rand(rng, 200)
    n0 = _rand(rng, 300) + H.revcomp(r0) + _rand(rng, 300)
    n1 = _rand(rng, 50) + locus(f1, _mutate(rng, r1, 2), 250) + _rand(rng, 50)
    asms = [[_rand(rng, 100), t0], [t1], [n0], [n1]]
    oligos, lengths, pairs = [f0, r0, f1, r1], [20, 22, 18, 20], [(0, 1), (2, 3)]
    b = _batch(tmp_path, asms)
    try:
        want = H.search(oligos, asms, 2)
        o = b.oligo_hits(oligos, 2, sites=True)
        try:
            S, _ = _compare(o, want, 4, 4)
            assert o.lengths.tolist() == lengths
            P, n_amp = O.amplicons(o, o.lengths, pairs, 100, 400)
            w_rows, w_n = H.amplicons(S, lengths, pairs, 100, 400, 4)
            assert [tuple(int(P[f][i]) for f in O.AMPLICON_FIELDS) for i in range(len(P["pair"]))] == w_rows
            assert np.array_equal(n_amp, w_n) and n_amp.tolist() == [[1, 1, 0, 0], [2, 0, 0, 1]]
            assert P["orientation"].tolist() == [0, 1, 0, 0, 0] and P["end"][0] - P["start"][0] == 300 and P["mm_f"][1] == 1 and P["mm_r"][4] == 2
            a = O.assay_summary(n_amp, 2)
            assert a["f_tar_amplified"].tolist() == [1.0, 0.5] and a["f_tar_single"].tolist() == [1.0, 0.0] and a["f_neg_amplified"].tolist() == [0.0, 0.5]
            s = O.oligo_summary(o, 2)
            assert s["f_tar"].tolist() == [1.0, 1.0, 0.5, 0.5] and s["f_neg"].tolist() == [0.0, 0.5, 0.5, 0.5]
            assert s["mean_best_mm_tar"].tolist() == [0.5, 0.0, 0.0, 0.0]
        finally:
            o.close()
    finally:
        b.close()


# ---- one marker golden -----------------------------------------------------------------------------------------------------------------

def test_marker_golden_primer_pairs():
    """tests/golden/markers, pan_b_k21_w10: the first 20 bases of every representative and the reverse complement of its last 20 as a
    primer pair, searched with 2 mismatches; everything against the restatement, and every representative's own assembly amplifies."""
    from seqwin_amd import oligos as O
    from seqwin_amd.device import Batch
    sub = {g["name"]: g for g in json.loads((GOLDEN / "subgraphs" / "manifest.json").read_text())["graphs"]}
    c = next(c for c in json.loads((GOLDEN / "markers" / "manifest.json").read_text())["cases"] if c["graph"] == "pan_b_k21_w10" and c["error"] is None)
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
        o64 = offs.astype(np.int64)
        keep = [i for i in range(len(o64) - 1) if o64[i + 1] - o64[i] >= 40 and not inexact[i]][:12]
        assert len(keep) >= 1
        texts = [blob[o64[i]:o64[i + 1]] for i in keep]
        oligos = [x for t in texts for x in (t[:20], H.revcomp(t[-20:]))]
        pairs = [(2 * i, 2 * i + 1) for i in range(len(texts))]
        ro = b.record_offsets()
        asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
        want = H.search(oligos, asms, 2)
        o = b.oligo_hits(oligos, 2, sites=True)
        try:
            S, _ = _compare(o, want, len(oligos), len(asms))
            longest = max(len(t) for t in texts)
            P, n_amp = O.amplicons(o, o.lengths, pairs, 40, longest)
            w_rows, w_n = H.amplicons(S, o.lengths.tolist(), pairs, 40, longest, len(asms))
            assert [tuple(int(P[f][i]) for f in O.AMPLICON_FIELDS) for i in range(len(P["pair"]))] == w_rows and np.array_equal(n_amp, w_n)
            own = m.reps()[0]["assembly_idx"].astype(np.int64)[keep]
            assert (n_amp[np.arange(len(texts)), own] >= 1).all()
        finally:
            o.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
