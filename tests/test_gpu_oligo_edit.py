"""GPU: the oligo search with indels (Batch.oligo_hits(max_edits=), csrc/oligo.hip) against the host
restatement of its specification (tests/tools/oligo_edit_host.py) on the same text: n_sites, the seven best-site fields and the whole
site list, exactly.  The scan gives a lane 16 consecutive ends and a wave 1024 (one tile), keeps up to 59 bases a lane in 64-bit
planes and warms its column up L + 2 d bases before the first end; sites are planted at all of these bounds."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oligo_edit_host as E  # noqa: E402
import oligo_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
TILE = 1024
NO_HIT = 0xFFFFFFFF
BEST = {"best_dist": "best_dist", "best_record": "best_record", "best_pos": "best_pos", "best_strand": "best_strand", "best_end": "best_end",
        "best_mismatch": "best_mismatch", "best_gaps": "best_gaps"}


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


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
    got = o.n_sites()
    assert got.dtype == np.uint32 and got.shape == (n_oligos, n_asm) and np.array_equal(got, want["n_sites"])
    for f, meth in BEST.items():
        got = getattr(o, meth)()
        assert got.dtype == np.uint32 and got.shape == (n_oligos, n_asm), f
        assert np.array_equal(got, want[f]), f
    st = o.stats()
    assert st["hits"] == st["candidates"] == int(want["n_sites"].sum())
    if not sites:
        return None, st
    S = o.sites()
    for f in E.SITE_FIELDS:
        assert S[f].dtype == np.uint32 and np.array_equal(S[f], want["sites"][f]), f
    assert "mm" not in S
    assert S["cell_offsets"].dtype == np.uint64 and np.array_equal(S["cell_offsets"], want["sites"]["cell_offsets"])
    return S, st


def _check(batch, oligos, assemblies, d, clamp=0, want=None, sites=True):
    want = want if want is not None else E.search(oligos, assemblies, d, clamp)
    o = batch.oligo_hits(oligos, three_prime=clamp, sites=sites, max_edits=d)
    try:
        assert o.sizes() == (len(oligos), len(assemblies), 0, clamp) and o.max_edits == d
        S, st = _compare(o, want, len(oligos), len(assemblies), sites)
        return want, S, st
    finally:
        o.close()


def _edit(rng, seq, kind):
    """one edit in the middle third of an oligo: `del` (the text has a base more: a text bulge), `ins` (an oligo bulge), `sub`"""
    s = bytearray(seq)
    i = rng.randrange(len(s) // 3, 2 * len(s) // 3)
    if kind == "del":
        del s[i]
    elif kind == "ins":
        s.insert(i, rng.choice(b"ACGT"))
    else:
        s[i] = ord("ACGT"["ACGT".index(chr(s[i])) ^ 2])
    return bytes(s)


# ---- lane, tile and run bounds; three lengths in one call --------------------------------------------------------------------------

LMIN = 8
EDITS = (0, 1, 2, 4)                                              # the max_edits of test_placed_sites


def _bounds(d):
    """(strand-0 ends, strand-1 starts) at the scan's bounds for max_edits = d: a lane owns the places first .. first + 15 of a tile of
    1024, a place p is the end p + k on strand 0 (k = LMIN - d) and the start p on strand 1: the last place of a lane and the first
    of the next, the last of a tile and the first of the next"""
    places = (15, 16, TILE - 1, TILE)
    return {p + LMIN - d for p in places}, set(places)


def _placed_data():
    """One run of 1024 + 70 bases, alone, between Ns, shifted and reverse-complemented; runs of 4..7 bases (Lmin - d .. Lmin - 1 for
    Lmin = 8) and of 8..40.  Oligos of 8, 17 and 32 (one edit may make them 7..33: kept inside 8..32) cut so that their sites lie at
    the lane and tile bounds of `_bounds` for every d of EDITS -- on strand 0 by their END, on strand 1 (reverse-complemented) by
    their START --, within L + d of the run's start and at its last base, each with a deleted, an inserted or a changed base in its
    middle third, which moves neither that end nor that start; degenerate letters; a palindrome."""
    rng = random.Random(2024)
    long_run = _rand(rng, TILE + 70)
    n = len(long_run)
    small = [_rand(rng, x) for x in (4, 5, 6, 7, 8, 9, 12, 16, 17, 33, 40)]
    pal = b"ACGTTGCATGCAACGT"
    asms = [
        [long_run],
        [b"N".join(small) + b"N" + long_run[:300] + b"NN" + long_run[300:700], b"n" + long_run[5:90] + b"R"],
        [H.revcomp(long_run), _rand(rng, 200) + pal + _rand(rng, 100)],
        [small[0][:3], b"AC", b"NNNN"],                           # nothing of Lmin - 4 valid bases: a NO_HIT column
        [long_run[1:600] + long_run[601:]],                       # the long run with one base deleted
    ]
    oligos = []
    kinds = ["del", "ins", "sub"]
    bound_ends = sorted(set().union(*(_bounds(d)[0] for d in EDITS)))
    bound_starts = sorted(_bounds(0)[1])
    for L in (8, 17, 32):
        text_len = {"del": L + 1 if L == 8 else L, "ins": L - 1 if L == 32 else L, "sub": L}   # (the edited oligo stays inside 8..32)
        for x, e in enumerate(bound_ends + [L, L + 1, L + 3, n, n - 1, 600 + L // 2]):
            kind = kinds[x % 3]
            if e - text_len[kind] >= 0:
                oligos.append(_edit(rng, long_run[e - text_len[kind]:e], kind))
        for x, st in enumerate(bound_starts):
            kind = kinds[x % 3]
            oligos.append(_edit(rng, H.revcomp(long_run[st:st + text_len[kind]]), kind))
        oligos.append(long_run[TILE - L:TILE])
    wide = bytearray(long_run[200:236])                           # 36 bases of text less 4 of them: a 32-mer whose site spans 36
    for i in (30, 22, 13, 5):
        del wide[i]
    oligos += [bytes(wide), b"ACGTNNRY", long_run[500:520].replace(b"A", b"R").replace(b"C", b"Y"), pal, H.revcomp(long_run[40:72]), b"GGWCCYRAK"]
    assert {len(o) for o in oligos} >= {8, 17, 32} and all(8 <= len(o) <= 32 for o in oligos) and min(len(o) for o in oligos) == LMIN
    return oligos, asms


@pytest.fixture(scope="module")
def placed(tmp_path_factory):
    oligos, asms = _placed_data()
    b = _batch(tmp_path_factory.mktemp("oleplaced"), asms, "p")
    yield b, oligos, asms
    b.close()


@pytest.mark.parametrize("d,clamp", [(0, 0), (1, 0), (1, 5), (2, 3), (4, 0), (4, 3)])
def test_placed_sites(placed, d, clamp):
    b, oligos, asms = placed
    assert d in EDITS
    o_len = np.array([len(o) for o in oligos])
    want, S, st = _check(b, oligos, asms, d, clamp)
    assert st["passes"] == 1 and st["chunks"] == 1 and st["launches"] == 1 and st["dp_steps"] > st["comparisons"]
    assert (want["n_sites"][:, 3] == 0).all() and (want["best_dist"][:, 3] == NO_HIT).all() and (want["best_end"][:, 3] == NO_HIT).all()
    if d >= 1:
        assert (S["gaps"] > 0).any() and (S["mismatch"] > 0).any() and (S["strand"] == 1).any()
        one = (S["assembly"] == 0) & (S["dist"] == 1) & (o_len[S["oligo"]] >= 16)      # (a planted site of a 17- or 32-mer, edited: no chance hit)
        ends, starts = _bounds(d)
        assert ends | {TILE + 70} <= set(S["end"][one & (S["strand"] == 0)].tolist())
        assert starts <= set(S["pos"][one & (S["strand"] == 1)].tolist())
    if d == 4 and clamp == 0:
        span = S["end"] - S["pos"]
        assert span.max() == 36 and span.min() == 4                # a 32-mer over 36 bases: more than one 32-bit plane; an 8-mer over 4
    _check(b, oligos, asms, d, clamp, want, sites=False)


def test_no_edits_equals_no_mismatches(placed):
    """max_edits = 0 is max_mismatch = 0, bit for bit, with end = pos + L, mismatch = 0, gaps = 0"""
    import ctypes
    from seqwin_amd._lib import lib
    b, oligos, asms = placed
    for clamp in (0, 3):
        o0 = b.oligo_hits(oligos, 0, clamp, sites=True)
        o1 = b.oligo_hits(oligos, three_prime=clamp, sites=True, max_edits=0)
        try:
            S0, S1 = o0.sites(), o1.sites()
            assert len(S0["oligo"]) > 20
            for f in ("oligo", "assembly", "record", "pos", "strand", "end", "dist", "mismatch", "gaps", "cell_offsets"):
                assert S0[f].dtype == S1[f].dtype and np.array_equal(S0[f], S1[f]), f
            assert np.array_equal(S1["end"], S1["pos"] + o1.lengths[S1["oligo"]]) and not S1["dist"].any()
            for f in ("n_sites", "best_dist", "best_record", "best_pos", "best_strand", "best_end", "best_mismatch", "best_gaps"):
                assert np.array_equal(getattr(o0, f)(), getattr(o1, f)()), f
            assert np.array_equal(o0.best_mm(), o1.best_dist())
            # the list's new accessor on the Hamming result: end = pos + L, mismatch = mm, gaps = 0
            n = len(S0["oligo"])
            offs = np.empty(len(S0["cell_offsets"]), np.uint64)
            cols = {f: np.empty(n, np.uint32) for f in ("oligo", "assembly", "record", "pos", "strand", "end", "mismatch", "gaps")}
            vp = ctypes.c_void_p
            assert lib.sw_oligos_sites_edit(o0._h, offs.ctypes.data_as(vp), *[c.ctypes.data_as(vp) for c in cols.values()]) == 0
            assert np.array_equal(offs, S0["cell_offsets"]) and all(np.array_equal(cols[f], S0[f]) for f in cols)
            assert np.array_equal(cols["mismatch"], S0["mm"]) and "mm" not in S1
            with pytest.raises(ValueError, match="best_dist"):
                o1.best_mm()
        finally:
            o0.close()
            o1.close()


def test_strands_and_a_palindrome(tmp_path):
    rng = random.Random(5)
    x = _rand(rng, 25)
    pal = b"ACGTTGCATGCAACGT"
    bulged = x[:12] + b"G" + x[12:]
    asms = [[_rand(rng, 500) + H.revcomp(bulged) + _rand(rng, 300)], [_rand(rng, 200) + pal + _rand(rng, 100), b"ACGTAC"], [b"ACGTACG", b"NNNNNNNNNNNN"]]
    b = _batch(tmp_path, asms)
    try:
        want, S, _ = _check(b, [x, pal], asms, 1)
        assert want["n_sites"].tolist() == [[1, 0, 0], [0, 2, 0]]
        assert (want["best_strand"][0, 0], want["best_pos"][0, 0], want["best_end"][0, 0], want["best_gaps"][0, 0]) == (1, 500, 526, 1)
        assert S["strand"].tolist() == [1, 0, 1] and S["pos"].tolist() == [500, 200, 200] and S["end"].tolist() == [526, 216, 216]
    finally:
        b.close()


# ---- the hooks -------------------------------------------------------------------------------------------------------------------------

def _five_data():
    rng = random.Random(9)
    anc = _rand(rng, 2500)
    asms = [[bytes(anc[:700 + 100 * g]) + _rand(rng, 30) + anc[701 + 100 * g:]] for g in range(4)]
    asms.insert(2, [_rand(rng, 300) + b"A" * 700 + _rand(rng, 300), anc[:900]])
    oligos = [b"AAAAAAAAA", anc[100:120], H.revcomp(anc[700:732]), _edit(rng, anc[1500:1517], "del"), b"ACGTNNRY", _edit(rng, anc[2000:2015], "ins"), anc[2400:2408]]
    return oligos, asms


@pytest.fixture(scope="module")
def five(tmp_path_factory):
    oligos, asms = _five_data()
    b = _batch(tmp_path_factory.mktemp("ole5"), asms, "f")
    want = E.search(oligos, asms, 2, 1)
    yield b, oligos, asms, want
    b.close()


@pytest.mark.parametrize("group", [1, 3])
def test_groups_of_oligos(five, monkeypatch, group):
    b, oligos, asms, want = five
    _, _, st1 = _check(b, oligos, asms, 2, 1, want)
    assert st1["passes"] == 1
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_GROUP", str(group))
    _, _, st = _check(b, oligos, asms, 2, 1, want)
    assert st["passes"] == -(-7 // group) and st["comparisons"] == st1["comparisons"] and st["dp_steps"] == st1["dp_steps"]
    _check(b, oligos, asms, 2, 1, want, sites=False)


def test_a_small_buffer_splits_and_doubles(five, monkeypatch):
    """1 KiB holds 128 candidates: the five assemblies together overflow it (halved), and every one of them alone does too (doubled)"""
    b, oligos, asms, want = five
    per_asm = want["n_sites"].sum(axis=0)
    assert per_asm.min() > 256
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", "1")
    for sites in (True, False):                                   # the candidates are buffered with or without the list
        _, _, st = _check(b, oligos, asms, 2, 1, want, sites=sites)
        assert st["chunk_splits"] >= 1 and st["buffer_doublings"] >= 2 and st["chunks"] >= 2, st
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_GROUP", "3")
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", "0")
    _, _, st = _check(b, oligos[:4], asms, 1, 0)
    assert st["buffer_doublings"] >= 1 and st["passes"] == 2


def test_a_launch_split(five, monkeypatch):
    b, oligos, asms, want = five
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_MAX_BLOCKS", "1")
    _, _, st = _check(b, oligos, asms, 2, 1, want)
    assert st["launches"] > 1


# ---- intervals through fetch -------------------------------------------------------------------------------------------------------------

def _ed_sets(P, text):
    """global unit-cost edit distance of a list of sets and a text"""
    prev = list(range(len(text) + 1))
    for i, s in enumerate(P, 1):
        cur = [i]
        for j, ch in enumerate(text, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ch not in s)))
        prev = cur
    return prev[-1]


def test_intervals_through_fetch(five):
    """the fetched text of every site, re-aligned on the host end to end, gives back dist (strand 1: its reverse complement)"""
    b, oligos, asms, _ = five
    o = b.oligo_hits(oligos, sites=True, max_edits=2)
    try:
        S, iv = o.sites(), o.intervals()
        assert len(iv) == len(S["oligo"]) > 300 and np.array_equal(iv["stop"], S["end"]) and np.array_equal(iv["start"], S["pos"])
        offs, blob, inexact = b.fetch(iv)
        assert not inexact.any()
        P = [E.sets_of(q) for q in oligos]
        for i in range(len(iv)):
            text = blob[int(offs[i]):int(offs[i + 1])]
            text = (H.revcomp(text) if S["strand"][i] else bytes(text)).decode()
            assert _ed_sets(P[S["oligo"][i]], text) == S["dist"][i] == S["mismatch"][i] + S["gaps"][i]
    finally:
        o.close()


# ---- the marker golden: two primer pairs, one site bulged by hand ---------------------------------------------------------------------------

def test_marker_golden_pairs_with_a_bulged_site(tmp_path):
    """tests/golden/markers, pan_b_k21_w10: the ends of a representative as two primer pairs (20-mers, and the 18-mers nested in them);
    a copy of its own assembly with one base deleted inside the forward primers' site joins the batch.  With max_edits = 1 the copy amplifies, its product one
    base shorter; with max_mismatch = 2 it does not."""
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
    b2 = None
    try:
        offs, blob, inexact = m.sequences(b, "reps")
        o64 = offs.astype(np.int64)
        keep = [i for i in range(len(o64) - 1) if o64[i + 1] - o64[i] >= 40 and not inexact[i]][:1]
        assert len(keep) == 1
        texts = [bytes(blob[o64[i]:o64[i + 1]]) for i in keep]
        t = texts[0]
        oligos = [t[:20], H.revcomp(t[-20:]), t[:18], H.revcomp(t[-18:])]
        pairs = [(0, 1), (2, 3)]
        ro = b.record_offsets()
        asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
        own = int(m.reps()[0]["assembly_idx"][keep[0]])
        copy = [bytes(r) for r in asms[own]]
        hit = [(ri, r.upper().find(texts[0])) for ri, r in enumerate(copy) if texts[0] in r.upper()]
        hit += [(ri, r.upper().find(H.revcomp(texts[0]))) for ri, r in enumerate(copy) if H.revcomp(texts[0]) in r.upper()]
        ri, at = hit[0]
        fwd = texts[0] in copy[ri].upper()
        cut = at + 10 if fwd else at + len(texts[0]) - 10             # the tenth base of the forward primer's site
        copy[ri] = copy[ri][:cut] + copy[ri][cut + 1:]
        asms.append(copy)
        b2 = Batch.from_fasta([GOLDEN / p for p in g["paths"]] + [_write(tmp_path, "bulged.fa", copy)])
        want = E.search(oligos, asms, 1)
        o = b2.oligo_hits(oligos, sites=True, max_edits=1)
        try:
            S, _ = _compare(o, want, 4, len(asms))
            longest = max(len(t) for t in texts)
            P, n_amp = O.amplicons(o, o.lengths, pairs, 30, longest)
            assert n_amp[0, own] >= 1 and n_amp[0, -1] >= 1 and n_amp[1, own] >= 1 and n_amp[1, -1] >= 1
            last = (P["pair"] == 0) & (P["assembly"] == len(asms) - 1)
            assert (P["end"][last] - P["start"][last]).tolist() == [len(texts[0]) - 1]
            assert want["best_gaps"][0, -1] == 1 and want["best_dist"][0, -1] == 1 and want["best_dist"][0, own] == 0
        finally:
            o.close()
        o = b2.oligo_hits(oligos, 2, sites=True)
        try:
            assert o.n_sites()[0, -1] == 0 and O.amplicons(o, o.lengths, pairs, 30, longest)[1][0, -1] == 0
        finally:
            o.close()
    finally:
        for x in (b2, m, kept, sg, f, ix, b):
            if x is not None:
                x.close()


# ---- the refusals reach the library too ---------------------------------------------------------------------------------------------------

def test_refusals(placed):
    b, oligos, asms = placed
    for kw in (dict(max_edits=5), dict(max_edits=-1), dict(max_edits=4, three_prime=4), dict(max_edits=1, max_mismatch=1), dict(max_edits=1.5)):
        with pytest.raises(ValueError):
            b.oligo_hits(oligos, **kw)
    import ctypes
    from seqwin_amd._lib import lib
    offs = np.array([0, 8], np.uint64)
    h = ctypes.c_void_p()
    for d, c in ((5, 0), (4, 4)):
        rc = lib.sw_batch_oligo_hits_edit(b._h, offs.ctypes.data_as(ctypes.c_void_p), b"ACGTACGT", ctypes.c_uint64(1), ctypes.c_uint64(d), ctypes.c_uint64(c),
                                          ctypes.c_int(0), ctypes.c_void_p(0), ctypes.byref(h))
        assert rc != 0 and not h.value
