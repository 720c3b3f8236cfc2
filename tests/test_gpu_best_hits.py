"""GPU: Layer B of csrc/hits.hip -- Batch.best_hits, Markers.best_hits: seeds, the vote and the winner's infix distance -- against
the host restatement (tests/tools/hits_host.py) on the same text: n_seeds and every seeds, record, strand, end and dist, exactly and
whole.  A band holds 64 implied end positions and a vote adds a band and the next; the window reaches 64 before and 192 + m behind
the band's start; the hit buffer is chunked, split and doubled under SEQWIN_AMD_HIT_BUFFER_KB."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import hits_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
KS = [1, 2, 4, 15, 16, 17, 21, 31, 32]
NONE = 0xFFFFFFFF


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


def _compare(h, want, nq, na, k):
    got = dict(seeds=h.seeds(), record=h.record(), strand=h.strand(), end=h.end(), dist=h.dist(), n_seeds=h.n_seeds())
    for f in ("n_seeds",) + H.FIELDS:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
        assert np.array_equal(got[f], want[f]), (f, got[f].tolist(), want[f].tolist())
    assert h.sizes() == (nq, na, int(want["n_seeds"].sum()), k)
    return got


def _check(batch, queries, assemblies, k, want=None):
    """best_hits of `queries`, everything compared with the restatement; returns (fields, stats)."""
    want = want if want is not None else H.best_hits(queries, assemblies, k)
    h = batch.best_hits(queries, k)
    try:
        got = _compare(h, want, len(queries), len(assemblies), k)
        st = h.stats()
        assert st["seeds"] == int(want["n_seeds"].sum()) and st["pairs_aligned"] == int((want["seeds"] > 0).sum())
        assert sum(st["chunk_hits"]) == st["hits"] and len(st["chunk_hits"]) == st["chunks"]
        return got, st
    finally:
        h.close()


def _run(tmp_path, queries, asms, k, want=None):
    b = _batch(tmp_path, asms)
    try:
        return _check(b, queries, asms, k, want)
    finally:
        b.close()


# ---- k sweep ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_k_sweep(tmp_path, k):
    """Assemblies as tests/test_gpu_screen.py::test_k_sweep builds them: an N, a run of N, lower case, IUPAC codes, U, and a
    reverse-complemented assembly; queries shorter than k, of exactly k, all N, with an N, with u."""
    rng = random.Random(k)
    anc = _rand(rng, 4000)
    r0 = bytearray(anc[:2500])
    r0[300:301] = b"N"
    r0[700:700 + k] = b"N" * k
    r0[1000:1100] = bytes(r0[1000:1100]).lower()
    r0[1500:1503] = b"RYK"
    asms = [[bytes(r0).replace(b"T", b"U", 5), anc[2500:]], [_rand(rng, 3000)], [anc[1000:3500], _rand(rng, 500)], [H.revcomp(anc[:2000])]]
    queries = [anc[100:100 + 3 * k + 40], H.revcomp(anc[2400:2600 + k]), _rand(rng, 200), anc[690:720 + 2 * k].lower(), anc[2490:2510 + k],
               anc[10:10 + k - 1], anc[10:10 + k], anc[10:10 + k + 1], b"N" * (k + 3), anc[3000:3000 + k] + b"N" + anc[3000 + k:3000 + 2 * k],
               anc[3500:3600].replace(b"T", b"u").decode()]
    got, st = _run(tmp_path, queries, asms, k)
    assert got["n_seeds"][5] == 0 and got["n_seeds"][8] == 0 and st["chunks"] <= 1
    if k >= 15:
        # (queries 6 and 7 share their first k-mer, which is therefore no seed: 7 keeps its second)
        assert got["n_seeds"][6] == 0 and got["n_seeds"][7] == 1 and got["dist"][0, 0] == 0 and got["strand"][0, 3] == 1 and got["dist"][0, 3] == 0
        assert got["strand"][1, 0] == 1 and got["dist"][1, 0] > 0 and got["dist"][1, 2] == 0         # spans asm 0's two records: not whole there
        assert np.all(got["seeds"][8] == 0) and np.all(got["dist"][8] == NONE) and np.all(got["seeds"][:, 1] == 0)


# ---- seeds -----------------------------------------------------------------------------------------------------------------------

def test_shared_and_repeated_kmers_are_no_seeds(tmp_path):
    rng = random.Random(2)
    k, a, b_, c = 21, _rand(rng, 100), _rand(rng, 60), _rand(rng, 100)
    rep = _rand(rng, 40)
    queries = [a + b_, b_ + c, rep + _rand(rng, 30) + rep, H.revcomp(b_)]
    asms = [[_rand(rng, 50) + a + b_ + c + _rand(rng, 50) + rep + _rand(rng, 80)]]
    got, _ = _run(tmp_path, queries, asms, k)
    # the shared stretch b_ carries no seed: only windows that reach into a (or c) do; the repeat's inner windows neither
    assert got["n_seeds"].tolist() == [100, 100, 2 * 40 + 30 - k + 1 - 2 * (40 - k + 1), 0]
    assert np.all(got["seeds"][3] == 0) and got["dist"][0, 0] == 0 and got["dist"][1, 0] == 0


def test_a_palindromic_kmer_is_no_seed(tmp_path):
    queries = [b"TTACGTCC", b"GGGATCAAA"]                  # ACGT and GATC are their own reverse complements
    asms = [[b"CCCCACGTCCCCC"], [b"AAAATTACGTCCAAAA", b"TTTGATCCC"]]
    got, _ = _run(tmp_path, queries, asms, 4)
    want = H.best_hits_literal(queries, asms, 4)
    for f in H.FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert got["n_seeds"].tolist() == [4, 5]


# ---- the vote ----------------------------------------------------------------------------------------------------------------------

def test_votes(tmp_path):
    """One assembly per situation, k = 21, one query of 300 bases cut from an ancestor (and a second of 150)."""
    rng = random.Random(77)
    k = 21
    q = _rand(rng, 300)
    q2 = _rand(rng, 150)
    indel = q[:150] + b"ACG" + q[150:]                     # the halves' implied ends lie 3 apart
    lead = 64 * 5 + 63 - (300 - k)                         # the first half's e = lead + (m - k): the last place of band 5; the second half's in band 6
    asms = [
        [_rand(rng, lead) + indel + _rand(rng, 200)],                                        # 0 straddles a multiple of 64: b and b + 1 add up
        [_rand(rng, 90) + q + _rand(rng, 40), _rand(rng, 10) + H.revcomp(q) + _rand(rng, 70)],  # 1 equal scores, two records and strands: the first
        [_rand(rng, 500) + q[:140] + b"N" * 20 + q[160:] + _rand(rng, 300)],                 # 2 split by an N run: one locus
        [q + _rand(rng, 400)],                                                               # 3 a copy at the record's start
        [_rand(rng, 400) + q],                                                               # 4 ... and at its end
        [q[40:200], _rand(rng, 30)],                                                         # 5 records shorter than the query
        [_rand(rng, 1000)],                                                                  # 6 no hit
        [_rand(rng, 300) + H.revcomp(q)[:250], q[100:] + _rand(rng, 5), q2[10:]],            # 7 clipped copies on either strand
    ]
    got, st = _run(tmp_path, [q, q2], asms, k)
    e = lead + 300 - k                                     # p - i + (m - k) of the first half's windows
    assert e % 64 == 63
    assert got["seeds"][0, 0] == 2 * (150 - k + 1) and got["dist"][0, 0] == 3 and got["end"][0, 0] == lead + 303
    assert got["record"][0, 1] == 1 and got["strand"][0, 1] == 0 and got["dist"][0, 1] == 0 and got["end"][0, 1] == 390
    assert got["seeds"][0, 2] == (140 - k + 1) + (140 - k + 1) and got["dist"][0, 2] == 20
    assert got["dist"][0, 3] == 0 and got["end"][0, 3] == 300 and got["dist"][0, 4] == 0 and got["end"][0, 4] == 700
    assert got["dist"][0, 5] == 140 and got["seeds"][0, 6] == 0 and got["dist"][0, 6] == NONE and got["strand"][0, 6] == 0
    assert got["dist"][1, 7] == 10 and got["record"][1, 7] == 11 and np.all(got["seeds"][1, :7] == 0)
    assert st["chunk_splits"] == 0 and st["chunks"] == 1 and st["striped_pairs"] == 0


def test_zero_queries_and_queries_without_seeds(tmp_path):
    rng = random.Random(3)
    asms = [[_rand(rng, 3000)], [_rand(rng, 1500), _rand(rng, 20)]]
    b = _batch(tmp_path, asms)
    try:
        h = b.best_hits([], 21)
        assert h.seeds().shape == (0, 2) and h.dist().shape == (0, 2) and h.n_seeds().shape == (0,) and h.sizes() == (0, 2, 0, 21)
        assert h.stats()["chunks"] == 0
        h.close()
        for queries in ([b"N" * 100], [b"ACGTACGT"], [b"", b"NNNN", b"ACGT" * 5]):
            got, st = _check(b, queries, asms, 21)
            assert not got["seeds"].any() and st["hits"] == 0
        for k in (0, 33):
            with pytest.raises(ValueError, match="1..32"):
                b.best_hits([b"ACGT"], k)
    finally:
        b.close()


# ---- run and lane bounds -------------------------------------------------------------------------------------------------------------

TILE = 1024   # k-mers per wave of the batch walk (csrc/kmer_walk.hpp)


def _bounds_case(k):
    """(queries, assemblies, restatement's result, what was added to every query).  Assembly 0, record 0: valid runs of k - 1, k,
    k + 15, k + 16, 1024 + k - 2, 1024 + k - 1 and 1024 + k bases between single Ns (0, 1, 16, 17, 1023, 1024 and 1025 k-mers: a
    lane's share and a tile's, one below and one above).  Record 1: sixteen runs, run j starting j places behind a multiple of 16
    in the record, so that a run starts at each of the 16 places of a packed word.  Assembly 1: the long run without its first base,
    every k-mer one lane place on.  Queries of k bases: the long run's first k-mer, the last of its first tile, its last (the first of
    its second tile), and the first k-mer of each of the sixteen runs.  A query without a seed (k = 5: short words repeat in the query
    text) grows by a base of its run until the restatement finds one."""
    rng = random.Random(2000 + k)
    runs = [_rand(rng, n) for n in (k - 1, k, k + 15, k + 16, TILE + k - 2, TILE + k - 1, TILE + k)]
    long_run = runs[-1]
    aligned, rec1 = [], bytearray()
    for j in range(16):
        rec1 += b"N" if j else b""
        rec1 += b"N" * ((j - len(rec1)) % 16)
        aligned.append((len(rec1), _rand(rng, k + 20 + j)))
        rec1 += aligned[-1][1]
    assert sorted(p % 16 for p, _ in aligned) == list(range(16))
    asms = [[b"N".join(runs), bytes(rec1)], [long_run[1:]]]
    # [run, first base, bases]; the long run's last k-mer grows towards the front, the others towards the back
    spec = [[long_run, 0, k], [long_run, TILE - 1, k], [long_run, TILE, k]] + [[run, 0, k] for _, run in aligned]
    while True:
        queries = [run[s:s + n] for run, s, n in spec]
        want = H.best_hits(queries, asms, k)
        short = np.flatnonzero(want["n_seeds"] == 0)
        if not len(short):
            break
        for q in short:
            run, s, n = spec[q]
            assert n < len(run) - 1, "the run is used up"
            spec[q][1] = s - 1 if q == 2 else s
            spec[q][2] = n + 1
    return queries, asms, want, [n - k for _, _, n in spec], aligned


@pytest.mark.parametrize("k", [21, 5, 32])
def test_run_and_lane_bounds(tmp_path, k):
    """tests/test_gpu_screen.py::test_run_and_lane_bounds for the best hits, which walk the batch with the same code: hits at a
    run's first k-mer, at the last of its first tile, at its last -- the only one of its second tile --, and at the first k-mer
    of runs that start at each of the 16 places of a packed word (_bounds_case).  On the host, when the case was made: every query
    has a seed at every k; at k = 21 and 32 every (query, assembly) has one run of the best score; at k = 5 a word of five bases
    lies in an assembly several times, twelve cells have 2 to 11 runs of the best score and the smallest key wins, as specified."""
    queries, asms, want, grown, aligned = _bounds_case(k)
    assert (want["n_seeds"] > 0).all() and (want["seeds"][:, 0] > 0).all()   # no query passes on an empty seed set
    got, st = _run(tmp_path, queries, asms, k, want)
    assert st["hits"] >= len(queries)
    if k >= 15:   # (random k-mers of this length do not repeat: every query is one seed, found where it was cut)
        long_at = len(asms[0][0]) - (TILE + k)
        assert not any(grown) and got["n_seeds"].tolist() == [1] * len(queries)
        assert got["seeds"][:, 0].tolist() == [1] * len(queries) and not got["dist"][:, 0].any() and not got["strand"][:, 0].any()
        assert got["record"][:, 0].tolist() == [0] * 3 + [1] * 16
        assert got["end"][:, 0].tolist() == [long_at + k, long_at + TILE - 1 + k, long_at + TILE + k] + [p + k for p, _ in aligned]
        # assembly 1 holds the long run from its second base on: not its first k-mer, the others one place earlier
        assert got["seeds"][:, 1].tolist() == [0, 1, 1] + [0] * 16 and got["end"][1:3, 1].tolist() == [TILE - 2 + k, TILE - 1 + k]
        assert got["record"][1:3, 1].tolist() == [2, 2]


# ---- the hooks ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """4 assemblies of two records over one ancestor with a few substitutions each, 6 queries (one reverse-complemented, one
    random)."""
    rng = random.Random(9)
    anc = _rand(rng, 6000)
    asms = []
    for g in range(4):
        seq = bytearray(anc)
        for _ in range(30 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([bytes(seq[:3500]), bytes(seq[3500:]) + _rand(rng, 200)])
    queries = [anc[i * 1000 + 50:i * 1000 + 650] for i in range(4)] + [H.revcomp(anc[4500:5300]), _rand(rng, 300)]
    b = _batch(tmp_path_factory.mktemp("hit4"), asms, "n")
    want = H.best_hits(queries, asms, 21)
    yield b, queries, asms, want
    b.close()


def test_the_buffer_splits_chunks_and_doubles(four, monkeypatch):
    b, queries, asms, want = four
    _, st = _check(b, queries, asms, 21, want)
    assert st["chunks"] == 1 and st["chunk_splits"] == 0 and st["buffer_doublings"] == 0 and st["launches"] == 1
    per = st["hits"] // 4                                   # about the hits of one assembly (8 bytes a key, twice for the sort)
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(max(1, (per * 16 * 5 // 4) // 1024)))   # holds one assembly, not two
    _, st2 = _check(b, queries, asms, 21, want)
    assert st2["chunks"] == 4 and st2["chunk_splits"] >= 2 and st2["hits"] == st["hits"] and st2["buffer_doublings"] == 0, st2
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(max(1, (per * 16 * 5 // 2) // 1024)))   # holds two, not four
    _, st3 = _check(b, queries, asms, 21, want)
    assert st3["chunks"] == 2 and st3["chunk_splits"] == 1, st3
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")     # 64 keys: below one assembly, the buffer doubles
    _, st4 = _check(b, queries, asms, 21, want)
    assert st4["chunks"] == 4 and st4["buffer_doublings"] >= 1 and st4["buffer_keys"] >= max(st4["chunk_hits"]), st4


def test_a_launch_split(four, monkeypatch):
    b, queries, asms, want = four
    monkeypatch.setenv("SEQWIN_AMD_HIT_MAX_BLOCKS", "1")
    _, st = _check(b, queries, asms, 21, want)
    assert st["launches"] > 4


def test_the_smallest_table(four, monkeypatch):
    b, queries, asms, want = four
    h = b.best_hits(queries, 21)
    d = h.stats()["distinct_kmers"]
    h.close()
    monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(d.bit_length()))
    _check(b, queries, asms, 21, want)


def test_blocks(four):
    b, queries, asms, want = four
    h = b.best_hits(queries, 21)
    try:
        assert np.array_equal(h.dist((1, 4), (2, 4)), want["dist"][1:4, 2:4]) and np.array_equal(h.end(slice(0, 2), range(1, 3)), want["end"][0:2, 1:3])
        assert h.seeds((2, 2), (0, 4)).shape == (0, 4)
        with pytest.raises(ValueError, match="outside"):
            h.record((0, 7), (0, 1))
    finally:
        h.close()


# ---- Markers.best_hits -------------------------------------------------------------------------------------------------------------

def test_markers_best_hits():
    from seqwin_amd.device import Batch
    from seqwin_amd.markers import hit_summary
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
        assert len(texts) > 0
        ro = b.record_offsets()
        asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
        want = H.best_hits(texts, asms, g["k"])
        h = m.best_hits(b, g["k"])
        try:
            got = _compare(h, want, len(texts), len(asms), g["k"])
            reps = m.reps()[0]
            own = reps["assembly_idx"].astype(np.int64)
            rows = np.arange(len(texts))
            assert np.all(got["dist"][rows, own] == 0)      # every representative is found in the assembly it was taken from
            s = hit_summary(h, [len(t) for t in texts], c["n_tar"])
            assert s.shape == (len(texts),) and np.all(s["similarity_tar"] > 0)
        finally:
            h.close()
        pick = [len(texts) - 1, 0]
        h, direct = m.best_hits(b, 21, select=pick), b.best_hits([texts[i] for i in pick], 21)
        assert np.array_equal(h.dist(), direct.dist()) and np.array_equal(h.seeds(), direct.seeds())
        h.close()
        direct.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
