"""GPU: best hits with seeds shared between queries (Batch.best_hits(..., seed_copies=c); k_hit_probe_shared and the owner lists of
csrc/hits.hip) against the host restatement (tests/tools/shared_seeds_host.py): n_seeds and every seeds,
record, strand, end and dist, exactly and whole.  The align and loci fields have no restatement that takes owner lists (align_host /
loci_host start from hits_host's unique seeds), so their yardstick is the duplication identity: a query set given twice at c = 2
answers, in both halves, what the set given once answers by default -- and c = 1 equals the default bit for bit in every mode."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import hits_host as H  # noqa: E402
import shared_seeds_host as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
NONE = 0xFFFFFFFF
TILE = 1024   # k-mers per wave of the batch walk (csrc/kmer_walk.hpp)
MATRIX = ("seeds", "record", "strand", "end", "dist")
ALIGN = ("start", "nident", "mismatch", "gaps")
MODES = [dict(), dict(align=True), dict(loci=True, min_seeds=1), dict(loci=True, min_seeds=2)]


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


def _fields(h, mode=None):
    """Everything a result of `mode` answers, as arrays; the handle is closed."""
    mode = mode or {}
    try:
        got = {f: getattr(h, f)() for f in MATRIX + ("n_seeds",)}
        if mode.get("align") or mode.get("loci"):
            got.update({f: getattr(h, f)() for f in ALIGN})
        if mode.get("loci"):
            got.update(n_loci=h.n_loci(), sum_nident=h.sum_nident())
            got.update({"loci_" + f: a for f, a in h.loci().items()})
        got["_stats"], got["_seed_stats"], got["_sizes"] = h.stats(), h.seed_stats(), h.sizes()
        return got
    finally:
        h.close()


def _same(a, b, what=""):
    assert sorted(a) == sorted(b), what
    for f in a:
        if not f.startswith("_"):
            assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), (what, f, a[f].tolist(), b[f].tolist())


def _check(batch, queries, asms, k, c, want=None, literal=False):
    """best_hits at the cap c, n_seeds and the matrix fields compared whole with the restatement; returns the fields."""
    want = want if want is not None else S.best_hits_shared(queries, asms, k, c)
    if literal:
        lit = S.best_hits_shared_literal(queries, asms, k, c)
        for f in MATRIX + ("n_seeds",):
            assert np.array_equal(lit[f], want[f]), f
    got = _fields(batch.best_hits(queries, k, seed_copies=c))
    for f in ("n_seeds",) + MATRIX:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, f
        assert np.array_equal(got[f], want[f]), (f, got[f].tolist(), want[f].tolist())
    st, ss = got["_stats"], got["_seed_stats"]
    assert got["_sizes"] == (len(queries), len(asms), int(want["n_seeds"].sum()), k)
    assert st["seeds"] == int(want["n_seeds"].sum()) and st["pairs_aligned"] == int((want["seeds"] > 0).sum())
    assert sum(st["chunk_hits"]) == st["hits"] == ss["hits"] and len(st["chunk_hits"]) == st["chunks"]
    host = S.seed_stats(queries, k, c)
    assert {f: ss[f] for f in host} == host
    return got


# ---- 1, 2: the duplication identity; c = 1 is the default ---------------------------------------------------------------------------

def _dup_case(k):
    """Queries and assemblies in the manner of tests/test_gpu_best_hits.py::test_k_sweep: assemblies that hold the ancestor exactly
    (with an N, lower case, U), with 3 substitutions and 1 insertion inside every query's place, reverse-complemented, and not at
    all; queries of up to 200 bases cut from the ancestor, one reverse-complemented, one random, one shorter than k."""
    rng = random.Random(100 + k)
    anc = _rand(rng, 3000)
    r0 = bytearray(anc[:1800])
    r0[1700:1701] = b"N"
    r0[1400:1450] = bytes(r0[1400:1450]).lower()
    cuts = [(100, 100 + 3 * k + 40), (400, 600), (900, 1080), (2000, 2150)]
    mut = bytearray(anc)
    for lo, hi in reversed(cuts):
        for x in (lo + 20, (lo + hi) // 2, hi - 20):
            mut[x] = ord("ACGT"[("ACGT".index(chr(mut[x])) + 1) % 4])
        mut[lo + 40:lo + 40] = b"G"
    asms = [[bytes(r0).replace(b"T", b"U", 5), anc[1800:]], [bytes(mut)], [H.revcomp(anc[:2500]), _rand(rng, 300)], [_rand(rng, 2000)]]
    queries = [anc[lo:hi] for lo, hi in cuts]
    queries[1] = H.revcomp(queries[1])
    queries += [_rand(rng, 150), anc[10:10 + k - 1]]
    return queries, asms


@pytest.fixture(scope="module", params=[21, 15, 8])
def dup(request, tmp_path_factory):
    k = request.param
    queries, asms = _dup_case(k)
    b = _batch(tmp_path_factory.mktemp(f"dup{k}"), asms, "d")
    yield b, queries, asms, k
    b.close()


@pytest.mark.parametrize("mode", MODES, ids=["plain", "align", "loci1", "loci2"])
def test_a_query_set_given_twice(dup, mode):
    """best_hits(Q + Q, seed_copies=2): either half equals best_hits(Q) row for row, in every field of the mode; the loci lists
    after the query index is mapped.  Plain, at k >= 15, the result is also the restatement's and finds the planted copies."""
    b, queries, asms, k = dup
    n, na = len(queries), len(asms)
    one = _fields(b.best_hits(queries, k, **mode), mode)
    two = _fields(b.best_hits(queries + queries, k, seed_copies=2, **mode), mode)
    assert one["_seed_stats"]["seed_copies"] == 0 and two["_seed_stats"]["seed_copies"] == 2
    assert two["_seed_stats"]["seed_windows"] == 2 * one["_seed_stats"]["seed_windows"] and two["_stats"]["hits"] == 2 * one["_stats"]["hits"]
    assert one["n_seeds"].sum() > 0 and (one["seeds"] > 0).any()
    for f in one:
        if f.startswith("_") or f.startswith("loci_"):
            continue
        assert two[f].dtype == one[f].dtype and np.array_equal(two[f][:n], one[f]) and np.array_equal(two[f][n:], one[f]), f
    if mode.get("loci"):
        q2 = two["loci_query"]
        cells = np.diff(one["loci_cell_offsets"].astype(np.int64))
        assert np.array_equal(np.diff(two["loci_cell_offsets"].astype(np.int64)), np.concatenate([cells, cells]))
        for half in (0, 1):
            sel = (q2 >= n) == bool(half)
            for f in one:
                if f.startswith("loci_") and f != "loci_cell_offsets":
                    a = two[f][sel] - (n * half if f == "loci_query" else 0)
                    assert a.dtype == one[f].dtype and np.array_equal(a, one[f]), (half, f)
        assert len(one["loci_query"]) > 0
    if not mode and k >= 15:
        _check(b, queries + queries, asms, k, 2)
        assert np.all(one["dist"][:4, 0] == 0) and np.all(one["dist"][:4, 1] == 4) and np.all(one["dist"][[0, 2], 2] == 0) and one["strand"][0, 2] == 1
        assert not one["seeds"][:, 3].any()


def test_twice_by_default_is_still_no_seed(dup):
    b, queries, asms, k = dup
    got = _fields(b.best_hits(queries + queries, k))
    assert not got["n_seeds"].any() and not got["seeds"].any() and np.all(got["dist"] == NONE) and got["_seed_stats"]["seed_copies"] == 0
    assert got["_seed_stats"]["seed_words"] == 0 and got["_seed_stats"]["dropped_windows"] > 0


@pytest.mark.parametrize("mode", MODES, ids=["plain", "align", "loci1", "loci2"])
def test_a_cap_of_one_is_the_default(dup, mode):
    b, queries, asms, k = dup
    one, c1 = _fields(b.best_hits(queries, k, **mode), mode), _fields(b.best_hits(queries, k, seed_copies=1, **mode), mode)
    _same(one, c1, "c = 1")
    assert c1["_seed_stats"]["seed_copies"] == 1 and one["_seed_stats"]["seed_copies"] == 0
    strip = lambda d: {f: v for f, v in d.items() if f != "seed_copies"}   # noqa: E731
    assert strip(c1["_seed_stats"]) == strip(one["_seed_stats"]) and c1["_stats"]["hits"] == one["_stats"]["hits"]


@pytest.fixture(scope="module")
def four(tmp_path_factory):
    """The shape of tests/test_gpu_best_hits.py's `four`: 4 assemblies of two records over one ancestor with a few substitutions
    each, 6 queries (one reverse-complemented, one random)."""
    rng = random.Random(9)
    anc = _rand(rng, 6000)
    asms = []
    for g in range(4):
        seq = bytearray(anc)
        for _ in range(30 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([bytes(seq[:3500]), bytes(seq[3500:]) + _rand(rng, 200)])
    queries = [anc[i * 1000 + 50:i * 1000 + 650] for i in range(4)] + [H.revcomp(anc[4500:5300]), _rand(rng, 300)]
    b = _batch(tmp_path_factory.mktemp("hit4s"), asms, "n")
    yield b, queries, asms
    b.close()


def test_a_cap_of_one_is_the_default_on_four(four):
    b, queries, asms = four
    for mode in (MODES[0], MODES[2]):
        _same(_fields(b.best_hits(queries, 21, **mode), mode), _fields(b.best_hits(queries, 21, seed_copies=1, **mode), mode))


def test_a_cap_of_one_is_the_default_on_a_marker_golden():
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
        mode = dict(align=True)
        one, c1 = _fields(m.best_hits(b, g["k"], **mode), mode), _fields(m.best_hits(b, g["k"], seed_copies=1, **mode), mode)
        _same(one, c1)
        assert one["n_seeds"].sum() > 0
        h = m.best_hits(b, g["k"], seed_copies=4)           # the summaries take such a result unchanged
        lens = np.diff(m.sequences(b, "reps")[0].astype(np.int64))
        s = hit_summary(h, lens, c["n_tar"])
        assert s.shape == (len(lens),) and h.seed_stats()["seed_copies"] == 4 and int(h.n_seeds().sum()) >= int(one["n_seeds"].sum())
        h.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()


# ---- 3: the cap -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 5])
def test_the_cap(tmp_path, k):
    """Segments of k + 4 bases (5 windows) that the text of three queries holds once, twice, three and four times, between Ns (no
    window spans two segments).  At the cap c exactly the words with at most c windows seed."""
    rng = random.Random(300 + k)
    a1, a2, a3, a4 = (_rand(rng, k + 4) for _ in range(4))
    queries = [b"N".join([a1, a2, a3, a4]), b"N".join([a2, a3, a4, a4]), b"N".join([a3, a4])]
    asms = [[_rand(rng, 300) + a1 + _rand(rng, 50) + a2 + _rand(rng, 50) + a3 + _rand(rng, 50) + a4 + _rand(rng, 200)], [_rand(rng, 700), a4 + a4]]
    b = _batch(tmp_path, asms)
    try:
        for c in (1, 2, 3, 4, 5):
            got = _check(b, queries, asms, k, c, literal=True)
            if k == 21:   # (random 21-mers do not repeat by chance: the multiplicities are the planted ones)
                kept = min(c, 4)
                assert got["n_seeds"].tolist() == [5 * kept, 5 * sum(m <= c for m in (2, 3, 4, 4)), 5 * sum(m <= c for m in (3, 4))]
                ss = got["_seed_stats"]
                assert ss["seed_words"] == 5 * kept and ss["dropped_words"] == 5 * (4 - kept) and ss["longest_owner_list"] == kept
                assert ss["dropped_windows"] == 5 * sum(m for m in (1, 2, 3, 4) if m > c) and ss["seed_windows"] == 5 * sum(m for m in (1, 2, 3, 4) if m <= c)
                assert got["seeds"][0, 0] > 0 and (c < 4 or got["seeds"][2, 1] > 0)
        for c in (0, 257):
            with pytest.raises(ValueError, match="1..256"):
                b.best_hits(queries, k, seed_copies=c)
    finally:
        b.close()


# ---- 4: orientation ---------------------------------------------------------------------------------------------------------------

def test_a_query_and_its_reverse_complement(tmp_path):
    rng = random.Random(41)
    k = 21
    q, q2 = _rand(rng, 250), _rand(rng, 120)
    mut = bytearray(q)
    mut[100] = ord("ACGT"[("ACGT".index(chr(mut[100])) + 1) % 4])
    asms = [[_rand(rng, 500) + q + _rand(rng, 300)], [_rand(rng, 100), H.revcomp(bytes(mut)) + _rand(rng, 400)], [_rand(rng, 900)],
            [q2 + _rand(rng, 20)]]
    queries = [q, H.revcomp(q), q2, H.revcomp(q2)]
    b = _batch(tmp_path, asms)
    try:
        got = _check(b, queries, asms, k, 2)
        for x, y in ((0, 1), (2, 3)):
            for f in ("seeds", "record", "dist", "end"):
                assert np.array_equal(got[f][x], got[f][y]), f
            hit = got["seeds"][x] > 0
            assert np.array_equal(got["strand"][x][hit] ^ 1, got["strand"][y][hit]) and not got["strand"][[x, y]][:, ~hit].any()
        assert got["seeds"][0].tolist() == [250 - k + 1, 250 - k + 1 - k, 0, 0] and got["dist"][0].tolist() == [0, 1, NONE, NONE]
        assert got["strand"][0].tolist() == [0, 1, 0, 0] and got["strand"][1].tolist() == [1, 0, 0, 0]
        assert not _fields(b.best_hits(queries, k))["n_seeds"].any()
    finally:
        b.close()


def test_an_inverted_repeat_and_a_palindrome(tmp_path):
    """X + spacer + revcomp(X) in one query: a word of X has two owners in that query, one window canonical and one not.  ACGT at
    k = 4, twice in the query text: its own reverse complement, no seed at any cap."""
    rng = random.Random(42)
    x = _rand(rng, 60)
    q = x + _rand(rng, 40) + H.revcomp(x)
    asms = [[_rand(rng, 200) + q + _rand(rng, 100)], [_rand(rng, 300) + x + _rand(rng, 300)], [H.revcomp(x) + _rand(rng, 100)]]
    b = _batch(tmp_path, asms)
    try:
        got = _check(b, [q], asms, 21, 2, literal=True)
        assert got["_seed_stats"]["longest_owner_list"] == 2 and got["n_seeds"].tolist() == [160 - 20]
        # in the whole copy every window of X and of its mirror image hits both owners: 2 * 40 hits on either strand's diagonal
        assert got["seeds"][0, 0] >= 2 * 40 and got["dist"][0, 0] == 0
        assert _fields(b.best_hits([q], 21))["n_seeds"].tolist() == [160 - 20 - 2 * 40]
    finally:
        b.close()
    queries = [b"TTACGTCC", b"GGACGTAAA"]
    asms = [[b"CCCCACGTCCCCC"], [b"AAAATTACGTCCAAAA", b"TTTGGACGTAAACC"]]
    b = _batch(tmp_path, asms, "p")
    try:
        got = _check(b, queries, asms, 4, 2, literal=True)
        assert got["_seed_stats"]["palindromic_words"] == 1 and got["n_seeds"].tolist() == [5 - 1, 6 - 1]   # every window but ACGT
    finally:
        b.close()


# ---- 5: repeats inside a query ------------------------------------------------------------------------------------------------------

def test_repeats_inside_a_query(tmp_path):
    """k = 15, queries of 200 bases.  A unit of 30 three times in a row: the owners of a word lie 30 and 60 apart, in the same band
    or the next.  The same unit twice, 170 apart: the owners' bands differ by two or three, their votes do not add up."""
    rng = random.Random(51)
    k, u = 15, _rand(rng, 30)
    near = _rand(rng, 20) + u + u + u + _rand(rng, 90)
    far = u + _rand(rng, 140) + u
    assert len(near) == len(far) == 200
    asms = [[_rand(rng, 300) + near + _rand(rng, 200)], [_rand(rng, 150) + far + _rand(rng, 100)], [_rand(rng, 500) + u + _rand(rng, 400)],
            [_rand(rng, 64 * 7 + 50) + u + u + _rand(rng, 300), H.revcomp(far)]]
    b = _batch(tmp_path, asms)
    try:
        for c in (1, 2, 3, 5, 6):
            got = _check(b, [near, far], asms, k, c, literal=(c == 5))
            ss = got["_seed_stats"]
            # the unit's 16 inner words have 5 windows in the text of both queries: dropped below c = 5, the longest lists from there on
            assert ss["longest_owner_list"] == (5 if c >= 5 else c) and (ss["dropped_windows"] >= 80) == (c < 5)
        assert got["dist"][0, 0] == 0 and got["dist"][1, 1] == 0 and got["strand"][1, 3] == 1 and got["dist"][1, 3] == 0
    finally:
        b.close()


# ---- 6: lane, wave and record bounds ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 5, 32])
def test_lane_wave_and_record_bounds(tmp_path, k):
    """c = 3, every query three times.  Record 0: a run of a tile and a lane's share more; one query is the 16 + k - 1 bases that
    make the 16 windows of lane 5 of the first tile, so that lane appends 48 keys and its neighbours none; another the 16 windows of
    the second tile's only lane.  Record 1: runs shorter than a tile between Ns, a query in one of them.  The last k-mer of record 1
    and the first of record 2 (another assembly's first) are queries too."""
    rng = random.Random(600 + k)
    long_run = _rand(rng, TILE + 16 + k - 1)
    shorts = [_rand(rng, n) for n in (k - 1, k, k + 15, 300, k + 16)]
    rec1 = b"N".join(shorts)
    rec2 = _rand(rng, 400)
    asms = [[_rand(rng, 37) + b"N" + long_run, rec1], [rec2, long_run[16 * 5 + 1:]]]
    base = [long_run[16 * 5:16 * 5 + 16 + k - 1], long_run[TILE:], shorts[3][100:130 + k], rec1[-k:], rec2[:k], shorts[1]]
    queries = base * 3
    b = _batch(tmp_path, asms)
    try:
        got = _check(b, queries, asms, k, 3, literal=(k != 5))
        n = len(base)
        for f in MATRIX + ("n_seeds",):
            assert np.array_equal(got[f][:n], got[f][n:2 * n]) and np.array_equal(got[f][:n], got[f][2 * n:]), f
        if k >= 15:
            assert got["n_seeds"][:n].tolist() == [16, 16, 31, 1, 1, 1] and got["_seed_stats"]["longest_owner_list"] == 3
            assert got["seeds"][:n, 0].tolist() == [16, 16, 31, 1, 0, 1] and got["seeds"][:n, 1].tolist() == [15, 16, 0, 0, 1, 0]
            assert got["end"][0, 0] == 38 + 16 * 5 + 16 + k - 1 and got["end"][1, 0] == 38 + len(long_run) and got["end"][3, 0] == len(rec1)
            assert got["record"][3, 0] == 1 and got["record"][4, 1] == 2 and got["end"][4, 1] == k and not got["dist"][:n, 0][got["seeds"][:n, 0] > 0].any()
            assert _fields(b.best_hits(queries, k, seed_copies=2))["_stats"]["hits"] == 0      # three windows a word: dropped whole
    finally:
        b.close()


# ---- 7: the largest cap -------------------------------------------------------------------------------------------------------------

def test_the_largest_cap(tmp_path, monkeypatch):
    rng = random.Random(7)
    k, q = 21, _rand(rng, 40)
    asms = [[_rand(rng, 200) + q + _rand(rng, 100)]]
    b = _batch(tmp_path, asms)
    try:
        one = _fields(b.best_hits([q], k))
        assert one["seeds"].tolist() == [[20]] and one["dist"].tolist() == [[0]]
        monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", "1")     # 64 keys: the one assembly's 5120 hits double the buffer
        got = _fields(b.best_hits([q] * 256, k, seed_copies=256))
        st, ss = got["_stats"], got["_seed_stats"]
        assert st["hits"] == 256 * 20 and st["chunks"] == 1 and st["buffer_doublings"] >= 1 and st["buffer_keys"] >= st["hits"], st
        assert ss["longest_owner_list"] == 256 and ss["seed_words"] == 20 and ss["seed_windows"] == 256 * 20 and ss["dropped_words"] == 0
        for f in MATRIX + ("n_seeds",):
            assert got[f].dtype == one[f].dtype and np.array_equal(got[f], np.repeat(one[f], 256, axis=0)), f
        assert not _fields(b.best_hits([q] * 256, k, seed_copies=255))["n_seeds"].any()
    finally:
        b.close()


# ---- 8: the hooks -------------------------------------------------------------------------------------------------------------------

def _hooked(b, queries, ref):
    got = _fields(b.best_hits(queries, 21, seed_copies=2))
    _same(ref, got, "hooked")
    return got["_stats"]


def test_the_hooks_on_the_shared_route(four, monkeypatch):
    b, queries, asms = four
    queries = queries + queries
    ref = _check(b, queries, asms, 21, 2)
    st = ref["_stats"]
    assert st["chunks"] == 1 and st["chunk_splits"] == 0 and st["buffer_doublings"] == 0 and st["launches"] == 1
    per = sum(st["chunk_hits"]) // 4                        # about the hits of one assembly (8 bytes a key, twice for the sort)
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(max(1, (per * 16 * 5 // 4) // 1024)))   # holds one assembly, not two
    st2 = _hooked(b, queries, ref)
    assert st2["chunks"] == 4 and st2["chunk_splits"] >= 2 and st2["hits"] == st["hits"] and st2["buffer_doublings"] == 0, st2
    monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(max(1, (per * 16 * 5 // 2) // 1024)))   # holds two, not four
    st3 = _hooked(b, queries, ref)
    assert st3["chunks"] == 2 and st3["chunk_splits"] == 1, st3
    monkeypatch.delenv("SEQWIN_AMD_HIT_BUFFER_KB")
    monkeypatch.setenv("SEQWIN_AMD_HIT_MAX_BLOCKS", "1")
    assert _hooked(b, queries, ref)["launches"] > 4
    monkeypatch.delenv("SEQWIN_AMD_HIT_MAX_BLOCKS")
    monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(st["distinct_kmers"].bit_length()))
    _hooked(b, queries, ref)


# ---- 9: degenerate inputs -----------------------------------------------------------------------------------------------------------

def test_degenerate_inputs(tmp_path):
    rng = random.Random(3)
    asms = [[_rand(rng, 3000)], [_rand(rng, 1500), _rand(rng, 20)]]
    b = _batch(tmp_path, asms)
    try:
        h = b.best_hits([], 21, seed_copies=3)
        assert h.seeds().shape == (0, 2) and h.dist().shape == (0, 2) and h.n_seeds().shape == (0,) and h.sizes() == (0, 2, 0, 21)
        assert h.stats()["chunks"] == 0 and h.seed_stats() == dict(seed_copies=3, seed_words=0, seed_windows=0, dropped_words=0, dropped_windows=0,
                                                                   palindromic_words=0, longest_owner_list=0, hits=0)
        h.close()
        for queries in ([b"N" * 100] * 2, [b"ACGTACGT", b"ACGTACGT"], [b"", b"NNNN", b"ACGT" * 5, b"ACGT" * 5], [_rand(rng, 100)] * 2):
            got = _check(b, queries, asms, 21, 2)
            assert not got["seeds"].any() and got["_stats"]["hits"] == 0 and np.all(got["dist"] == NONE)
        got = _fields(b.best_hits([_rand(rng, 100)] * 2, 21, loci=True, min_seeds=1, seed_copies=2), MODES[2])
        assert not got["n_loci"].any() and len(got["loci_query"]) == 0
        with pytest.raises(ValueError, match="min_seeds"):
            b.best_hits([b"ACGT"], 21, loci=True, min_seeds=0, seed_copies=2)
    finally:
        b.close()
