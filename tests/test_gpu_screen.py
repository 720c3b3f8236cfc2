"""GPU: the exact k-mer containment screen of csrc/screen.hip (Batch.screen, Markers.screen) against the host restatement of its
specification (tests/tools/screen_host.py) on the same text: every count and every n_kmers, exactly and whole.  The probe pass gives
a lane 16 consecutive k-mers and a wave 1024 (one tile); a bitmap word holds 32 k-mer numbers; run lengths and query sizes straddle
all three."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import screen_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
KS = [1, 2, 3, 15, 16, 17, 21, 31, 32]
TILE = 1024


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


def _check(batch, queries, assemblies, k, want=None):
    """Screen `queries` and compare everything with the restatement; returns (counts, n_kmers, stats)."""
    w_counts, w_nk = want if want is not None else H.screen(queries, assemblies, k)
    s = batch.screen(queries, k)
    try:
        counts, nk = s.counts(), s.n_kmers()
        assert counts.dtype == np.uint32 and nk.dtype == np.uint32
        assert counts.shape == (len(queries), len(assemblies))
        assert np.array_equal(nk, w_nk)
        assert np.array_equal(counts, w_counts)
        st = s.stats()
        assert s.sizes() == (len(queries), len(assemblies), st["distinct_kmers"], k)
        cont = s.containment()
        assert cont.dtype == np.float64 and np.array_equal(cont, H.containment(w_counts, w_nk), equal_nan=True)
        return counts, nk, st
    finally:
        s.close()


# ---- k sweep ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_k_sweep(tmp_path, k):
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
    b = _batch(tmp_path, asms)
    try:
        counts, nk, st = _check(b, queries, asms, k)
        assert nk[5] == 0 and nk[6] == 1 and nk[8] == 0
        assert st["query_positions"] == sum(len(q) for q in queries) and st["batch_kmers"] > 0 and st["chunks"] == 1
    finally:
        b.close()


# ---- run and lane bounds ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 5, 32])
def test_run_and_lane_bounds(tmp_path, k):
    """Valid runs of k - 1, k, k + 15, k + 16, 1024 + k - 2, 1024 + k - 1 and 1024 + k bases (0, 1, 16, 17, 1023, 1024 and 1025
    k-mers: a lane's share and a tile's, one below and one above), as records and as the stretches between Ns of one record; two
    records of one assembly that share k-mers; an assembly without a record of k bases; hits at the last k-mer of a run -- which
    is the first of its second tile --, at the last of its first tile and at its first."""
    rng = random.Random(1000 + k)
    lens = [k - 1, k, k + 15, k + 16, TILE + k - 2, TILE + k - 1, TILE + k]
    runs = [_rand(rng, n) for n in lens]
    shared = _rand(rng, 3 * k + 50)
    long_run = runs[-1]
    asms = [
        [r for r in runs],                                                  # one run per record
        [b"N".join(runs), b"NN" + runs[2] + b"N"],                          # the same runs between single Ns in one record
        [_rand(rng, 100) + shared + _rand(rng, 80), shared[k:] + _rand(rng, 60)],   # two records that share k-mers
        [_rand(rng, k - 1), _rand(rng, k - 1), b"N" * (k + 2)],             # nothing of k valid bases: a zero column
        [long_run[1:]],                                                     # the long run without its first k-mer, one place on
    ]
    # of the long run's 1025 k-mers: the last (the first of its second tile), the last of its first tile, the first
    queries = runs + [shared, long_run[-k:], long_run[TILE - 1:TILE - 1 + k], long_run[:k], runs[2][-k:], runs[2][:k]]
    b = _batch(tmp_path, asms)
    try:
        counts, nk, _ = _check(b, queries, asms, k)
        assert np.all(counts[:, 3] == 0) and counts[0].sum() == 0 and nk[0] == 0
        if k >= 15:   # (random k-mers of this length do not repeat: the counts are the run's k-mers)
            assert nk[:7].tolist() == [0, 1, 16, 17, TILE - 1, TILE, TILE + 1]
            assert counts[:7, 0].tolist() == nk[:7].tolist() and counts[:7, 1].tolist() == nk[:7].tolist()
            assert counts[8, 0] == 1 and counts[8, 4] == 1          # (in assembly 4 the last of the first tile)
            assert counts[9, 0] == 1 and counts[9, 4] == 1
            assert counts[10, 0] == 1 and counts[10, 4] == 0
            assert counts[7, 2] == nk[7]
    finally:
        b.close()


# ---- bitmap word bounds ----------------------------------------------------------------------------------------------------------

def _word_bound_case(k=21, seed=5):
    """Queries of 31, 32, 33, 64 and 65 distinct k-mers, one that shares k-mers of the first and of the last bitmap word of the
    65 with it and one that shares nothing; one assembly holds every query, one holds half of each, one holds none."""
    rng = random.Random(seed)
    qs = [_rand(rng, n + k - 1) for n in (31, 32, 33, 64, 65)]
    big = qs[4]
    qs.append(big[:k + 2] + b"N" + big[62:])          # numbers of the 65: its first three and its last three (another word)
    qs.append(_rand(rng, 40 + k))
    asms = [[b"N".join(qs[:6]), _rand(rng, 300)], [b"N".join(q[:len(q) // 2] for q in qs[:5])], [_rand(rng, 2000)]]
    return qs, asms, k


def test_bitmap_word_bounds(tmp_path):
    qs, asms, k = _word_bound_case()
    b = _batch(tmp_path, asms)
    try:
        counts, nk, st = _check(b, qs, asms, k)
        assert nk[:6].tolist() == [31, 32, 33, 64, 65, 6] and counts[:6, 0].tolist() == nk[:6].tolist()
        assert counts[6].sum() == 0 and counts[:, 2].sum() == 0 and 0 < counts[4, 1] < 65
        assert st["distinct_kmers"] == 31 + 32 + 33 + 64 + 65 + nk[6] and st["hits"] >= 31 + 32 + 33 + 64 + 65
        assert 0 < st["atomics"] <= st["hits"]
    finally:
        b.close()


# ---- degenerate queries ----------------------------------------------------------------------------------------------------------

def test_degenerate_queries(tmp_path):
    rng = random.Random(3)
    asms = [[_rand(rng, 3000)], [_rand(rng, 1500), _rand(rng, 20)], []]
    b = _batch(tmp_path, asms[:2])
    try:
        s = b.screen([], 21)
        assert s.counts().shape == (0, 2) and s.n_kmers().shape == (0,) and s.sizes() == (0, 2, 0, 21) and s.containment().shape == (0, 2)
        assert s.stats()["chunks"] == 0
        s.close()
        for queries in ([b"N" * 100], [b"ACGTACGT"], [b"", b"NNNN", b"ACGT" * 5]):       # Ns only, shorter than k, neither has a window
            counts, nk, st = _check(b, queries, asms[:2], 21)
            assert not counts.any() and not nk.any() and st["distinct_kmers"] == 0 and st["hits"] == 0
        queries = [_rand(rng, 300), _rand(rng, 21), _rand(rng, 60)]                       # absent from every assembly
        counts, nk, st = _check(b, queries, asms[:2], 21)
        assert not counts.any() and nk.tolist() == [280, 1, 40] and st["hits"] == 0 and st["atomics"] == 0
    finally:
        b.close()


# ---- the hooks: table nearly full, chunks, launch split ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """9 assemblies of two records each over one ancestor, and queries with a little more than 8192 distinct 21-mers."""
    rng = random.Random(9)
    anc = _rand(rng, 12_000)
    asms = []
    for g in range(9):
        seq = bytearray(anc)
        for _ in range(40 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([bytes(seq[:7000]), bytes(seq[7000:]) + _rand(rng, 200)])
    queries = [anc[i * 1000:i * 1000 + 1100] for i in range(8)] + [H.revcomp(anc[8500:9500]), _rand(rng, 500)]
    b = _batch(tmp_path_factory.mktemp("scr9"), asms, "n")
    want = H.screen(queries, asms, 21)
    yield b, queries, asms, want
    b.close()


def test_a_table_forced_nearly_full(nine, monkeypatch):
    b, queries, asms, want = nine
    _, _, st = _check(b, queries, asms, 21, want)
    d = st["distinct_kmers"]
    assert d > 8192 and st["table_capacity"] >= 2 * d
    bits = d.bit_length()                                   # 2^bits: the next power of two above d
    monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(bits))
    _, _, st = _check(b, queries, asms, 21, want)
    assert st["table_capacity"] == 1 << bits and st["longest_chain"] > 1, st
    for small in (bits - 1, 0):                             # a capacity at or below |D|
        monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(small))
        with pytest.raises(ValueError, match="distinct"):
            b.screen(queries, 21)


def test_tiny_tables_wrap_at_their_end(tmp_path, monkeypatch):
    """3 distinct k-mers in 4 slots, 6 and 7 in 8: with so few slots a probe chain runs over the table's end."""
    asms = [[b"ACGTTGCAAGGCTA"], [b"TTTTTTTTTT"], [b"CCTTGCAACGT"]]
    b = _batch(tmp_path, asms)
    try:
        for queries, k, bits, d in (([b"ACGTTGC"], 5, 2, 3), ([b"ACGTTGC", b"GGCTA"], 4, 3, 6), ([b"ACGTTGCAAGG"], 4, 3, 7)):
            assert len(H.kmer_set(queries, k)) == d
            monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(bits))
            _, _, st = _check(b, queries, asms, k)
            assert st["table_capacity"] == 1 << bits and st["distinct_kmers"] == d
    finally:
        b.close()


def test_chunks(nine, monkeypatch):
    b, queries, asms, want = nine
    words = (len(H.kmer_set(queries, 21)) + 31) // 32       # of a bitmap row
    assert words * 4 >= 1024
    kb = 12 * words // 1024                                 # a budget of at most 3 rows: 9 assemblies in 3 chunks or more
    rows = kb * 1024 // (4 * words)
    assert 1 <= rows <= 3
    monkeypatch.setenv("SEQWIN_AMD_SCR_BITMAP_KB", str(kb))
    _, _, st = _check(b, queries, asms, 21, want)
    assert st["chunks"] == -(-9 // rows) >= 3 and len(st["chunk_probe_ms"]) == st["chunks"] == len(st["chunk_reduce_ms"]), st
    monkeypatch.setenv("SEQWIN_AMD_SCR_BITMAP_KB", "0")     # below one row: a row per chunk
    _, _, st = _check(b, queries, asms, 21, want)
    assert st["chunks"] == 9, st


def test_a_launch_split(nine, monkeypatch):
    b, queries, asms, want = nine
    _, _, st1 = _check(b, queries, asms, 21, want)
    assert st1["launches"] == 1
    monkeypatch.setenv("SEQWIN_AMD_SCR_MAX_BLOCKS", "1")
    _, _, st = _check(b, queries[:3], asms, 21, (want[0][:3], want[1][:3]))
    assert st["launches"] > 1 and st["batch_kmers"] == st1["batch_kmers"], st
    monkeypatch.setenv("SEQWIN_AMD_SCR_MAX_BLOCKS", "3")    # (a last launch that is a partial one)
    _, _, st = _check(b, queries[:3], asms, 21, (want[0][:3], want[1][:3]))
    assert st["launches"] > 1


def test_blocks_of_counts(nine):
    b, queries, asms, (w_counts, w_nk) = nine
    s = b.screen(queries, 21)
    try:
        nq, na = len(queries), len(asms)
        for rows, cols in (((0, nq), (0, na)), ((2, 5), (3, 9)), ((9, 10), (0, 1)), ((4, 4), (0, 9)), ((0, 10), (8, 9)), ((3, 7), (2, 2))):
            blk = s.counts(rows, cols)
            assert blk.dtype == np.uint32 and blk.shape == (rows[1] - rows[0], cols[1] - cols[0])
            assert np.array_equal(blk, w_counts[rows[0]:rows[1], cols[0]:cols[1]])
            assert np.array_equal(s.containment(rows, cols), H.containment(w_counts, w_nk)[rows[0]:rows[1], cols[0]:cols[1]], equal_nan=True)
        assert np.array_equal(s.counts(slice(1, 4), range(2, 6)), w_counts[1:4, 2:6])
        for rows, cols in (((0, nq + 1), (0, 1)), ((0, 1), (0, na + 1)), ((3, 2), (0, 1)), ((0, 1), (5, 4))):
            with pytest.raises(ValueError, match="outside"):
                s.counts(rows, cols)
    finally:
        s.close()


def test_k_outside_1_to_32_raises(nine):
    b = nine[0]
    for k in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            b.screen([b"ACGT"], k)


# ---- a realistic shape (tests/test_release_library_screen.py runs this and the word bounds on the release library) ------------------

@pytest.fixture(scope="module")
def synthetic():
    from seqwin_amd.device import Batch
    b = Batch.synthetic(64, 2, 20_000, n_ancestors=3, snp_ppm=10_000, seed=7)
    offs = b.record_offsets()
    asms = [[b.record(r) for r in range(int(offs[a]), int(offs[a + 1]))] for a in range(64)]
    rng = random.Random(17)
    queries = []
    for i in range(40):
        rec = asms[rng.randrange(64)][rng.randrange(2)]
        at, n = rng.randrange(0, 18_000), rng.randrange(200, 1500)
        q = rec[at:at + n]
        if i % 3 == 1:
            q = H.revcomp(q)
        elif i % 3 == 2:                                    # a SNP every 50 bases
            q = bytearray(q)
            for j in range(25, len(q), 50):
                q[j] = ord("ACGT"["ACGT".index(chr(q[j])) ^ 1])
            q = bytes(q)
        queries.append(q)
    queries += [_rand(rng, rng.randrange(100, 800)) for _ in range(10)]
    yield b, queries, asms
    b.close()


@pytest.mark.parametrize("k", [21, 11])
def test_realistic_shape(synthetic, k):
    b, queries, asms = synthetic
    counts, nk, st = _check(b, queries, asms, k)
    assert st["batch_kmers"] == sum(len(H.canonical_words(r, k)) for recs in asms for r in recs) and st["chunks"] == 1 and st["launches"] == 1
    assert (counts[:40].max(axis=1) == nk[:40]).sum() >= 27       # an untouched slice is contained whole in its own assembly
    if k == 21:
        assert counts[40:].sum() == 0                             # random 21-mers are not in 2.5 Mbp
        snp = counts[2:40:3].max(axis=1) / nk[2:40:3]
        assert np.all(snp < 0.7) and np.all(snp > 0.3)            # a SNP every 50 bases takes 21 of 50 windows away


# ---- Markers.screen --------------------------------------------------------------------------------------------------------------

def test_markers_screen():
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
        o = offs.astype(np.int64)
        texts = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        assert len(texts) > 0
        for k in (g["k"], 11):
            s, direct = m.screen(b, k), b.screen(texts, k)
            try:
                assert np.array_equal(s.counts(), direct.counts()) and np.array_equal(s.n_kmers(), direct.n_kmers())
                assert s.sizes() == direct.sizes() and s.sizes()[0] == len(texts)
                ro = b.record_offsets()
                asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
                w_counts, w_nk = H.screen(texts, asms, k)
                assert np.array_equal(s.counts(), w_counts) and np.array_equal(s.n_kmers(), w_nk)
                if k == g["k"]:   # a representative is an interval of its own assembly
                    own = m.reps()[0]["assembly_idx"].astype(np.int64)
                    cont = s.containment()
                    assert np.all(cont[np.arange(len(texts)), own] == 1.0)
            finally:
                s.close()
                direct.close()
        pick = [len(texts) - 1, 0]
        s = m.screen(b, 21, select=pick)
        want = b.screen([texts[i] for i in pick], 21)
        assert np.array_equal(s.counts(), want.counts())
        s.close()
        want.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
