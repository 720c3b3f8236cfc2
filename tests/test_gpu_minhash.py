"""GPU: MinHash sketches and pair counts of csrc/minhash.hip against the host restatement of the specification
(tests/tools/minhash_host.py), exactly: sketch arrays, `shared`, `total`.  The hash pass gives a lane 16 consecutive k-mers and a
wave 1024 (one tile); record lengths straddle both."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import minhash_host as H  # noqa: E402
from minhash_cases import HAND_CASES  # noqa: E402

pytestmark = pytest.mark.gpu

LANE, TILE = 16, 1024


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n):
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def _write(tmp_path, name, records):
    p = tmp_path / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d some text\n" % (name.encode(), i))
            r = bytes(r)
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def _csr(sketches):
    offs = np.zeros(len(sketches) + 1, np.uint64)
    np.cumsum([len(s) for s in sketches], out=offs[1:])
    hs = np.concatenate([np.asarray(s, np.uint64) for s in sketches]) if sketches else np.zeros(0, np.uint64)
    return offs, hs.astype(np.uint64)


def _check_batch(paths, assemblies, k, s, want_general=None):
    """Sketches and all pair counts of FASTA files against the restatement; returns the stats."""
    from seqwin_amd.device import Batch
    b = Batch.from_fasta(paths, n_cpu=2)
    mh = b.minhash(k, s)
    try:
        want = [H.sketch(recs, k, s) for recs in assemblies]
        w_offs, w_hs = _csr(want)
        offs, hs = mh.sketches()
        assert offs.dtype == np.uint64 and hs.dtype == np.uint64
        assert np.array_equal(offs, w_offs)
        assert np.array_equal(hs, w_hs)
        assert mh.sizes() == (len(paths), len(w_hs), s, H.hash_bits(k))
        n = len(paths)
        sh, to = mh.counts()
        w_sh, w_to = H.counts_block(w_offs, w_hs, s, range(n), range(n))
        assert np.array_equal(sh, w_sh) and np.array_equal(to, w_to)
        st = mh.stats()
        if want_general is not None:
            assert (st["general_route"] > 0) == want_general, st
        return st
    finally:
        mh.close()
        b.close()


def _hash_shape_assemblies(k, seed):
    rng = random.Random(seed)
    a0 = []
    r = _rand(rng, 3000)
    at = 100
    for run in (1, k - 1, k):                       # N runs of length 1, k - 1 and k
        if run:
            r[at:at + run] = b"N" * run
        at += 2 * k + 40
    r[0:1] = b"N"
    r[-1:] = b"n"                                   # an N run at the record's first and last base
    r[900:1000] = bytes(r[900:1000]).lower()        # a lower-case stretch
    for j, c in zip((1200, 1201, 1300, 1400, 1500), b"RYKMS"):
        r[j] = c                                    # IUPAC letters
    a0.append(r)
    a0.append(_rand(rng, k - 1))                    # shorter than k
    a0.append(_rand(rng, k))                        # exactly k
    for nk in (LANE - 1, LANE, LANE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + LANE + 1):
        a0.append(_rand(rng, nk + k - 1))           # k-mer counts around a lane's and a wave's share
    a1 = [b"N" * 50, _rand(rng, k - 1), b"NNNN" + bytes(_rand(rng, k - 1)) + b"RR" + bytes(_rand(rng, k - 1))]   # no valid k-mer
    a2 = [_rand(rng, 5000), bytes(_rand(rng, 700)).lower()]
    return [a0, a1, a2]


@pytest.mark.parametrize("k", [1, 3, 8, 9, 15, 16, 17, 21, 24, 25, 31, 32])
def test_hash_shapes(tmp_path, k):
    asms = _hash_shape_assemblies(k, 100 + k)
    paths = [_write(tmp_path, f"a{i}.fa", recs) for i, recs in enumerate(asms)]
    assert len(H.sketch(asms[1], k, 64)) == 0
    _check_batch(paths, asms, k, 64)


def _selection_assemblies():
    rng = random.Random(77)
    unit = bytes(_rand(rng, 7))
    return [
        [_rand(rng, 20_000), _rand(rng, 3000)],
        [_rand(rng, 300)],                          # fewer than S distinct k-mers for the larger S
        [b"A" * 30_000],                            # one distinct hash, 29 980 copies
        [unit * 3000],                              # a tandem repeat: 7 distinct k-mers
        [_rand(rng, 90_000)],                       # much larger than its neighbours
        [_rand(rng, 40)],                           # much smaller
    ]


@pytest.fixture(scope="module")
def selection_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mh_sel")
    asms = _selection_assemblies()
    return [_write(d, f"s{i}.fa", recs) for i, recs in enumerate(asms)], asms


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 1000])
def test_selection(selection_files, s):
    paths, asms = selection_files
    st = _check_batch(paths, asms, 21, s, want_general=True)
    # the poly-A and the tandem repeat fall short under any threshold (1 and 7 distinct hashes in ~3000 copies or more each: no
    # candidate, fewer than S distinct ones, or more copies than the range holds); the random assemblies must not
    assert st["general_route"] == 2, st
    assert st["capacity"] >= 2 * s + 256 and st["largest_candidates"] >= 1


@pytest.mark.parametrize("s", [1, 2, 63, 64, 65, 1000])
def test_selection_through_the_general_route(selection_files, s, monkeypatch):
    paths, asms = selection_files
    monkeypatch.setenv("SEQWIN_AMD_MH_CAND_CAP", "8")
    st = _check_batch(paths, asms, 21, s, want_general=True)
    assert st["capacity"] == 8 and st["general_route"] >= 5, st


def test_a_sketch_size_above_the_lds_sort_sends_every_assembly_through_the_general_route(tmp_path):
    """From a capacity above 16384 candidates on (S = 8000: 2 S + 256 and its margin) there is no pre-selection and no LDS sort."""
    rng = random.Random(8)
    asms = [[_rand(rng, 12_000), _rand(rng, 3000)], [_rand(rng, 5000)], [b"N" * 40], [_rand(rng, 30)]]
    paths = [_write(tmp_path, f"b{i}.fa", recs) for i, recs in enumerate(asms)]
    st = _check_batch(paths, asms, 21, 8000, want_general=True)
    assert st["general_route"] == 3 and st["capacity"] == 16384 and st["candidates"] == 0 and st["largest_candidates"] == 0, st
    assert st["hash_ms"] >= 0 and st["select_ms"] > 0


def test_a_hash_pass_of_several_launches(tmp_path, monkeypatch):
    """A launch holds fewer than 2^32 threads and the hash pass gives every tile a wave, so a large set (15 000 genomes: 73 M tiles)
    is hashed by several launches.  Tiles that a launch drops would leave their assemblies without candidates, to be finished --
    with the right sketch -- by the general route: the route taken is what shows it.  SEQWIN_AMD_MH_MAX_BLOCKS lowers the launch
    size: at 1 workgroup (4 tiles) per launch the 112 tiles here take 28 launches, at 3 (12 tiles) the last launch is a partial one."""
    rng = random.Random(21)
    asms = [[_rand(rng, 30_000), _rand(rng, 5000)], [_rand(rng, 41_000)], [_rand(rng, 36_000)]]
    paths = [_write(tmp_path, f"l{i}.fa", recs) for i, recs in enumerate(asms)]
    for blocks in ("1", "3"):
        monkeypatch.setenv("SEQWIN_AMD_MH_MAX_BLOCKS", blocks)
        st = _check_batch(paths, asms, 21, 1000, want_general=False)
        assert st["general_route"] == 0 and st["largest_candidates"] > 1000, st
    monkeypatch.setenv("SEQWIN_AMD_MH_CAND_CAP", "8")          # and the general route's own hash launches
    st = _check_batch(paths, asms, 21, 1000, want_general=True)
    assert st["general_route"] == 3


def test_plain_random_assemblies_do_not_take_the_general_route(tmp_path):
    rng = random.Random(5)
    asms = [[_rand(rng, n)] for n in (30_000, 8000, 100_000, 12_000)]
    paths = [_write(tmp_path, f"p{i}.fa", recs) for i, recs in enumerate(asms)]
    for s in (64, 1000):
        st = _check_batch(paths, asms, 21, s, want_general=False)
        assert 0 < st["candidates"] <= 4 * st["capacity"]
    st = _check_batch(paths, asms, 12, 1000, want_general=False)   # the 32-bit sketch
    assert st["general_route"] == 0


# ---- pairs --------------------------------------------------------------------------------------------------------------------

S_PAIRS = 130


def _crafted_sketches(bits):
    """140 lists of lengths 0, 1, 63, 64, 65, S - 1, S (and others) drawn from one pool, so that they overlap; the 64-bit pool
    holds values that differ only in their top or only in their bottom half."""
    rng = random.Random(bits)
    if bits == 64:
        pool = sorted({(hi << 32) | lo for hi in (0, 1, 2, 0x7FFFFFFF, 0xFFFFFFFF) for lo in rng.sample(range(1 << 32), 60)} |
                      {0, (1 << 64) - 1})
    else:
        pool = sorted(set(rng.sample(range(1 << 32), 300)) | {0, (1 << 32) - 1})
    lens = [0, 1, 63, 64, 65, S_PAIRS - 1, S_PAIRS, 2, 17, 100]
    lists = [sorted(rng.sample(pool, lens[i % len(lens)])) for i in range(138)]
    lists.append(list(lists[6]))          # an identical pair
    lists.append([])
    return lists


@pytest.fixture(scope="module", params=[64, 32])
def crafted(request):
    from seqwin_amd.device import MinHash
    lists = _crafted_sketches(request.param)
    offs, hs = _csr(lists)
    n = len(lists)
    want = H.counts_block(offs, hs, S_PAIRS, range(n), range(n))
    mh = MinHash.from_sketches(offs, hs, S_PAIRS, hash_bits=request.param)
    yield mh, want, n
    mh.close()


@pytest.mark.parametrize("rows,cols", [((5, 6), (7, 8)), ((2, 5), (3, 133)), ((10, 75), (70, 135)), ((0, 140), (0, 140)),
                                       ((139, 140), (139, 140)), ((61, 67), (63, 129)), ((3, 3), (0, 5))])
def test_pair_blocks(crafted, rows, cols):
    mh, (w_sh, w_to), n = crafted
    sh, to = mh.counts(rows, cols)
    assert sh.dtype == np.uint32 and sh.shape == (rows[1] - rows[0], cols[1] - cols[0])
    assert np.array_equal(sh, w_sh[rows[0]:rows[1], cols[0]:cols[1]])
    assert np.array_equal(to, w_to[rows[0]:rows[1], cols[0]:cols[1]])
    sh_t, to_t = mh.counts(cols, rows)
    assert np.array_equal(sh, sh_t.T) and np.array_equal(to, to_t.T)


def test_a_pair_block_of_several_launches(crafted, monkeypatch):
    """The pair kernel's rows are split over launches the same way: one row per launch here."""
    mh, (w_sh, w_to), n = crafted
    monkeypatch.setenv("SEQWIN_AMD_MH_MAX_BLOCKS", "2")
    sh, to = mh.counts((3, 76), (1, 140))
    assert np.array_equal(sh, w_sh[3:76, 1:140]) and np.array_equal(to, w_to[3:76, 1:140])


def test_crafted_sketches_come_back_and_ranges_are_checked(crafted):
    mh, _, n = crafted
    offs, hs = mh.sketches()
    lists = _crafted_sketches(mh.sizes()[3])
    w_offs, w_hs = _csr(lists)
    assert np.array_equal(offs, w_offs) and np.array_equal(hs, w_hs)
    for rows, cols in (((0, n + 1), (0, 1)), ((0, 1), (0, n + 1)), ((3, 2), (0, 1))):
        with pytest.raises(ValueError, match="outside"):
            mh.counts(rows, cols)
    assert mh.stats()["general_route"] == 0


_HAND = [(c, bits) for c in HAND_CASES for bits in (64, 32) if bits == 64 or max(c[1] + c[2] + [0]) < (1 << 32)]


@pytest.mark.parametrize("case,bits", _HAND, ids=[f"{c[0]}-{bits}" for c, bits in _HAND])
def test_hand_made_pairs(case, bits):
    from seqwin_amd.device import MinHash
    name, a, b, s, shared, total = case
    offs, hs = _csr([a, b])
    mh = MinHash.from_sketches(offs, hs, s, hash_bits=bits)
    try:
        sh, to = mh.counts()
        assert (int(sh[0, 1]), int(to[0, 1])) == (shared, total) and (int(sh[1, 0]), int(to[1, 0])) == (shared, total)
        assert (int(sh[0, 0]), int(to[0, 0])) == (len(a), len(a)) and (int(sh[1, 1]), int(to[1, 1])) == (len(b), len(b))
    finally:
        mh.close()


def test_a_long_row_is_searched_outside_lds():
    """Sketches above 48 KiB take the pair kernel's form that searches the row in global memory."""
    from seqwin_amd.device import MinHash
    rng = np.random.default_rng(3)
    pool = np.unique(rng.integers(0, 1 << 63, 12_000, dtype=np.uint64))
    lists = [np.sort(rng.choice(pool, n, replace=False)) for n in (7000, 6500, 0, 1, 7000)]
    offs, hs = _csr(lists)
    mh = MinHash.from_sketches(offs, hs, 7000)
    try:
        sh, to = mh.counts()
        w_sh, w_to = H.counts_block(offs, hs, 7000, range(5), range(5))
        assert np.array_equal(sh, w_sh) and np.array_equal(to, w_to)
    finally:
        mh.close()


# ---- real batches and the reduction ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def synthetic():
    from seqwin_amd.device import Batch
    b = Batch.synthetic(7, 2, 5000, n_ancestors=2, snp_ppm=20_000, seed=3)
    offs = b.record_offsets()
    asms = [[b.record(r) for r in range(int(offs[a]), int(offs[a + 1]))] for a in range(7)]
    mh = b.minhash(21, 200)
    yield b, mh, asms
    mh.close()
    b.close()


def test_synthetic_batch(synthetic):
    b, mh, asms = synthetic
    want = [H.sketch(recs, 21, 200) for recs in asms]
    w_offs, w_hs = _csr(want)
    offs, hs = mh.sketches()
    assert np.array_equal(offs, w_offs) and np.array_equal(hs, w_hs)
    sh, to = mh.counts()
    w_sh, w_to = H.counts_block(w_offs, w_hs, 200, range(7), range(7))
    assert np.array_equal(sh, w_sh) and np.array_equal(to, w_to)
    j = mh.jaccard()
    assert j.dtype == np.float64 and np.array_equal(j, H.jaccard(w_sh, w_to))
    assert np.array_equal(j, j.T) and np.all(np.diag(j) == 1.0)
    assert np.any((j > 0) & (j < 1)), "the SNP rate must put some pair strictly between 0 and 1"
    assert np.array_equal(mh.counts((0, 3), None)[0], mh.counts(None, (0, 3))[0].T)


def test_reduction(synthetic):
    _, mh, _ = synthetic
    n = 7
    a, b2 = mh.frac_rowsums(), mh.frac_rowsums()
    assert a.tobytes() == b2.tobytes()                      # the same bits
    j = mh.jaccard()
    for rows, cols in (((0, n), (0, n)), ((0, 3), (0, 3)), ((3, n), (0, 3)), ((2, 3), (1, 6))):
        blk = j[rows[0]:rows[1], cols[0]:cols[1]]
        want = float(np.mean(2 * blk / (1 + blk)))
        got = mh.expected_frac(rows, cols)
        # both sides add the same N non-negative f64 terms in different orders
        assert abs(got - want) <= blk.size * 2.0 ** -53 * want, (rows, cols, got, want)
    n_tar = 3
    e_abs, e_pres = mh.penalty_fracs(n_tar)
    w_abs = 1 - H.expected_frac(j[:n_tar, :n_tar])
    w_pres = H.expected_frac(j[n_tar:, :n_tar])
    # (1 - x rounds once more on either side: half an ulp of a value below 1, 2^-54, each)
    assert abs(e_abs - w_abs) <= n_tar * n_tar * 2.0 ** -53 * (1 - w_abs) + 2.0 ** -53
    assert abs(e_pres - w_pres) <= (n - n_tar) * n_tar * 2.0 ** -53 * w_pres
    for bad in (0, n):
        with pytest.raises(ValueError):
            mh.penalty_fracs(bad)


def test_a_pair_of_empty_sketches_raises_zero_division():
    from seqwin_amd.device import MinHash
    offs, hs = _csr([[1, 2], [], []])
    mh = MinHash.from_sketches(offs, hs, 5)
    try:
        sh, to = mh.counts()
        assert (int(sh[1, 2]), int(to[1, 2])) == (0, 0) and (int(sh[0, 1]), int(to[0, 1])) == (0, 2)
        with pytest.raises(ZeroDivisionError):
            mh.jaccard()
        with pytest.raises(ZeroDivisionError):
            mh.expected_frac()
        with pytest.raises(ZeroDivisionError):
            mh.frac_rowsums((1, 2), (1, 3))
        assert mh.jaccard((0, 1), (0, 3)).tolist() == [[1.0, 0.0, 0.0]]
        assert mh.expected_frac((0, 1), (0, 3)) == pytest.approx(1 / 3, rel=1e-15)
    finally:
        mh.close()


# ---- a real-shaped case that needs no hook (tests/test_release_library_minhash.py runs these two on the release library) --------

def test_real_shaped_case(tmp_path):
    rng = random.Random(11)
    anc = _rand(rng, 40_000)
    asms = []
    for g in range(4):
        seq = bytearray(anc)
        for _ in range(400 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([seq[:25_000], seq[25_000:], _rand(rng, 2000)])
    paths = [_write(tmp_path, f"g{i}.fa", recs) for i, recs in enumerate(asms)]
    st = _check_batch(paths, asms, 21, 1000, want_general=False)
    assert st["capacity"] == 4096


def test_jaccard_matrix_on_paths(tmp_path):
    from seqwin_amd.mash import jaccard_matrix
    rng = random.Random(12)
    anc = _rand(rng, 30_000)
    asms = []
    for g in range(3):
        seq = bytearray(anc)
        for _ in range(600 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([seq])
    paths = [_write(tmp_path, f"j{i}.fa", recs) for i, recs in enumerate(asms)]
    j = jaccard_matrix(paths, 21, 1000, n_cpu=2)
    offs, hs = _csr([H.sketch(recs, 21, 1000) for recs in asms])
    want = H.jaccard(*H.counts_block(offs, hs, 1000, range(3), range(3)))
    assert j.shape == (3, 3) and j.dtype == np.float64 and np.array_equal(j, want)
    assert 0 < j[0, 2] < j[0, 1] < 1
