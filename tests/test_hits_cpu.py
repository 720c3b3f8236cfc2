"""CPU: the two host restatements of the best-hit specification (tests/tools/hits_host.py) against each other
on random inputs and against hand-made cases with the answers written out; markers.hit_summary on a hand-made matrix; and the
argument checks of the C entry points that need no device.  The device side (seqwin_amd/csrc/hits.hip) is compared with the same
restatement in tests/test_gpu_infix_direct.py and tests/test_gpu_best_hits.py."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import hits_host as H  # noqa: E402

KS = [1, 2, 4, 15, 16, 17, 21, 31, 32]


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("seed", range(6))
def test_infix_forms_agree_on_random_pairs(seed):
    rng = random.Random(seed)
    records = [_rand(rng, rng.randrange(0, 200), b"ACGTN" if seed % 2 else b"ACGT") for _ in range(4)] + [b"acgun" * 9]
    queries = [_rand(rng, rng.randrange(0, 90), b"ACGTX" if seed % 3 == 0 else b"AC") for _ in range(5)] + [records[0][10:70], H.revcomp(records[1][5:50])]
    pairs = []
    for _ in range(40):
        r = rng.randrange(len(records))
        a = rng.randrange(0, len(records[r]) + 1)
        pairs.append((rng.randrange(len(queries)), rng.randrange(2), r, a, rng.randrange(a, len(records[r]) + 1)))
    d, e = H.infix(queries, records, pairs)
    d2, e2 = H.infix_literal(queries, records, pairs)
    assert d.dtype == np.uint32 and e.dtype == np.uint32 and np.array_equal(d, d2) and np.array_equal(e, e2)


INFIX_HAND = [
    # queries, records, (query, strand, record, start, stop), dist, end
    (["ACGT"], ["TTACGTTT"], (0, 0, 0, 0, 8), 0, 6),                # an exact copy ends behind position 5
    (["ACGT"], ["TTACGTTT"], (0, 1, 0, 0, 8), 0, 6),                # ACGT is its own reverse complement
    (["AACC"], ["TTGGTTAA"], (0, 1, 0, 0, 8), 0, 6),                # GGTT is the reverse complement
    (["ACGT"], ["TTACGTTT"], (0, 0, 0, 3, 8), 1, 6),                # the text starts at C: A is inserted
    (["ACGT"], ["ACGTACGT"], (0, 0, 0, 0, 8), 0, 4),                # two exact copies: the smallest end
    (["ACGT"], ["ACNT"], (0, 0, 0, 0, 4), 1, 4),                    # an N equals nothing
    (["ANGT"], ["ANGT"], (0, 0, 0, 0, 4), 1, 4),                    # ... not even another N
    ([""], ["ACGT"], (0, 0, 0, 2, 4), 0, 2),                        # an empty query
    (["ACG"], ["ACGT"], (0, 0, 0, 3, 3), 3, 3),                     # an empty text
    (["acgu"], ["TTACGTTT"], (0, 0, 0, 0, 8), 0, 6),                # lower case, U reads as T
    (["AAAA"], ["CCCC"], (0, 0, 0, 0, 4), 4, 0),                    # nothing matches: the first column attains m already
]


@pytest.mark.parametrize("case", INFIX_HAND, ids=[str(i) for i in range(len(INFIX_HAND))])
def test_infix_hand_made_cases(case):
    queries, records, pair, dist, end = case
    for fn in (H.infix, H.infix_literal):
        d, e = fn(queries, records, [pair])
        assert (int(d[0]), int(e[0])) == (dist, end), fn.__name__


@pytest.mark.parametrize("k", KS)
def test_best_hits_forms_agree_on_random_text(k):
    rng = random.Random(k)
    anc = _rand(rng, 900)
    r0 = bytearray(anc[:500])
    r0[200:201] = b"N"
    r0[300:320] = bytes(r0[300:320]).lower()
    asms = [[bytes(r0), anc[500:]], [_rand(rng, 300)], [H.revcomp(anc[100:700]), _rand(rng, 50)], [], [anc[400:600].replace(b"T", b"U")]]
    queries = [anc[50:50 + 3 * k + 40], H.revcomp(anc[550:700]), _rand(rng, 80), anc[480:520 + k], b"N" * 40, anc[10:10 + k], anc[10:10 + k - 1],
               anc[150:260], anc[560:640] + b"AC" + anc[640:700], ""]
    a, b = H.best_hits(queries, asms, k), H.best_hits_literal(queries, asms, k)
    for f in ("n_seeds",) + H.FIELDS:
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), f
    assert a["seeds"].shape == (len(queries), len(asms)) and not a["seeds"][:, 3].any() and np.all(a["dist"][:, 3] == H.NONE)
    if k >= 15:   # (query 8 shares its k-mers with query 1: only the windows across its insertion stay seeds)
        assert a["dist"][0, 0] == 0 and a["dist"][1, 0] == 0 and a["strand"][1, 0] == 1 and a["record"][1, 0] == 1 and a["n_seeds"][8] <= k + 1


def test_best_hits_hand_made_cases():
    # k = 3, one query AACCG (m = 5): windows AAC, ACC, CCG, all unique and none its own reverse complement -> 3 seeds.
    # Record TTAACCGTT holds the copy at 2: p - i = 2 for all three, e = 2 + (5 - 3) = 4, band 0, score 3.
    # s0 = -2, lo = 0, hi = min(9, -2 + 192 + 5) = 9: dist 0, the copy ends behind position 6.
    # Record CGGTT is the reverse complement: windows CGG (= CCG, i = 2), GGT (= ACC, i = 1), GTT (= AAC, i = 0) at p = 0, 1, 2;
    # o = 1, i' = m - k - i = 0, 1, 2, e = p - i' + 2 = 2: score 3, strand 1, dist 0, end 5.
    for fn in (H.best_hits, H.best_hits_literal):
        out = fn(["AACCG"], [["TTAACCGTT"], ["GG", "CGGTT"], ["TTTT"]], 3)
        assert out["n_seeds"].tolist() == [3]
        assert out["seeds"].tolist() == [[3, 3, 0]] and out["record"].tolist() == [[0, 2, H.NONE]] and out["strand"].tolist() == [[0, 1, 0]]
        assert out["dist"].tolist() == [[0, 0, H.NONE]] and out["end"].tolist() == [[7, 5, H.NONE]]
        # AAC twice in the query text (two queries): no seed any more; ACGT at k = 4 is its own reverse complement: no seed
        out = fn(["AACCG", "GAAC"], [["TTAACCGTT"]], 3)
        assert out["n_seeds"].tolist() == [2, 1] and out["seeds"].tolist() == [[2], [0]]   # (GAA is not in the record)
        out = fn(["ACGT"], [["ACGT"]], 4)
        assert out["n_seeds"].tolist() == [0] and out["seeds"].tolist() == [[0]] and out["dist"].tolist() == [[H.NONE]]
        # equal scores in two records: the smaller record wins; on two strands of one record: strand 0
        out = fn(["AACCG"], [["AACCG", "AACCG"]], 3)
        assert out["record"].tolist() == [[0]]
        out = fn(["AACCG"], [["CGGTT" + "T" * 70 + "AACCG"]], 3)
        assert out["strand"].tolist() == [[0]] and out["end"].tolist() == [[80]]


def test_k_outside_1_to_32_is_refused():
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            H.best_hits(["ACGT"], [["ACGT"]], k)
        with pytest.raises(ValueError):
            H.best_hits_literal(["ACGT"], [["ACGT"]], k)


def test_the_c_abi_refuses_bad_arguments_without_a_device():
    from seqwin_amd._core import _ptr
    from seqwin_amd._lib import c_u64, c_vp, check, lib
    from seqwin_amd.device import INFIX_PAIR_DTYPE, _infix_pairs
    offs = np.array([0, 4], np.uint64)
    h = c_vp()
    for k in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            check(lib.sw_batch_best_hits(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(k), ctypes.byref(h)))
    assert INFIX_PAIR_DTYPE.itemsize == 20
    d, e = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    for pair in ((1, 0, 0, 0, 4), (0, 2, 0, 0, 4), (0, 0, 0, 5, 4)):      # no such query, no such strand, start > stop
        pr = _infix_pairs([pair])
        with pytest.raises(ValueError, match="names no query"):
            check(lib.sw_batch_infix_distances(None, _ptr(offs), b"ACGT", c_u64(1), _ptr(pr), c_u64(1), _ptr(d), _ptr(e), None, None))
    with pytest.raises(ValueError):
        _infix_pairs([(0, 0, 0, -1, 4)])


def test_hit_summary_on_a_hand_made_matrix():
    from seqwin_amd.markers import HIT_SUMMARY_DTYPE, hit_summary
    no = 0xFFFFFFFF
    dist = np.array([[0, 10, no, 5, 200],
                     [1, 1, 1, 1, 1],          # a query of length 0
                     [2, 3, 4, no, no]], np.uint32)
    s = hit_summary(dist, [100, 0, 20], n_tar=3, min_identity=0.75)
    assert s.dtype == HIT_SUMMARY_DTYPE
    # row 0: targets 1.0, 0.9 and no hit -> 0; non-targets 0.05 and min(1, 2.0)
    assert s["similarity_tar"][0] == (1.0 + (1.0 - 10 / 100) + 0.0) / 3 and s["f_tar"][0] == 2 / 3
    assert s["distance_neg"][0] == (5 / 100 + 1.0) / 2 and s["f_neg"][0] == 1 / 2
    for f in HIT_SUMMARY_DTYPE.names:
        assert np.isnan(s[f][1]), f
    # row 2: 0.25 * 20 = 5: 2, 3 and 4 all count; no hit reads distance 1 and never counts
    assert s["f_tar"][2] == 1.0 and s["distance_neg"][2] == 1.0 and s["f_neg"][2] == 0.0
    assert s["similarity_tar"][2] == ((1 - 2 / 20) + (1 - 3 / 20) + (1 - 4 / 20)) / 3
    all_tar = hit_summary(dist, [100, 0, 20], 5)
    assert np.isnan(all_tar["distance_neg"]).all() and np.isnan(all_tar["f_neg"]).all()
    with pytest.raises(ValueError):
        hit_summary(dist, [100, 0, 20], 6)
    with pytest.raises(ValueError):
        hit_summary(dist, [100, 0], 2)
