"""CPU: the two host restatements of the shared-seed rule (tests/tools/shared_seeds_host.py) against each
other on random inputs and on hand-made cases with the answers written out; both against tests/tools/hits_host.py at c = 1; the
bounds of c, in the restatements, in Batch.best_hits and at the C entry point (checked before a device is touched).  The device
side is compared with the same restatement in tests/test_gpu_best_hits_shared.py."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import hits_host as H  # noqa: E402
import shared_seeds_host as S  # noqa: E402

ALL = ("n_seeds",) + H.FIELDS


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _same(a, b):
    for f in ALL:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), (f, a[f].tolist(), b[f].tolist())


def _case(k, seed):
    """Queries that share words with each other, with themselves and with their reverse complements, over assemblies with an N,
    lower case, U, an empty assembly and a reverse-complemented one."""
    rng = random.Random(1000 * k + seed)
    anc = _rand(rng, 900)
    r0 = bytearray(anc[:500])
    r0[200:201] = b"N"
    r0[300:320] = bytes(r0[300:320]).lower()
    unit = anc[600:630]
    asms = [[bytes(r0), anc[500:]], [_rand(rng, 300)], [H.revcomp(anc[100:700]), _rand(rng, 50)], [], [anc[400:600].replace(b"T", b"U")],
            [_rand(rng, 40) + unit + _rand(rng, 10) + unit + _rand(rng, 150) + unit]]
    queries = [anc[50:50 + 3 * k + 40], anc[50:50 + 3 * k + 40], H.revcomp(anc[60:60 + 2 * k + 30]), anc[480:520 + k], b"N" * 40,
               unit + _rand(rng, 5) + unit + _rand(rng, 100) + unit, anc[560:640] + b"AC" + anc[600:700], anc[10:10 + k - 1], "", anc[100:160].lower()]
    return queries, asms


@pytest.mark.parametrize("k", [1, 2, 4, 15, 21, 32])
@pytest.mark.parametrize("c", [1, 2, 3, 256])
def test_the_two_forms_agree_on_random_text(k, c):
    queries, asms = _case(k, c)
    a, b = S.best_hits_shared(queries, asms, k, c), S.best_hits_shared_literal(queries, asms, k, c)
    _same(a, b)
    assert int(a["n_seeds"].sum()) == S.seed_stats(queries, k, c)["seed_windows"]
    if k >= 15 and c >= 2:   # the sequence given twice: both rows are what one copy alone finds at the same cap
        assert a["n_seeds"][0] == a["n_seeds"][1] > 0 and all(np.array_equal(a[f][0], a[f][1]) for f in H.FIELDS) and a["dist"][0, 0] == 0


@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 17, 21, 31, 32])
def test_c_1_is_the_unique_rule(k):
    """tests/test_hits_cpu.py::test_best_hits_forms_agree_on_random_text's inputs and this file's: both forms at c = 1 equal
    hits_host.best_hits."""
    rng = random.Random(k)
    anc = _rand(rng, 900)
    r0 = bytearray(anc[:500])
    r0[200:201] = b"N"
    asms = [[bytes(r0), anc[500:]], [_rand(rng, 300)], [H.revcomp(anc[100:700]), _rand(rng, 50)], [], [anc[400:600].replace(b"T", b"U")]]
    queries = [anc[50:50 + 3 * k + 40], H.revcomp(anc[550:700]), _rand(rng, 80), anc[480:520 + k], b"N" * 40, anc[10:10 + k], anc[10:10 + k - 1],
               anc[150:260], anc[560:640] + b"AC" + anc[640:700], ""]
    for qs, ams in ((queries, asms), _case(k, 0)):
        want = H.best_hits(qs, ams, k)
        _same(S.best_hits_shared(qs, ams, k, 1), want)
        _same(S.best_hits_shared_literal(qs, ams, k, 1), want)


def test_hand_made_cases():
    for fn in (S.best_hits_shared, S.best_hits_shared_literal):
        # k = 3.  AACCG twice: the words AAC, ACC, CCG have two windows each.  c = 1: no seed; c = 2: three owners per query, and
        # either row is hits_host's hand-made case of one AACCG (record TTAACCGTT: score 3, dist 0, end 7; CGGTT: strand 1, end 5)
        out = fn(["AACCG", "AACCG"], [["TTAACCGTT"], ["GG", "CGGTT"], ["TTTT"]], 3, 1)
        assert out["n_seeds"].tolist() == [0, 0] and not out["seeds"].any() and np.all(out["dist"] == H.NONE)
        out = fn(["AACCG", "AACCG"], [["TTAACCGTT"], ["GG", "CGGTT"], ["TTTT"]], 3, 2)
        assert out["n_seeds"].tolist() == [3, 3]
        assert out["seeds"].tolist() == [[3, 3, 0]] * 2 and out["record"].tolist() == [[0, 2, H.NONE]] * 2 and out["strand"].tolist() == [[0, 1, 0]] * 2
        assert out["dist"].tolist() == [[0, 0, H.NONE]] * 2 and out["end"].tolist() == [[7, 5, H.NONE]] * 2
        # a query and its reverse complement: CGGTT's windows CGG, GGT, GTT are CCG, ACC, AAC in the other orientation.  Against
        # TTAACCGTT query 0 is found on strand 0 and query 1 on strand 1, at the same place
        out = fn(["AACCG", "CGGTT"], [["TTAACCGTT"]], 3, 2)
        assert out["n_seeds"].tolist() == [3, 3] and out["seeds"].tolist() == [[3], [3]] and out["strand"].tolist() == [[0], [1]]
        assert out["dist"].tolist() == [[0], [0]] and out["end"].tolist() == [[7], [7]]
        # a repeat inside a query: AAC at 0 and 5 of AACCGAAC (m = 8; AAC, ACC, CCG, CGA, GAA, AAC).  c = 1: four seeds; c = 2: six
        # owners.  Record AACCGAAC: the batch windows AAC at 0 and 5 hit both owners each: e = p - i + 5 = 5, 0, 10, 5; the other
        # four windows e = 5.  Band 0 holds all eight hits
        out = fn(["AACCGAAC"], [["AACCGAAC"]], 3, 1)
        assert out["n_seeds"].tolist() == [4] and out["seeds"].tolist() == [[4]]
        out = fn(["AACCGAAC"], [["AACCGAAC"]], 3, 2)
        assert out["n_seeds"].tolist() == [6] and out["seeds"].tolist() == [[8]] and out["dist"].tolist() == [[0]] and out["end"].tolist() == [[8]]
        # the cap drops a word whole: AAC has three windows in AACAACAAC + ... at c = 2 it is no seed, at c = 3 it is
        q = "AACGAACTAAC"                                    # AAC at 0, 4, 8; ACG, CGA, GAA, ACT, CTA, TAA once
        assert fn([q], [[q]], 3, 2)["n_seeds"].tolist() == [6] and fn([q], [[q]], 3, 3)["n_seeds"].tolist() == [9]
        # ACGT at k = 4 is its own reverse complement: no seed at any cap, however many windows have it
        out = fn(["ACGT", "ACGT"], [["ACGT"]], 4, 2)
        assert out["n_seeds"].tolist() == [0, 0] and out["seeds"].tolist() == [[0], [0]]
    st = S.seed_stats(["AACGAACTAAC", "ACGT"], 3, 2)         # ACG now twice (kept), CGT = ACG's reverse complement: three windows
    assert st == dict(seed_copies=2, seed_words=5, seed_windows=5, dropped_words=2, dropped_windows=6, palindromic_words=0, longest_owner_list=1)
    assert S.seed_stats(["ACGT", "ACGT", "AAAA"], 4, 2) == dict(seed_copies=2, seed_words=1, seed_windows=1, dropped_words=0, dropped_windows=0,
                                                                 palindromic_words=1, longest_owner_list=1)


def test_the_bounds_of_c():
    for c in (0, 257, -1):
        with pytest.raises(ValueError, match="1..256"):
            S.best_hits_shared(["ACGT"], [["ACGT"]], 3, c)
        with pytest.raises(ValueError, match="1..256"):
            S.best_hits_shared_literal(["ACGT"], [["ACGT"]], 3, c)
    for c in (1, 256):
        S.best_hits_shared(["ACGT"], [["ACGT"]], 3, c)


def test_the_c_abi_refuses_a_bad_cap_without_a_device():
    from seqwin_amd._abi import PROTOTYPES
    from seqwin_amd._core import _ptr
    from seqwin_amd._lib import c_u64, c_vp, check, lib
    assert "sw_batch_best_hits_shared" in PROTOTYPES and "sw_hits_seed_stats" in PROTOTYPES
    offs = np.array([0, 4], np.uint64)
    h = c_vp()
    for c in (0, 257):
        with pytest.raises(ValueError, match="1..256"):
            check(lib.sw_batch_best_hits_shared(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(3), c_u64(c), c_u64(0), c_u64(0), ctypes.byref(h)))
    with pytest.raises(ValueError, match="1..32"):
        check(lib.sw_batch_best_hits_shared(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(33), c_u64(2), c_u64(0), c_u64(0), ctypes.byref(h)))
    with pytest.raises(ValueError, match="0..2"):
        check(lib.sw_batch_best_hits_shared(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(3), c_u64(2), c_u64(3), c_u64(1), ctypes.byref(h)))
    with pytest.raises(ValueError, match="min_seeds"):
        check(lib.sw_batch_best_hits_shared(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(3), c_u64(2), c_u64(2), c_u64(0), ctypes.byref(h)))
    with pytest.raises(ValueError, match="NULL"):
        check(lib.sw_hits_seed_stats(None, None))
