"""CPU: the host restatement of the MinHash specification (tests/tools/minhash_host.py, the yardstick of tests/test_gpu_minhash.py)
against pinned facts a wrong restatement cannot pass, the pair rule against counts worked out by hand, and the library's argument
checks, which happen before a device is touched."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import minhash_host as H  # noqa: E402
from minhash_cases import HAND_CASES  # noqa: E402


def test_smhasher_verification_value():
    assert H.smhasher_verification() == 0x6384BA69


def test_pinned_kmer_hashes():
    assert H.hash_kmer(b"ACGTACGTACGTACGTACGTA") == 0xb4e9c495b633d387      # k = 21, canonical as written
    assert H.hash_kmer(b"ACGTACGTACGTACGT") == 0xac055887                  # k = 16: the 32-bit form
    assert H.hash_kmer(b"ACG") == 0xc784a159
    assert H.hash_bits(16) == 32 and H.hash_bits(17) == 64
    # the 32-bit form is the low half of h1
    h1, _ = H.murmur3_x64_128(np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).reshape(1, 16), 42)
    assert int(h1[0]) & 0xFFFFFFFF == 0xac055887 and int(h1[0]) >> 32 != 0


def test_canonical_choice():
    # TTTTC: its reverse complement GAAAA is smaller
    assert bytes(H.canonical_kmers(b"TTTTC", 5)[0]) == b"GAAAA"
    assert H.hash_kmer(b"TTTTC") == H.hash_kmer(b"GAAAA")
    # a palindrome is its own reverse complement
    assert bytes(H.canonical_kmers(b"ACGT", 4)[0]) == b"ACGT" and bytes(H.canonical_kmers(b"GAATTC", 6)[0]) == b"GAATTC"
    # lower case counts as upper case; a window with another letter is skipped; a k-mer never spans records
    assert np.array_equal(H.kmer_hashes(b"acgTTgca", 4), H.kmer_hashes(b"ACGTTGCA", 4))
    assert len(H.kmer_hashes(b"ACGNACGTA", 4)) == 2 and len(H.kmer_hashes(b"ACG", 4)) == 0
    assert [bytes(x) for x in H.canonical_kmers(b"ACGRACGTA", 4)] == [b"ACGT", b"CGTA"]
    assert len(H.sketch([b"ACGT", b"ACGT"], 5, 10)) == 0
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            H.sketch([b"ACGT"], k, 10)


def test_sketch_is_the_s_smallest_distinct_hashes():
    rng = random.Random(2)
    recs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (500, 30, 21, 20)]
    allh = sorted({int(x) for r in recs for x in H.kmer_hashes(r, 21)})
    assert [int(x) for x in H.sketch(recs, 21, 50)] == allh[:50]
    assert [int(x) for x in H.sketch(recs, 21, 10**6)] == allh
    assert len(H.sketch([b"A" * 1000], 21, 50)) == 1


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_pair_rule_on_hand_made_lists(case):
    _, a, b, s, shared, total = case
    assert H.pair_walk(a, b, s) == (shared, total)
    assert H.pair_walk(b, a, s) == (shared, total)        # symmetric
    assert H.pair_fast(a, b, s) == (shared, total)


def test_the_closed_form_equals_the_walk():
    """pair_fast (what the big blocks of the GPU tests are compared with) against the literal walk on random lists whose lengths
    stay at or below S, as a sketch's do."""
    rng = random.Random(1)
    for _ in range(3000):
        s = rng.choice([1, 2, 5, 10, 50])
        a = sorted(rng.sample(range(60), rng.randint(0, min(s, 40))))
        b = sorted(rng.sample(range(60), rng.randint(0, min(s, 40))))
        assert H.pair_walk(a, b, s) == H.pair_fast(a, b, s), (a, b, s)


def test_jaccard_of_two_empty_sketches_raises():
    with pytest.raises(ZeroDivisionError):
        H.jaccard(np.array([[0]]), np.array([[0]]))
    assert H.jaccard(np.array([[1]]), np.array([[3]]))[0, 0] == 1 / 3


def test_minhash_entries_are_in_the_abi_table():
    from seqwin_amd._abi import PROTOTYPES
    for name in ("sw_batch_minhash", "sw_minhash_from_sketches", "sw_minhash_sizes", "sw_minhash_export", "sw_minhash_counts",
                 "sw_minhash_frac_rowsums", "sw_minhash_stats", "sw_minhash_free"):
        assert name in PROTOTYPES, name


def test_the_minhash_hooks_are_test_only():
    rel, tst = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    assert rel.exists() and tst.exists()
    blob_rel, blob_tst = rel.read_bytes(), tst.read_bytes()
    for h in (b"SEQWIN_AMD_MH_CAND_CAP\0", b"SEQWIN_AMD_MH_MAX_BLOCKS\0"):
        assert h not in blob_rel and h in blob_tst, h


def test_arguments_are_checked_before_a_device_is_touched():
    from seqwin_amd._lib import c_vp, lib
    from seqwin_amd.device import MinHash
    h = c_vp()
    for k in (0, 33, 1 << 40):
        assert lib.sw_batch_minhash(None, k, 1000, 42, None, ctypes.byref(h)) == 2 and b"1..32" in lib.sw_last_error()
    assert lib.sw_batch_minhash(None, 21, 0, 42, None, ctypes.byref(h)) == 2 and b"sketch size" in lib.sw_last_error()
    assert lib.sw_batch_minhash(None, 21, 1000, 1 << 32, None, ctypes.byref(h)) == 2 and b"seed" in lib.sw_last_error()
    assert lib.sw_batch_minhash(None, 21, 1000, 42, None, ctypes.byref(h)) == 2 and b"NULL" in lib.sw_last_error()
    out = (ctypes.c_uint32 * 4)()
    dbl = (ctypes.c_double * 4)()
    assert lib.sw_minhash_counts(None, 0, 1, 0, 1, out, out) == 2 and b"NULL" in lib.sw_last_error()
    assert lib.sw_minhash_frac_rowsums(None, 0, 1, 0, 1, dbl) == 2
    assert lib.sw_minhash_sizes(None, None, None, None, None) == 2 and lib.sw_minhash_export(None, None, None) == 2
    assert lib.sw_minhash_stats(None, None, None) == 2
    lib.sw_minhash_free(None)
    with pytest.raises(ValueError, match="strictly ascending"):
        MinHash.from_sketches([0, 3], [1, 3, 3], 10)
    with pytest.raises(ValueError, match="strictly ascending"):
        MinHash.from_sketches([0, 2, 4], [1, 2, 9, 4], 10)
    with pytest.raises(ValueError, match="more than s"):
        MinHash.from_sketches([0, 3], [1, 2, 3], 2)
    with pytest.raises(ValueError, match="above 2\\^32 - 1"):
        MinHash.from_sketches([0, 2], [1, 1 << 32], 10, hash_bits=32)
    with pytest.raises(ValueError, match="hash_bits"):
        MinHash.from_sketches([0, 1], [1], 10, hash_bits=16)
    with pytest.raises(ValueError, match="sketch size"):
        MinHash.from_sketches([0, 0], [], 0)
    with pytest.raises(ValueError, match="non-decreasing"):
        MinHash.from_sketches(np.array([0, 2, 1, 3], np.uint64), [1, 2, 3], 10)
    with pytest.raises(ValueError, match="offsets"):
        MinHash.from_sketches([0, 2], [1, 2, 3], 10)
