"""CPU: the host restatement of csrc/seqs.hip (tests/tools/seqs_host.py) pinned on hand-computed cases and on the metric axioms it
must obey, and the new entry points present in the generated ABI table."""
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import seqs_host as H  # noqa: E402


def test_hand_computed_distances():
    r = "ACGTTGCAAGGCTA"
    assert H.distance(r, r) == (0, 0)                                   # identity
    assert H.distance(r, "ACGTTGGAAGGCTA") == (1, 0)                    # one substitution
    assert H.distance(r, "ACGTTGCATAGGCTA") == (1, 0)                   # one insertion
    assert H.distance(r, "ACGTTGAAGGCTA") == (1, 0)                     # one deletion
    assert H.revcomp(r) == b"TAGCCTTGCAACGT"
    assert H.distance(r, "TAGCCTTGCAACGT") == (0, 1)                    # pure reverse complement
    assert H.revcomp("ACGCGT") == b"ACGCGT" and H.distance("ACGCGT", "ACGCGT") == (0, 0)   # a reverse palindrome: the tie is forward
    assert H.distance("N", "N") == (1, 0)                               # an invalid base equals nothing
    assert H.distance("ACNGT", "ACNGT") == (1, 0) and H.distance("ACRGT", "ACGT") == (1, 0)
    assert H.distance("", "ACG") == (3, 0) and H.distance("ACG", "") == (3, 0) and H.distance("", "") == (0, 0)
    assert H.distance("AAAA", "CCCC") == (4, 0) and H.distance("AAAA", "TTTT") == (0, 1)
    assert H.distance("AC", "CA") == (2, 0)                             # d_fwd = d_rev = 2 (revcomp of CA is TG)
    assert H.levenshtein("GATTACA", "GCATGCT") == 4 and H.levenshtein("ACGT" * 20, "CGTA" * 20) == 2


def test_hand_computed_fetch():
    text = "acgtNNrACGTacgu"
    assert H.fetch(text, 0, 4) == ("ACGT", False)
    assert H.fetch(text, 0, 5) == ("ACGTN", True) and H.fetch(text, 3, 8) == ("TNNNA", True)
    assert H.fetch(text, 7, 11) == ("ACGT", False) and H.fetch(text, 6, 7) == ("N", True)
    assert H.fetch(text, 4, 4) == ("", False)


def test_symmetry_and_triangle_inequality():
    rng = random.Random(11)

    def rnd(n):
        return "".join(rng.choice("ACGTACGTACGTN") for _ in range(n))

    def mutate(s):
        out = []
        for ch in s:
            x = rng.random()
            if x < 0.05:
                continue
            out.append(rng.choice("ACGT") if x < 0.10 else ch)
            if x > 0.95:
                out.append(rng.choice("ACGT"))
        return "".join(out)

    for _ in range(60):
        a = rnd(rng.choice([1, 5, 40, 70, 130]))
        b = mutate(a) if rng.random() < 0.7 else rnd(rng.choice([1, 30, 90]))
        c = mutate(b) if rng.random() < 0.7 else rnd(rng.choice([2, 64]))
        if rng.random() < 0.3:
            b = H.revcomp(b).decode()
        dab, dba = H.distance(a, b), H.distance(b, a)
        assert dab[0] == dba[0]                                         # d(R, S) = d(S, R)
        assert H.levenshtein(a, b) == H.levenshtein(b, a)
        assert H.levenshtein(a, H.revcomp(b)) == H.levenshtein(H.revcomp(a), b)   # the reverse complement is an isometry
        assert H.distance(a, c)[0] <= dab[0] + H.distance(b, c)[0]       # triangle, on the strand-free distance
        assert H.levenshtein(a, c) <= H.levenshtein(a, b) + H.levenshtein(b, c)
        assert abs(len(a) - len(b)) <= H.levenshtein(a, b) <= max(len(a), len(b))


def test_the_new_entry_points_are_in_the_abi_table():
    from seqwin_amd._abi import PROTOTYPES
    for name in ("sw_batch_fetch", "sw_markers_fetch", "sw_seqs_sizes", "sw_seqs_export", "sw_seqs_stats", "sw_seqs_free",
                 "sw_batch_edit_distances", "sw_markers_row_distances"):
        assert name in PROTOTYPES, name
