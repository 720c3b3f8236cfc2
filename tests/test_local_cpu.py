"""CPU: the two host restatements of the local alignment with affine gap scores (tests/tools/local_host.py)
against each other, against hand-made cases with the nine figures written out, and against the canonical infix alignment re-scored
under the same system.  No device is touched."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import hits_host as H  # noqa: E402
import local_host as L  # noqa: E402

BLASTN = (2, -3, 5, 2)


def both(pattern: str, text: str, scoring=BLASTN):
    """The nine figures of both forms, which must agree; '#' is an invalid base."""
    lit = L.local_literal_one(pattern, text, scoring)
    vec = L.local_one(H._codes(pattern.encode()), H._codes(text.encode()), scoring)
    assert tuple(int(v) for v in vec) == tuple(int(v) for v in lit), (pattern, text, scoring, vec, lit)
    out = {f: np.array([v], np.uint32) for f, v in zip(L.FIELDS, lit)}
    L.check(out, scoring, [pattern.encode()], [text.encode()], [(0, 0, 0, 0, len(text))])
    return tuple(int(v) for v in lit)


@pytest.mark.parametrize("scoring", L.SCORINGS)
@pytest.mark.parametrize("alphabet", ["AC", "ACGT"])
def test_the_two_forms_agree_on_random_pairs(scoring, alphabet):
    """Two letters and go = 0 make the ties: of extension against opening, of the diagonal against E and F, of equal maxima."""
    rng = random.Random(1000 * len(alphabet) + 7 * scoring[0] + 3 * scoring[2] - scoring[1])
    positive = gapped = 0
    for _ in range(40):
        m, n = rng.randrange(1, 28), rng.randrange(1, 40)
        pat = "".join(rng.choice(alphabet) for _ in range(m))
        text = "".join(rng.choice(alphabet) for _ in range(n))
        if rng.random() < 0.5 and m > 6:                                # a diverged copy of the pattern inside the text
            cp = list(pat)
            for _ in range(rng.randrange(0, 4)):
                at = rng.randrange(len(cp))
                cp[at:at + 1] = rng.choice(["", rng.choice(alphabet), rng.choice(alphabet) * 2, "#"])
            text = text[:n // 2] + "".join(cp) + text[n // 2:]
        got = both(pat, text, scoring)
        positive += got[0] > 0
        gapped += got[8] > 0
    assert positive >= 30
    if scoring[2] == 0:
        assert gapped > 0


A12, B12 = "ACGTTGCAAGCT", "GGATCCTTAGCA"


def test_an_exact_copy_scores_r_m_and_spans_the_query():
    p = "ACGTACGTAC"
    for sc in L.SCORINGS:
        assert both(p, "TT" + p + "GG", sc) == (sc[0] * 10, 0, 10, 2, 12, 10, 0, 0, 0)


def test_half_a_copy_at_a_record_end():
    p = "ACGTTGCAAC" + "GGATCCTTAG"
    assert both(p, "TTTTTT" + p[:10]) == (20, 0, 10, 6, 16, 10, 0, 0, 0)
    assert both(p, p[10:] + "AAAAAA") == (20, 10, 20, 0, 10, 10, 0, 0, 0)


@pytest.mark.parametrize("scoring", L.SCORINGS)
def test_one_mismatch_is_kept_where_two_matches_pay_for_it(scoring):
    """Eight matches, a mismatch, two matches: the tail is worth 2 r + p.  Kept where that is positive; where it is 0 the shorter
    alignment ends in the smaller column and wins; where it is negative the tail is cut."""
    r, p, _, _ = scoring
    got = both("ACGTTGCA" + "T" + "GG", "CC" + "ACGTTGCA" + "A" + "GG" + "CC", scoring)
    if 2 * r > -p:
        assert got == (10 * r + p, 0, 11, 2, 13, 10, 1, 0, 0)
    else:
        assert got == (8 * r, 0, 8, 2, 10, 8, 0, 0, 0)
    assert {s: 2 * s[0] > -s[1] for s in L.SCORINGS} == {(2, -3, 5, 2): True, (1, -2, 0, 1): False, (1, -1, 1, 1): True, (1, -3, 5, 2): False,
                                                         (5, -4, 10, 6): True}


def test_a_gap_of_one_and_a_gap_of_three():
    assert both(A12 + B12, "CC" + A12 + "T" + B12 + "CC") == (48 - 5 - 2, 0, 24, 2, 27, 24, 0, 1, 1)        # a text base faces a gap
    assert both(A12 + "TTT" + B12, "CC" + A12 + B12 + "CC") == (48 - 5 - 6, 0, 27, 2, 26, 24, 0, 1, 3)      # three pattern bases do
    assert both(A12 + B12, "CC" + A12 + "TTT" + B12 + "CC") == (48 - 5 - 6, 0, 24, 2, 29, 24, 0, 1, 3)


def test_extension_wins_a_tie_against_opening():
    """go = 0: behind the gap's first column E equals H, so extending and opening cost the same; the record must say one gap."""
    got = both("ACGTACGT" + "GGCCAATT", "ACGTACGT" + "TT" + "GGCCAATT", (1, -2, 0, 1))
    assert got == (16 - 2, 0, 16, 0, 18, 16, 0, 1, 2)
    got = both("ACGTACGT" + "TT" + "GGCCAATT", "ACGTACGT" + "GGCCAATT", (1, -2, 0, 1))
    assert got == (16 - 2, 0, 18, 0, 16, 16, 0, 1, 2)


def test_the_diagonal_wins_a_tie_against_e_and_f():
    """(1, -2, 0, 1): a mismatch costs what a gap in the text and a gap in the pattern cost together.
    ACGT.G.ACGT against ACGT.C.ACGT: behind H[4][4] = 4 the cell (5, 5) has diagonal 4 - 2, E = H[5][4] - 1 = 3 - 1 and F = H[4][5] - 1
    = 3 - 1: all 2, the diagonal's record (one mismatch, no gap) is carried into the four matches behind it.
    ACGT.G.ACGT against ACGT.CC.ACGT: H[5][5] = 2 as before (text ACGTC), with E[5][5] = 2 carrying two gaps.  In cell (5, 6) the
    diagonal is H[4][5] - 2 = 3 - 2 = 1 with the record of E[4][5] plus a mismatch, (0, 0, 1, 1, 1); E = max(E[5][5], H[5][5]) - 1 = 1
    by extension, (0, 0, 0, 2, 3); F = H[4][6] - 1 = 2 - 1 = 1, (0, 0, 0, 2, 3).  All tie, the diagonal's record is carried; four
    matches follow: score 5, 9 rows, 10 columns, ins = (1 + 9 - 10) / 2 = 0, nident = 9 - 1.  E or F first would read (5, 0, 9, 0,
    10, 8, 0, 2, 3)."""
    assert both("ACGT" + "G" + "ACGT", "ACGT" + "C" + "ACGT", (1, -2, 0, 1)) == (6, 0, 9, 0, 9, 8, 1, 0, 0)
    assert both("ACGT" + "G" + "ACGT", "ACGT" + "CC" + "ACGT", (1, -2, 0, 1)) == (5, 0, 9, 0, 10, 8, 1, 1, 1)


def test_e_wins_a_tie_against_f():
    """(1, -2, 0, 1), P = ACATTT, T = GCACTTT.  Two alignments of score 2 end next to cell (3, 4): CA = CA in H[3][3] with the record
    (1, 1, 0, 0, 0), and AC = AC in H[2][4] with (0, 2, 0, 0, 0).  In (3, 4) the bases A and C differ: the diagonal is H[2][3] - 2 =
    -2, E = max(E[3][3], H[3][3]) - 1 = 2 - 1 opens from the first, (1, 1, 0, 1, 1), F = max(F[2][4], H[2][4]) - 1 = 2 - 1 opens from the
    second, (0, 2, 0, 1, 1).  E is first in the order, so H[3][4] = 1 carries (1, 1, 0, 1, 1), and TTT = TTT behind it ends in the only
    cell of score 4, (6, 7): qstart 1, sstart 1, 5 rows, 6 columns, ins = (1 + 5 - 6) / 2 = 0, nident 5 -- CA-TTT under CACTTT.  F
    first would read (4, 0, 6, 2, 7, 5, 0, 1, 1), ACATTT over AC-TTT.  With pattern and text exchanged the two openings change
    roles: E opens from H[4][2] = 2, (2, 0, 0, 0, 0), F from H[3][3] = 2, (1, 1, 0, 0, 0); E wins again, the end cell is (7, 6): 5 rows,
    6 columns, ins 0 -- ACTTT under ACATTT."""
    assert both("ACATTT", "GCACTTT", (1, -2, 0, 1)) == (4, 1, 6, 1, 7, 5, 0, 1, 1)
    assert both("GCACTTT", "ACATTT", (1, -2, 0, 1)) == (4, 2, 7, 0, 6, 5, 0, 1, 1)


def test_equal_maxima_the_smallest_column_then_the_smallest_row():
    assert both("ACGT", "ACGT" + "TT" + "ACGT") == (8, 0, 4, 0, 4, 4, 0, 0, 0)          # two columns
    assert both("GCA" + "T" + "GCA", "GCA") == (6, 0, 3, 0, 3, 3, 0, 0, 0)              # two rows of one column
    assert both("GCA" + "T" + "GCA", "CCGCA") == (6, 0, 3, 2, 5, 3, 0, 0, 0)


def test_an_invalid_base_equals_nothing_on_either_side():
    assert both("ACGTTGCA" + "#" + "GGATCCTT", "ACGTTGCA" + "A" + "GGATCCTT") == (32 - 3, 0, 17, 0, 17, 16, 1, 0, 0)
    assert both("ACGTTGCA" + "A" + "GGATCCTT", "ACGTTGCA" + "#" + "GGATCCTT") == (32 - 3, 0, 17, 0, 17, 16, 1, 0, 0)
    assert both("ACGTTGCA" + "#" + "GGATCCTT", "ACGTTGCA" + "#" + "GGATCCTT") == (32 - 3, 0, 17, 0, 17, 16, 1, 0, 0)
    assert both("####", "####") == (0,) * 9


def test_empty_sides_and_no_match_at_all():
    assert both("", "ACGT") == (0,) * 9
    assert both("ACGT", "") == (0,) * 9
    assert both("", "") == (0,) * 9
    assert both("AAAA", "CCGGTT") == (0,) * 9
    out = L.alignments([b"AAAA", b""], [b"CCGGCGCC"], [(0, 0, 0, 3, 8), (1, 1, 0, 2, 2), (0, 1, 0, 5, 8)])
    assert out["score"].tolist() == [0, 0, 0] and out["sstart"].tolist() == [3, 2, 5] and out["send"].tolist() == [3, 2, 5]
    assert out["qend"].tolist() == [0, 0, 0]


def test_pairs_strands_and_windows():
    queries = [b"ACGTTGCAAGCT", b"ggatccuuagca", b"ACGTXGCAAGCT"]
    records = [b"TTTT" + b"ACGTTGCAAGCT" + b"CCCC" + H.revcomp(b"GGATCCTTAGCA") + b"AA", b"NNNNACGTTGCAAGCTNN"]
    pairs = [(0, 0, 0, 0, 34), (0, 0, 0, 6, 34), (1, 1, 0, 0, 34), (1, 0, 0, 0, 34), (2, 0, 1, 0, 18), (0, 1, 1, 2, 18)]
    vec, lit = L.alignments(queries, records, pairs), L.alignments_literal(queries, records, pairs)
    for f in L.FIELDS:
        assert np.array_equal(vec[f], lit[f]), f
        assert vec[f].dtype == np.uint32
    L.check(vec, BLASTN, queries, records, pairs)
    assert vec["score"][:3].tolist() == [24, 20, 24] and vec["qstart"][:3].tolist() == [0, 2, 0]
    assert vec["sstart"][:3].tolist() == [4, 6, 20] and vec["send"][:3].tolist() == [16, 16, 32]
    assert vec["score"][4] == 2 * 11 - 3 and vec["mismatch"][4] == 1 and vec["sstart"][4] == 4


@pytest.mark.parametrize("scoring", L.SCORINGS)
def test_local_is_at_least_the_infix_alignment_rescored(scoring):
    rng = random.Random(11)
    seen = 0
    for _ in range(30):
        m = rng.randrange(5, 40)
        pat = "".join(rng.choice("ACGT") for _ in range(m))
        cp = list(pat)
        for _ in range(rng.randrange(0, 3)):
            at = rng.randrange(len(cp))
            cp[at:at + 1] = rng.choice(["", rng.choice("ACGT"), rng.choice("ACGT") * 2])
        text = "".join(rng.choice("ACGT") for _ in range(9)) + "".join(cp) + "".join(rng.choice("ACGT") for _ in range(7))
        pc, tc = H._codes(pat.encode()), H._codes(text.encode())
        _, _, _, nident, _, _, ops = A.align_one(pc, tc)
        global_score = L.rescore(nident, ops, scoring)
        local_score = L.local_one(pc, tc, scoring)[0]
        if global_score > 0:
            seen += 1
            assert local_score >= global_score, (pat, text, scoring)
    assert seen >= 10


def test_the_bounds_of_the_scoring_system_and_of_two_to_the_16():
    for bad in ((0, -3, 5, 2), (256, -3, 5, 2), (2, 0, 5, 2), (2, -256, 5, 2), (2, 3, 5, 2), (2, -3, -1, 2), (2, -3, 256, 2), (2, -3, 5, 0),
                (2, -3, 5, 256)):
        with pytest.raises(ValueError):
            L.local_one(H._codes(b"ACGT"), H._codes(b"ACGT"), bad)
        with pytest.raises(ValueError):
            L.local_literal_one("ACGT", "ACGT", bad)
    for ok in ((1, -1, 0, 1), (255, -255, 255, 255)):
        assert both("ACGT", "ACGT", ok)[0] == 4 * ok[0]
    big, small = np.zeros(1 << 16, np.uint8), np.zeros(4, np.uint8)
    for a, b in ((big, small), (small, big)):
        with pytest.raises(ValueError):
            L.local_one(a, b)
    with pytest.raises(ValueError):
        L.local_literal_one("A" * (1 << 16), "ACGT")
    assert L.local_one(np.zeros((1 << 16) - 1, np.uint8)[:0], small) == (0,) * 9
