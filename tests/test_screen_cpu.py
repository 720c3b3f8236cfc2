"""CPU: the two host restatements of the exact k-mer containment screen (tests/tools/screen_host.py) against
each other and against hand-made cases with the expected matrix written out, and markers.screen_summary on a hand-made matrix.
The device side (seqwin_amd/csrc/screen.hip) is compared with the same restatement in tests/test_gpu_screen.py."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import screen_host as H  # noqa: E402

KS = [1, 2, 3, 15, 16, 17, 21, 31, 32]


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _both(queries, assemblies, k):
    c, n = H.screen(queries, assemblies, k)
    c2, n2 = H.screen_literal(queries, assemblies, k)
    assert c.dtype == np.uint32 and n.dtype == np.uint32 and c.shape == (len(queries), len(assemblies))
    assert np.array_equal(c, c2) and np.array_equal(n, n2)
    return c, n


@pytest.mark.parametrize("k", KS)
def test_the_vectorised_form_equals_the_literal_form_on_random_text(k):
    rng = random.Random(k)
    anc = _rand(rng, 600)
    asms = [[anc[:350], anc[350:]], [_rand(rng, 400)], [anc[100:500], _rand(rng, k - 1)], []]
    queries = [anc[50:50 + 3 * k + 7], H.revcomp(anc[200:260 + k]), _rand(rng, 80), anc[340:360 + k]]
    c, n = _both(queries, asms, k)
    assert c[0, 0] == n[0] and c[1, 0] == n[1] and np.all(c[:, 3] == 0)


@pytest.mark.parametrize("k", KS)
def test_the_vectorised_form_equals_the_literal_form_on_crafted_text(k):
    rng = random.Random(100 + k)
    base = bytearray(_rand(rng, 5 * k + 200))
    rec = bytearray(base)
    rec[40:41] = b"N"                                           # an N, a lower-case stretch, U for T, IUPAC letters
    rec[90:130] = bytes(rec[90:130]).lower()
    rec = bytes(rec).replace(b"T", b"U", 3).replace(b"t", b"u", 2)
    rec2 = bytes(base[:60]) + b"RYKM" + bytes(base[60:])
    asms = [[rec], [rec2, b"N" * 40], [bytes(base[:k - 1]), bytes(base[k:2 * k - 1])]]   # the last: every record shorter than k
    queries = [bytes(base[10:10 + k - 1]), bytes(base[10:10 + k]), bytes(base[10:10 + k + 1]),   # lengths k - 1, k, k + 1
               bytes(base[30:30 + 2 * k + 20]).lower(), bytes(base[35:45 + k]).replace(b"T", b"u"),
               b"N" * (k + 5), bytes(base[100:100 + k]) + b"N" + bytes(base[100 + k:100 + 2 * k]), b"",
               "".join(chr(c) for c in base[150:150 + k + 9])]                           # a str
    c, n = _both(queries, asms, k)
    assert n[0] == 0 and n[1] == 1 and n[5] == 0 and n[7] == 0 and np.all(c[:, 2] == 0)
    assert 1 <= n[2] <= 2 and n[6] <= 2
    cont = H.containment(c, n)
    assert cont.dtype == np.float64 and np.isnan(cont[0]).all() and np.isnan(cont[5]).all()
    assert np.array_equal(cont[1:5], c[1:5] / n[1:5, None].astype(np.float64))


HAND = [
    # name, k, queries, assemblies (lists of records), counts, n_kmers
    # AT and TA are their own reverse complements; CCAT holds CC (= GG), CA (= TG) and AT
    ("AT is its own reverse complement", 2, ["AT", "ATAT", "TA"], [["AT"], ["TA"], ["CCAT"]],
     [[1, 0, 1], [1, 1, 1], [0, 1, 0]], [1, 2, 1]),
    # ACGTACGT: ACGT, CGTA, GTAC (a palindrome too), TACG = CGTA, ACGT -> 3 distinct; TTACGTTT holds ACGT and TACG = CGTA
    ("ACGT is a palindrome at k = 4", 4, ["ACGT", "ACGTACGT"], [["ACGT"], ["TTACGTTT"], ["ACGA"]],
     [[1, 1, 0], [1, 2, 0]], [1, 3]),
    # AACCG: AAC, ACC, CCG; CGGTT is its reverse complement; GGTT holds GGT = ACC and GTT = AAC; TTTT only TTT = AAA
    ("a query and its reverse complement give identical rows", 3, ["AACCG", "CGGTT"], [["AACCG"], ["GGTT"], ["TTTT"]],
     [[3, 2, 0], [3, 2, 0]], [3, 3]),
    # AAAAAA: AAA four times; AAATTT: AAA, AAT, ATT = AAT, TTT = AAA -> 2 distinct; AATT: AAT, ATT = AAT
    ("a k-mer repeated in a query counts once", 3, ["AAAAAA", "AAATTT"], [["AAAA"], ["TTT"], ["AATT"]],
     [[1, 1, 0], [1, 1, 1]], [1, 2]),
    # ccgu = CCGT is the reverse complement of ACGG
    ("a k-mer split by a record boundary or an N gives no hit", 4, ["ACGG"], [["AC", "GG"], ["ACNGG"], ["ACGG"], ["ccgu"]],
     [[0, 0, 1, 1]], [1]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_cases(case):
    _, k, queries, asms, counts, n_kmers = case
    for fn in (H.screen, H.screen_literal):
        c, n = fn(queries, asms, k)
        assert c.tolist() == counts, fn.__name__
        assert n.tolist() == n_kmers, fn.__name__


def test_k_outside_1_to_32_is_refused():
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            H.screen(["ACGT"], [["ACGT"]], k)
        with pytest.raises(ValueError):
            H.screen_literal(["ACGT"], [["ACGT"]], k)


def test_screen_summary_on_a_hand_made_matrix():
    from seqwin_amd.markers import SCREEN_SUMMARY_DTYPE, screen_summary
    counts = np.array([[10, 9, 8, 0, 1],
                       [0, 0, 0, 0, 0],       # a query without a k-mer
                       [20, 18, 17, 18, 20],
                       [3, 3, 3, 3, 3]], np.uint32)
    n_kmers = np.array([10, 0, 20, 3], np.uint32)
    s = screen_summary((counts, n_kmers), n_tar=3, min_containment=0.9)
    assert s.dtype == SCREEN_SUMMARY_DTYPE and s["n_kmers"].tolist() == [10, 0, 20, 3]
    # row 0: targets 1.0, 0.9, 0.8 -> mean 0.9; 9 / 10 >= 0.9 sits ON the boundary and counts: 2 of 3.  Non-targets 0, 0.1
    assert s["containment_tar"][0] == (10 / 10 + 9 / 10 + 8 / 10) / 3 and s["f_tar"][0] == 2 / 3
    assert s["containment_neg"][0] == (0 / 10 + 1 / 10) / 2 and s["f_neg"][0] == 0.0
    for f in ("containment_tar", "f_tar", "containment_neg", "f_neg"):
        assert np.isnan(s[f][1]), f
    # row 2: 18 / 20 = 0.9 counts, 17 / 20 does not
    assert s["f_tar"][2] == 2 / 3 and s["f_neg"][2] == 1.0 and s["containment_neg"][2] == (18 / 20 + 20 / 20) / 2
    assert s["containment_tar"][3] == 1.0 and s["f_tar"][3] == 1.0 and s["f_neg"][3] == 1.0
    # the boundary moves with the threshold; an empty group reads nan
    assert screen_summary((counts, n_kmers), 3, min_containment=0.91)["f_tar"][0] == 1 / 3
    all_tar = screen_summary((counts, n_kmers), 5)
    assert np.isnan(all_tar["containment_neg"]).all() and np.isnan(all_tar["f_neg"]).all() and all_tar["f_tar"][3] == 1.0
    with pytest.raises(ValueError):
        screen_summary((counts, n_kmers), 6)
    with pytest.raises(ValueError):
        screen_summary((counts, n_kmers[:3]), 2)
