"""CPU: the two host restatements of the oligo search (tests/tools/oligo_host.py) against each other and on hand-made cases whose
every figure is written out, `seqwin_amd.oligos.amplicons` against its restatement and on hand-made site lists, the two summaries,
and the ValueErrors a call raises before a device is touched (the Python check and the library's own)."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oligo_host as H  # noqa: E402

from seqwin_amd import oligos as O  # noqa: E402

NO_HIT = 0xFFFFFFFF


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---- the two forms against each other ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alphabet,seed", [(b"ACGT", 1), (b"AC", 2), (b"ACGT", 3)])
def test_the_two_forms_agree(alphabet, seed):
    """Random 4-letter and 2-letter texts (on two letters, with 7 mismatches, the short oligos hit nearly everywhere), with Ns, lower case and
    U in the text and IUPAC codes in the oligos; every max_mismatch / three_prime of the GPU tests."""
    rng = random.Random(seed)
    asms = []
    for a in range(3):
        recs = []
        for r in range(2):
            t = bytearray(_rand(rng, rng.randrange(5, 140), alphabet))
            for _ in range(rng.randrange(0, 3)):
                t[rng.randrange(len(t))] = ord(rng.choice("NnRy-"))
            if r:
                t = bytearray(bytes(t).lower().replace(b"t", b"u"))
            recs.append(bytes(t))
        asms.append(recs)
    oligos = [_rand(rng, n, alphabet) for n in (8, 9, 15, 16, 17, 31, 32)] + [b"ACGTNNRY", b"acgurykm", asms[0][0][3:13].replace(b"-", b"N"), H.revcomp(b"AAAACCCCAC")]
    for max_mm, clamp in ((0, 0), (1, 1), (3, 5), (7, 0), (3, 8)):
        a, b = H.sites_loop(oligos, asms, max_mm, clamp), H.sites_planes(oligos, asms, max_mm, clamp)
        assert a == b
        if alphabet == b"AC" and max_mm == 7:
            assert len(a) > 100


# ---- hand-made cases ---------------------------------------------------------------------------------------------------------------

def test_a_degenerate_letter_saves_a_mismatch():
    """text GATTACAGGA, oligo GATTACAC: at pos 0 the window GATTACAG differs in its last base only (G against C): mm = 1.  With
    GATTACAS (S = C or G) the same window has mm = 0.  No other window and no window of the reverse complement comes within 1."""
    asm = [[b"GATTACAGGA"]]
    assert H.sites_loop([b"GATTACAC"], asm, 1) == [(0, 0, 0, 0, 0, 1)]
    assert H.sites_loop([b"GATTACAC"], asm, 0) == []
    assert H.sites_loop([b"GATTACAS"], asm, 0) == [(0, 0, 0, 0, 0, 0)]
    assert H.sites_planes([b"GATTACAS"], asm, 0) == [(0, 0, 0, 0, 0, 0)]


def test_the_clamp_on_either_strand():
    """oligo AAAACCCC, its reverse complement GGGGTTTT.
    Record 0 = AAAACCCG: strand 0 at pos 0, one mismatch at position 7, the oligo's 3' end: a hit with three_prime = 0, none with 1.
    Record 1 = CAAACCCC: strand 0 at pos 0, one mismatch at position 0, the 5' end: a hit with three_prime = 0, 1 and 7, none with 8.
    Record 2 = CGGGTTTT: strand 1 at pos 0, the mismatch at the window's position 0 -- on strand 1 that IS the oligo's 3' end: a hit
    with three_prime = 0, none with 1.
    Record 3 = GGGGTTTA: strand 1 at pos 0, the mismatch at the window's position 7, the oligo's 5' end: a hit with 0, 1 and 7."""
    asm = [[b"AAAACCCG", b"CAAACCCC", b"CGGGTTTT", b"GGGGTTTA"]]
    o = [b"AAAACCCC"]
    for form in (H.sites_loop, H.sites_planes):
        assert form(o, asm, 1, 0) == [(0, 0, 0, 0, 0, 1), (0, 0, 1, 0, 0, 1), (0, 0, 2, 0, 1, 1), (0, 0, 3, 0, 1, 1)]
        assert form(o, asm, 1, 1) == [(0, 0, 1, 0, 0, 1), (0, 0, 3, 0, 1, 1)]
        assert form(o, asm, 1, 7) == [(0, 0, 1, 0, 0, 1), (0, 0, 3, 0, 1, 1)]
        assert form(o, asm, 1, 8) == []


def test_a_palindromic_oligo_gives_two_sites():
    """ACGTACGT is its own reverse complement.  In TTACGTACGTTT it lies at pos 2: a site on strand 0 and a site on strand 1, both
    with mm = 0; n_sites = 2 and the best site is the strand-0 one."""
    asm = [[b"TTACGTACGTTT"]]
    for form in (H.sites_loop, H.sites_planes):
        assert form([b"ACGTACGT"], asm, 0) == [(0, 0, 0, 2, 0, 0), (0, 0, 0, 2, 1, 0)]
    r = H.search([b"ACGTACGT"], asm, 0)
    assert r["n_sites"].tolist() == [[2]] and r["best_strand"].tolist() == [[0]] and r["best_pos"].tolist() == [[2]]


def test_the_tie_order_of_the_best_site():
    """oligo AAAACCCC, max_mismatch 1, one assembly of three records:
    record 0 = TAAACCCCT:           pos 0 TAAACCCC strand 0 mm 1 (pos 1 AAACCCCT has mm 2: no hit)
    record 1 = GGAAAACCCCGGGGTTTT:  pos 2 strand 0 mm 0, pos 10 strand 1 mm 0 (GGGGTTTT)
    record 2 = AAAACCCC:            pos 0 strand 0 mm 0
    The order is (mm, record, pos, strand): the mm-1 site of record 0 loses to the mm-0 sites although its record is smaller; among
    those record 1 wins over record 2, and in record 1 pos 2 over pos 10."""
    asm = [[b"TAAACCCCT", b"GGAAAACCCCGGGGTTTT", b"AAAACCCC"]]
    S = H.sites_loop([b"AAAACCCC"], asm, 1)
    assert S == [(0, 0, 0, 0, 0, 1), (0, 0, 1, 2, 0, 0), (0, 0, 1, 10, 1, 0), (0, 0, 2, 0, 0, 0)]
    r = H.search([b"AAAACCCC"], asm, 1, form=H.sites_loop)
    assert (r["n_sites"][0, 0], r["best_mm"][0, 0], r["best_record"][0, 0], r["best_pos"][0, 0], r["best_strand"][0, 0]) == (4, 0, 1, 2, 0)
    assert r["sites"]["cell_offsets"].tolist() == [0, 4]


def test_a_window_over_an_n_is_no_site():
    """AAAACNCCAAAACCCC: the oligo AAAACCCC would fit pos 0 with one mismatch (N against C), but that window touches an invalid base:
    no site, at any max_mismatch.  The copy at pos 8 is the only hit.  A second assembly without a valid run of 8 bases has none:
    its cell is NO_HIT with n_sites 0."""
    asms = [[b"AAAACNCCAAAACCCC"], [b"AAAACCCNAAACCCC", b"ACGT"]]
    for mm in (0, 1, 7):
        for form in (H.sites_loop, H.sites_planes):
            assert [s[:5] for s in form([b"AAAACCCC"], asms, mm) if s[5] <= 1] == [(0, 0, 0, 8, 0)]
    r = H.search([b"AAAACCCC"], asms, 1)
    assert r["n_sites"].tolist() == [[1, 0]] and r["best_mm"].tolist() == [[0, NO_HIT]] and r["best_record"].tolist() == [[0, NO_HIT]]


# ---- amplicons -------------------------------------------------------------------------------------------------------------------

def _list(rows):
    cols = np.array(rows, np.uint32).reshape(-1, 6)
    return {f: cols[:, i] for i, f in enumerate(("oligo", "assembly", "record", "pos", "strand", "mm"))}


def _rows(P):
    return [tuple(int(P[f][i]) for f in O.AMPLICON_FIELDS) for i in range(len(P["pair"]))]


def test_amplicons_both_orientations():
    """oligo 0 = f (20 long), oligo 1 = r (18 long); pair (0, 1).
    record 5 (assembly 0): f strand 0 at 100 (mm 1), r strand 1 at 300 (mm 0): `+`, product [100, 318).
    record 9 (assembly 2): r strand 0 at 50 (mm 2), f strand 1 at 400 (mm 0): `-`, product [50, 420).
    record 9 also has f strand 0 at 500 -- behind every strand-1 site: no product."""
    S = _list([(0, 0, 5, 100, 0, 1), (0, 2, 9, 400, 1, 0), (0, 2, 9, 500, 0, 0), (1, 0, 5, 300, 1, 0), (1, 2, 9, 50, 0, 2)])
    P, n = O.amplicons(S, [20, 18], [(0, 1)], 50, 1000, n_assemblies=3)
    assert _rows(P) == [(0, 0, 5, 100, 318, 0, 1, 0), (0, 2, 9, 50, 420, 1, 0, 2)]
    assert n.tolist() == [[1, 0, 1]] and n.dtype == np.uint32
    assert H.amplicons(S, [20, 18], [(0, 1)], 50, 1000, 3)[0] == _rows(P)


def test_amplicons_with_f_equal_r_count_plus_only():
    """One oligo (10 long) as both primers: strand 0 at 10, strand 1 at 90 -> one `+` product [10, 100); `-` would name the same two
    sites again and is not counted."""
    S = _list([(0, 0, 0, 10, 0, 0), (0, 0, 0, 90, 1, 0)])
    P, n = O.amplicons(S, [10], [(0, 0)], 1, 1000, n_assemblies=1)
    assert _rows(P) == [(0, 0, 0, 10, 100, 0, 0, 0)] and n.tolist() == [[1]]
    assert H.amplicons(S, [10], [(0, 0)], 1, 1000, 1)[0] == _rows(P)


def test_amplicon_length_bounds_are_inclusive():
    """f (8 long) strand 0 at 0, r (8 long) strand 1 at 92: the product [0, 100) has 100 bases: kept for bounds 100..100, 99..100 and
    100..101, dropped for 101..200 and 50..99.  pf == pr (two 8-base sites at one place) gives a product of 8 bases."""
    S = _list([(0, 0, 0, 0, 0, 0), (1, 0, 0, 92, 1, 0)])
    for lo, hi, want in ((100, 100, 1), (99, 100, 1), (100, 101, 1), (101, 200, 0), (50, 99, 0)):
        P, n = O.amplicons(S, [8, 8], [(0, 1)], lo, hi, n_assemblies=1)
        assert n.tolist() == [[want]] and len(P["pair"]) == want
    S = _list([(0, 0, 0, 7, 0, 0), (1, 0, 0, 7, 1, 0)])
    P, n = O.amplicons(S, [8, 8], [(0, 1)], 8, 8, n_assemblies=1)
    assert _rows(P) == [(0, 0, 0, 7, 15, 0, 0, 0)]


def test_two_forward_by_two_reverse_sites_give_four_products():
    """f strand 0 at 0 and 10, r strand 1 at 200 and 300 (both 20 long) in one record: [0, 220), [0, 320), [10, 220), [10, 320);
    the same sites in another record of another assembly do not combine across records."""
    S = _list([(0, 0, 0, 0, 0, 0), (0, 0, 0, 10, 0, 1), (0, 1, 1, 0, 0, 0), (1, 0, 0, 200, 1, 0), (1, 0, 0, 300, 1, 2), (1, 1, 2, 200, 1, 0)])
    P, n = O.amplicons(S, [20, 20], [(0, 1)], 1, 10_000, n_assemblies=2)
    assert _rows(P) == [(0, 0, 0, 0, 220, 0, 0, 0), (0, 0, 0, 0, 320, 0, 0, 2), (0, 0, 0, 10, 220, 0, 1, 0), (0, 0, 0, 10, 320, 0, 1, 2)]
    assert n.tolist() == [[4, 0]]


def test_amplicons_against_the_restatement_on_random_lists():
    rng = random.Random(11)
    for _ in range(5):
        rows = sorted({(rng.randrange(3), 0, rng.randrange(2), rng.randrange(60), rng.randrange(2), rng.randrange(3)) for _ in range(40)})
        rows = [(q, r, r, p, s, m) for q, _, r, p, s, m in rows]          # (assembly = record here)
        rows = sorted({r[:5]: r for r in rows}.values())                  # one mm per site
        S = _list(rows)
        lengths, pairs = [8, 12, 20], [(0, 1), (1, 0), (2, 2), (0, 2)]
        P, n = O.amplicons(S, lengths, pairs, 15, 45, n_assemblies=2)
        want, wn = H.amplicons(S, lengths, pairs, 15, 45, 2)
        assert _rows(P) == want and np.array_equal(n, wn)


def test_summaries():
    n = np.array([[1, 0, 2, 0], [0, 0, 0, 0], [3, 1, 0, 1]], np.uint32)
    best = np.array([[0, NO_HIT, 2, NO_HIT], [NO_HIT] * 4, [1, 3, NO_HIT, 0]], np.uint32)
    s = O.oligo_summary(dict(n_sites=n, best_mm=best), 2)
    assert s["f_tar"].tolist() == [0.5, 0.0, 1.0] and s["f_neg"].tolist() == [0.5, 0.0, 0.5]
    assert s["mean_best_mm_tar"][0] == 0.0 and np.isnan(s["mean_best_mm_tar"][1]) and s["mean_best_mm_tar"][2] == 2.0
    a = O.assay_summary(np.array([[1, 2, 0, 0], [0, 0, 1, 1], [1, 1, 0, 3]], np.uint32), 2)
    assert a["f_tar_amplified"].tolist() == [1.0, 0.0, 1.0] and a["f_tar_single"].tolist() == [0.5, 0.0, 1.0]
    assert a["f_neg_amplified"].tolist() == [0.0, 1.0, 0.5]


# ---- the ValueErrors -------------------------------------------------------------------------------------------------------------

BAD = [
    (dict(oligos=[]), "oligos"),
    (dict(oligos=[b"ACGTACGT"] * 4097), "oligos"),
    (dict(oligos=[b"ACGTACG"]), "letters"),
    (dict(oligos=[b"A" * 33]), "letters"),
    (dict(oligos=[b"ACGTACGX"]), "IUPAC"),
    (dict(oligos=[b"ACGT-CGT"]), "IUPAC"),
    (dict(oligos=[b"ACGTACGT"], max_mismatch=8), "max_mismatch"),
    (dict(oligos=[b"ACGTACGTAC"], max_mismatch=9), "max_mismatch"),
    (dict(oligos=[b"ACGTACGT"], max_mismatch=-1), "max_mismatch"),
    (dict(oligos=[b"ACGTACGT"], three_prime=9), "three_prime"),
]


@pytest.mark.parametrize("kw,match", BAD)
def test_value_errors_of_the_python_check(kw, match):
    with pytest.raises(ValueError, match=match):
        O.check_oligos(**kw)


def test_the_python_check_takes_what_is_allowed():
    assert O.check_oligos(["acgurykm", b"N" * 32], 7, 8) == [b"acgurykm", b"N" * 32]
    assert O.check_oligos([b"ACGTACGTA"], 8, 0) == [b"ACGTACGTA"]
    with pytest.raises(ValueError, match="list"):
        O.check_oligos("ACGTACGT")


@pytest.mark.parametrize("kw,match", [b for b in BAD if b[0].get("max_mismatch", 0) >= 0])
def test_value_errors_of_the_library_before_a_device_is_touched(kw, match):
    """sw_batch_oligo_hits checks its oligos before it looks at the batch: with a NULL batch a bad call names its own fault."""
    from seqwin_amd._core import _ptr
    from seqwin_amd._lib import c_u64, c_vp, check, lib
    qs = kw["oligos"]
    offs = np.zeros(len(qs) + 1, np.uint64)
    np.cumsum([len(q) for q in qs], out=offs[1:])
    h = c_vp()
    with pytest.raises(ValueError, match=match):
        check(lib.sw_batch_oligo_hits(None, _ptr(offs), b"".join(qs), c_u64(len(qs)), c_u64(kw.get("max_mismatch", 0)), c_u64(kw.get("three_prime", 0)),
                                      ctypes.c_int(0), c_vp(0), ctypes.byref(h)))
    with pytest.raises(ValueError, match="NULL"):     # a good call but no batch
        offs = np.array([0, 8], np.uint64)
        check(lib.sw_batch_oligo_hits(None, _ptr(offs), b"ACGTACGT", c_u64(1), c_u64(0), c_u64(0), ctypes.c_int(0), c_vp(0), ctypes.byref(h)))
