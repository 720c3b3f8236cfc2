"""CPU: the host restatement of all seeded loci per (query, assembly) (tests/tools/loci_host.py) -- its two
forms against each other and against hand-made cases whose lists are written out in tests/tools/loci_cases.py, and its invariants on
random cases: the locus of a cell with the most seeds (ties to the smallest record, strand, band) is the winner of section 3.2e and
carries exactly align_host.best_hits_aligned's fields."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import loci_cases as C  # noqa: E402
import loci_host as L  # noqa: E402

CASES = C.hand_made()
KEYS = L.LIST_FIELDS + ("lo", "hi", "cell_offsets", "n_loci", "sum_nident", "n_candidates")


def _both(queries, asms, min_seeds=1):
    a = L.best_hits_loci(queries, asms, C.K, min_seeds)
    b = L.best_hits_loci_literal(queries, asms, C.K, min_seeds)
    assert set(a) == set(b) == set(KEYS)
    for f in KEYS:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), f
    return a


def _rows(got):
    return [tuple(int(got[f][j]) for f in C.COLS) for j in range(len(got["query"]))]


def _winner_is_a_locus(queries, asms, got):
    """The cell's locus with the most seeds, ties to the smallest (record, strand, band), carries best_hits_aligned's fields."""
    want = A.best_hits_aligned(queries, asms, C.K)
    nq, na = want["seeds"].shape
    offs = got["cell_offsets"].astype(np.int64)
    assert offs.shape == (nq * na + 1,) and got["cell_offsets"].dtype == np.uint64 and offs[-1] == len(got["query"])
    for q in range(nq):
        for a in range(na):
            seg = range(offs[q * na + a], offs[q * na + a + 1])
            assert (len(seg) > 0) == (want["seeds"][q, a] > 0)
            assert all(got["query"][j] == q and got["assembly"][j] == a for j in seg)
            if not len(seg):
                assert got["n_loci"][q, a] == 0 and got["sum_nident"][q, a] == 0
                continue
            j = min(seg, key=lambda j: (-int(got["seeds"][j]), int(got["record"][j]), int(got["strand"][j]), int(got["band"][j])))
            for f in ("seeds", "record", "strand", "end", "dist", "start", "nident", "mismatch", "gaps", "lo", "hi"):
                assert got[f][j] == want[f][q, a], (q, a, f)
            keep = [j for j in seg if not got["dup"][j]]
            assert got["n_loci"][q, a] == len(keep) and got["sum_nident"][q, a] == sum(int(got["nident"][j]) for j in keep)
    return want


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made(name):
    queries, asms, rows = CASES[name]
    got = _both(queries, asms)
    have = _rows(got)
    assert len(have) == len(rows), have
    for h, w in zip(have, rows):
        assert all(x == y for x, y in zip(h, w) if y is not None), (h, w)
    assert np.all(got["mismatch"] + got["gaps"] == got["dist"]) and np.all(got["start"] <= got["end"])
    _winner_is_a_locus(queries, asms, got)
    n_loci = np.zeros((len(queries), len(asms)), np.uint32)
    sums = np.zeros_like(n_loci)
    for h in have:
        if not h[12]:
            n_loci[h[0], h[1]] += 1
            sums[h[0], h[1]] += h[9]
    assert np.array_equal(got["n_loci"], n_loci) and np.array_equal(got["sum_nident"], sums)


def test_expectations_of_the_cases():
    """What each scenario is there for, said once more on the lists."""
    n = {name: _both(*CASES[name][:2]) for name in CASES}
    assert n["two_copies"]["n_loci"].tolist() == [[2]] and n["two_copies"]["sum_nident"].tolist() == [[120]]
    assert n["suppression"]["n_loci"].tolist() == [[1, 1]]                           # four copies, two loci
    assert n["suppression"]["n_candidates"] == 4 and n["two_copies"]["n_candidates"] == 2
    assert n["strands_records"]["n_loci"].tolist() == [[3]]
    assert n["mutations"]["sum_nident"].tolist() == [[60, 59, 59]]
    assert n["duplicate"]["dup"].tolist() == [0, 1] and n["duplicate"]["n_loci"].tolist() == [[1]] and n["duplicate"]["sum_nident"].tolist() == [[60]]
    assert n["last_band"]["band"].tolist() == [14, 0] and n["last_band"]["strand"].tolist() == [0, 1]
    assert n["empty"]["n_loci"].tolist() == [[0, 0], [0, 0], [0, 1]]


def test_min_seeds_drops_the_locus_and_keeps_the_winner():
    queries, asms, rows = CASES["single_seed"]
    one, two = _both(queries, asms, 1), _both(queries, asms, 2)
    assert one["n_loci"].tolist() == [[1, 1]] and one["seeds"].tolist() == [50, 1]
    assert two["n_loci"].tolist() == [[1, 0]] and two["sum_nident"][0, 1] == 0 and two["seeds"].tolist() == [50]
    assert two["cell_offsets"].tolist() == [0, 1, 1]
    want = A.best_hits_aligned(queries, asms, C.K)       # the matrix fields know nothing of min_seeds
    assert want["seeds"].tolist() == [[50, 1]] and want["nident"][0, 1] == one["nident"][1]
    for form in (L.best_hits_loci, L.best_hits_loci_literal):
        with pytest.raises(ValueError, match="min_seeds"):
            form(queries, asms, C.K, 0)


@pytest.mark.parametrize("seed", range(6))
def test_random_invariants(seed):
    queries, asms = C.random_small(seed)
    got = _both(queries, asms)
    _winner_is_a_locus(queries, asms, got)
    order = [(r[0], r[2], r[3], r[4]) for r in _rows(got)]
    assert order == sorted(order) and len(set(order)) == len(order)
    for ms in (2, 5):
        sub = _both(queries, asms, ms)
        keep = got["seeds"] >= ms                         # a higher floor only removes entries: the suppression looks at all candidates
        for f in L.LIST_FIELDS[:12]:
            assert np.array_equal(sub[f], got[f][keep]), f
