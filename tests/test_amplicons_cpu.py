"""The two host restatements of the amplicon stage (tests/tools/amplicons_host.py) against each other, against
hand-written product tables, and -- without probes and max_dg -- against seqwin_amd.oligos.amplicons on the same site dicts.  No GPU."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import amplicons_host as A  # noqa: E402

from seqwin_amd import oligos as O  # noqa: E402

COLS = ("oligo", "assembly", "record", "pos", "end", "strand", "dist")


def _sites(rows, dg=None, edit=False):
    """rows of (oligo, assembly, record, pos, end, strand, dist[, dg]) -> the dict OligoHits.sites() gives, in the list's order"""
    rows = sorted(rows, key=lambda r: (r[0], r[1], r[2], r[3], r[4], r[5]) if edit else (r[0], r[1], r[2], r[3], r[5]))
    S = {f: np.array([r[i] for r in rows], np.uint32) for i, f in enumerate(COLS)}
    if rows and len(rows[0]) > 7:
        S["dg"] = np.array([r[7] for r in rows], np.int32)
    if not edit:
        S["mm"] = S["dist"].copy()
    return S


def _same(x, y):
    for f in A.FIELDS + ("cell_offsets", "n_amplicons", "n_detected"):
        assert np.array_equal(x[f], y[f]), f


def _table(res):
    return [tuple(int(res[f][i]) for f in A.FIELDS) for i in range(len(res["pair"]))]


def _against_oligos(S, lengths, pairs, lo, hi, na, res):
    prod, n_amp = O.amplicons(S, lengths, pairs, lo, hi, n_assemblies=na)
    for f in O.AMPLICON_FIELDS:
        assert np.array_equal(prod[f].astype(np.uint32), res[f]), f
    assert np.array_equal(n_amp, res["n_amplicons"])


# oligos 0 = f, 1 = r, 2 = the probe, 10 letters each; two assemblies, records 0 and 1 in assembly 0, record 2 in assembly 1
HAND = [
    (0, 0, 0, 100, 110, 0, 0), (1, 0, 0, 190, 200, 1, 1),      # + : [100, 200), length 100 = max_len
    (1, 0, 0, 191, 201, 1, 0),                                 #     length 101: out
    (1, 0, 0, 300, 310, 0, 2), (0, 0, 0, 340, 350, 1, 0),      # - : [300, 350), length 50 = min_len
    (0, 0, 0, 339, 349, 1, 0),                                 #     length 49: out
    (2, 0, 0, 110, 120, 0, 0),                                 # the probe flush against f's site: counts
    (2, 0, 0, 180, 190, 1, 0),                                 # flush against r's site, other strand: counts
    (2, 0, 0, 181, 191, 1, 1),                                 # one base into r's site: does not count
    (2, 0, 0, 99, 109, 0, 0),                                  # before f's site
    (1, 0, 1, 60, 70, 1, 0),                                   # record 1 has no site of f: no product across the boundary
    (0, 1, 2, 5, 15, 0, 1), (1, 1, 2, 5, 15, 1, 0),            # + with pos_r == pf: [5, 15), too short at min_len 50
]


def test_hand_written_table_with_a_probe():
    S = _sites(HAND)
    want = [(0, 0, 0, 100, 200, 0, 0, 1, 2), (0, 0, 0, 300, 350, 1, 0, 2, 0)]
    for form in (A.amplicons_loop, A.amplicons_merge):
        res = form(S, [(0, 1)], 50, 100, 2, probes=[2])
        assert _table(res) == want
        assert res["n_amplicons"].tolist() == [[2, 0]] and res["n_detected"].tolist() == [[1, 0]]
        assert res["cell_offsets"].tolist() == [0, 2, 2]
    # the bounds one wider on each side let the two neighbours in; a pair given twice is two rows; a pair without a probe next to one with
    for form in (A.amplicons_loop, A.amplicons_merge):
        res = form(S, [(0, 1), (0, 1)], 49, 101, 2, probes=[None, 2])
        rows = [(0, 0, 100, 200, 0, 0, 1), (0, 0, 100, 201, 0, 0, 0), (0, 0, 300, 349, 1, 0, 2), (0, 0, 300, 350, 1, 0, 2)]
        assert _table(res) == [(0,) + r + (0,) for r in rows] + [(1,) + r + (n,) for r, n in zip(rows, (2, 3, 0, 0))]
        assert res["n_detected"].tolist() == [[0, 0], [2, 0]]


def test_hand_written_equal_positions_and_self_pairs():
    S = _sites(HAND)
    for form in (A.amplicons_loop, A.amplicons_merge):
        res = form(S, [(0, 1), (1, 0)], 1, 10, 2)
        # pair (0, 1): + in record 2; pair (1, 0): its - is the same place, and there f is oligo 1 (d 0), r oligo 0 (d 1)
        assert _table(res) == [(0, 1, 2, 5, 15, 0, 1, 0, 0), (1, 1, 2, 5, 15, 1, 0, 1, 0)]
        _against_oligos(S, [10, 10, 10], [(0, 1), (1, 0)], 1, 10, 2, res)
    # an oligo that is its own reverse complement sits on both strands of one place; with f == r only + is formed
    P = _sites([(0, 0, 0, 40, 52, 0, 0), (0, 0, 0, 40, 52, 1, 0), (0, 0, 0, 70, 82, 0, 1), (0, 0, 0, 70, 82, 1, 1)])
    for form in (A.amplicons_loop, A.amplicons_merge):
        res = form(P, [(0, 0)], 12, 42, 1)
        assert _table(res) == [(0, 0, 0, 40, 52, 0, 0, 0, 0), (0, 0, 0, 40, 82, 0, 0, 1, 0), (0, 0, 0, 70, 82, 0, 1, 1, 0)]
        _against_oligos(P, [12], [(0, 0)], 12, 42, 1, res)


def test_hand_written_edit_ends_and_dg_filter():
    # an edit result: the last site's own end decides the bound, and a probe site with a bulge ends a base later
    E = _sites([(0, 0, 0, 10, 20, 0, 0), (1, 0, 0, 100, 111, 1, 1), (1, 0, 0, 101, 110, 1, 1),
                (2, 0, 0, 50, 61, 0, 1), (2, 0, 0, 90, 101, 1, 1)], edit=True)
    for form in (A.amplicons_loop, A.amplicons_merge):
        res = form(E, [(0, 1)], 1, 100, 1, probes=[2])
        # [10, 111) is 101 long: out, though pos 100 + L 10 would be in; [10, 110) is in, though pos 101 + L would be out
        # the probe at [90, 101) ends at pos_last 101: counts; so does [50, 61)
        assert _table(res) == [(0, 0, 0, 10, 110, 0, 0, 1, 2)]
    D = _sites([(0, 0, 0, 10, 20, 0, 0, -9000), (0, 0, 0, 30, 40, 0, 2, -4000), (1, 0, 0, 80, 90, 1, 0, -8000), (1, 0, 0, 95, 105, 1, 1, -5000),
                (2, 0, 0, 50, 60, 0, 3, -100)])
    for form in (A.amplicons_loop, A.amplicons_merge):
        assert len(form(D, [(0, 1)], 1, 200, 1, probes=[2])["pair"]) == 4
        res = form(D, [(0, 1)], 1, 200, 1, probes=[2], max_dg=-6000)
        assert _table(res) == [(0, 0, 0, 10, 90, 0, 0, 0, 1)]   # the primers are filtered, the probe (dg -100) is not


def _random_sites(rng, n_oligos, n_asm, recs_per_asm, n, edit, span=400, with_dg=False):
    rows = set()
    while len(rows) < n:
        q, a = rng.randrange(n_oligos), rng.randrange(n_asm)
        rec = a * recs_per_asm + rng.randrange(recs_per_asm)
        pos = rng.randrange(span)
        L = 10 + q
        end = pos + L + (rng.randrange(-2, 3) if edit else 0)
        rows.add((q, a, rec, pos, end, rng.randrange(2)))
    return _sites([r + (rng.randrange(0, 4),) + ((rng.randrange(-9000, 0),) if with_dg else ()) for r in rows], edit=edit)


@pytest.mark.parametrize("edit", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_forms_agree_on_random_sites(seed, edit):
    rng = random.Random(seed * 2 + edit)
    n_oligos, n_asm = 5, 3
    S = _random_sites(rng, n_oligos, n_asm, 2, 260, edit, with_dg=not edit)
    pairs = [(0, 1), (1, 0), (2, 2), (3, 4), (0, 1), (4, 0)]
    probes = [2, None, 0, 1, 3, A.NO_PROBE]
    lengths = [10 + q for q in range(n_oligos)]
    for lo, hi in ((1, 60), (20, 150), (35, 35)):
        plain = A.amplicons_loop(S, pairs, lo, hi, n_asm)
        _same(plain, A.amplicons_merge(S, pairs, lo, hi, n_asm))
        assert plain["n_probe"].sum() == 0 and plain["n_detected"].sum() == 0
        _against_oligos({k: v for k, v in S.items() if edit or k != "end"}, lengths, pairs, lo, hi, n_asm, plain)
        with_probe = A.amplicons_loop(S, pairs, lo, hi, n_asm, probes=probes)
        _same(with_probe, A.amplicons_merge(S, pairs, lo, hi, n_asm, probes=probes))
        for f in A.FIELDS[:8]:
            assert np.array_equal(with_probe[f], plain[f]), f
        if not edit:
            filt = A.amplicons_loop(S, pairs, lo, hi, n_asm, probes=probes, max_dg=-4000)
            _same(filt, A.amplicons_merge(S, pairs, lo, hi, n_asm, probes=probes, max_dg=-4000))
            assert len(filt["pair"]) <= len(plain["pair"])
    assert len(A.amplicons_loop(S, pairs, 1, 150, n_asm, probes=probes)["pair"]) > 20
    assert A.amplicons_loop(S, pairs, 1, 150, n_asm, probes=probes)["n_detected"].sum() > 0
