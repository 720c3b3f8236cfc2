"""CPU: the oligo windows' specification in its two host restatements (tests/tools/windows_host.py) --
against each other, against tables written out by hand, against the sum invariant and the strand symmetry --, the readers of
seqwin_amd/pileup.py on a hand-made table, and the ValueErrors a call raises before a device is touched.  The device side is compared
with the same restatement in tests/test_gpu_windows_direct.py and tests/test_gpu_best_hits_windows.py."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import hits_host as H  # noqa: E402
import pileup_host as P  # noqa: E402
import windows_host as W  # noqa: E402

from seqwin_amd import pileup as R  # noqa: E402

OPS = {ch: i for i, ch in enumerate("=XID")}
MM0, MM1, MM2, MM3, MM4P, GAPPED, FWD, REV = range(8)
PERFECT = (MM0, FWD, REV)


def _both(m, strand, ops, lengths, mm, c3):
    """One script through both forms: [m, n_lengths, 8] each."""
    out = []
    for form in (W.add_script_loops, W.add_script_prefix):
        rows = np.zeros((m, len(lengths), 1, 8), np.uint32)
        form(rows, 0, strand, np.array([OPS[o] for o in ops], np.uint8), list(lengths), mm, c3)
        out.append(rows[:, :, 0])
    return out


def _table(m, n_lengths, *cells):
    """cells: (u, l, classes that get 1)"""
    out = np.zeros((m, n_lengths, 8), np.uint32)
    for u, l, classes in cells:
        for c in classes:
            out[u, l, c] += 1
    return out


# name: (strand, ops, lengths, max_mismatch, three_prime, m, the table by hand: (start u, length index, classes))
HAND = {
    # X at pattern index 2 lies in all three windows of 8; on strand 0 it is among the first 3 positions of each, never among the last 3
    "one X near the left end": (0, "==X=======", (8,), 1, 3, 10, [(0, 0, (MM1, FWD)), (1, 0, (MM1, FWD)), (2, 0, (MM1, FWD))]),
    # strand 1: pattern index 2 is query position 7: among the last 3 of the windows at u = 0 (5..7), 1 (6..8) and 2 (7..9)
    "one X, strand 1": (1, "==X=======", (8,), 1, 3, 10, [(0, 0, (MM1, REV)), (1, 0, (MM1, REV)), (2, 0, (MM1, REV))]),
    # X at index 4: distance 3 from the left end of window 1 (clean), distance 2 from it in window 2 (left_bad)
    "X at distance c and c - 1 from the left end": (0, "====X=====", (8,), 1, 3, 10, [(0, 0, (MM1, FWD, REV)), (1, 0, (MM1, FWD, REV)), (2, 0, (MM1, FWD))]),
    # X at index 5: the last 3 of window 0 are 5..7 (right_bad), of window 1 6..8 (clean)... and of window 2 7..9
    "X at distance c and c - 1 from the right end": (0, "=====X====", (8,), 1, 3, 10, [(0, 0, (MM1, REV)), (1, 0, (MM1, FWD, REV)), (2, 0, (MM1, FWD, REV))]),
    "three_prime 0": (0, "X======X", (8,), 2, 0, 8, [(0, 0, (MM2, FWD, REV))]),
    "three_prime 8 is the whole window of 8": (0, "===X====", (8,), 2, 8, 8, [(0, 0, (MM1,))]),
    "e above max_mismatch": (0, "===XX===", (8,), 1, 3, 8, [(0, 0, (MM2,))]),
    "e equal to max_mismatch": (0, "===XX===", (8,), 2, 3, 8, [(0, 0, (MM2, FWD, REV))]),
    "e = 3": (0, "==XXX===", (8,), 3, 2, 8, [(0, 0, (MM3, FWD, REV))]),
    "e = 4": (0, "==XXXX==", (8,), 4, 2, 8, [(0, 0, (MM4P, FWD, REV))]),
    "e = 5": (0, "==XXXXX=", (8,), 5, 1, 8, [(0, 0, (MM4P, FWD, REV))]),
    # a run of D before pattern index 1: inside window 0 (0 < 1 < 8), at the edge of window 1, outside window 2
    "D run at slot u + 1 and u": (0, "=DD=========", (8,), 2, 3, 10, [(0, 0, (GAPPED,)), (1, 0, PERFECT), (2, 0, PERFECT)]),
    # before pattern index 8: at the far edge of window 0 (s + L), inside windows 1 and 2
    "D run at slot u + L and u + L - 1": (0, "========D==", (8,), 2, 3, 10, [(0, 0, PERFECT), (1, 0, (GAPPED,)), (2, 0, (GAPPED,))]),
    # strand 1: pattern windows s = 0, 1, 2 are the query windows u = 2, 1, 0
    "D run, strand 1": (1, "=D=========", (8,), 2, 3, 10, [(2, 0, (GAPPED,)), (1, 0, PERFECT), (0, 0, PERFECT)]),
    "I at a window's first position": (0, "=I========", (8,), 2, 3, 10, [(0, 0, (GAPPED,)), (1, 0, (GAPPED,)), (2, 0, PERFECT)]),
    "I at a window's last position": (0, "========I=", (8,), 2, 3, 10, [(0, 0, PERFECT), (1, 0, (GAPPED,)), (2, 0, (GAPPED,))]),
    "an empty text": (0, "IIIIIIIIII", (8,), 2, 3, 10, [(0, 0, (GAPPED,)), (1, 0, (GAPPED,)), (2, 0, (GAPPED,))]),
    # the table follows the order of the lengths given; the query has one window of 10 and three of 8
    "two lengths in the order given": (0, "X=========", (10, 8), 1, 3, 10, [(0, 0, (MM1, FWD)), (0, 1, (MM1, FWD)), (1, 1, PERFECT), (2, 1, PERFECT)]),
    "a query one base short of the length": (0, "=======", (8,), 1, 3, 7, []),
    "a gapped window is neither FWD_OK nor REV_OK, whatever its X": (0, "====I===X", (8,), 8 - 1, 0, 9, [(0, 0, (GAPPED,)), (1, 0, (GAPPED,))]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_scripts(name):
    strand, ops, lengths, mm, c3, m, cells = HAND[name]
    want = _table(m, len(lengths), *cells)
    loops, prefix = _both(m, strand, ops, lengths, mm, c3)
    assert np.array_equal(loops, want), (name, np.argwhere(loops != want).tolist())
    assert np.array_equal(prefix, want), (name, np.argwhere(prefix != want).tolist())


def test_hand_made_pairs_filter_and_labels():
    """Whole pairs through both forms: the scripts are section 3.2f's; a pair over the bound or labelled 0xFF adds nothing; an
    empty text is GAPPED everywhere; an invalid base on either side is an X."""
    queries = [b"ACGTACGTAC", b"ACGTNCGTAC", b""]
    records = [b"GGACGTACGTACGG", b"GGACGTTCGTACGG", H.revcomp(b"GGACGTTCGTACGG"), b"GGACGTNCGTACGG"]
    pairs = np.array([(0, 0, 0, 0, 14),     # a clean copy
                      (0, 0, 1, 0, 14),     # ====X=====
                      (0, 1, 2, 0, 14),     # the same copy from the other strand
                      (0, 0, 0, 3, 3),      # an empty text
                      (1, 0, 0, 0, 14),     # the query's N is an X
                      (0, 0, 3, 0, 14),     # the text's N is an X
                      (2, 0, 0, 0, 14),     # an empty query
                      (0, 0, 1, 0, 14)])    # left out by its label
    groups = [0, 0, 1, 1, 0, 1, 0, P.LEAVE_OUT]
    al = A.alignments(queries, records, pairs)
    o = al["offsets"].astype(np.int64)
    scripts = ["".join(A.OPS[x] for x in al["ops"][o[i]:o[i + 1]]) for i in range(len(pairs))]
    assert scripts == ["=" * 10, "====X=====", "=====X====", "I" * 10, "====X=====", "====X=====", "", "====X====="]
    want = np.zeros((20, 1, 2, 8), np.uint32)
    for u in range(3):
        want[u, 0, 0, [MM0, FWD, REV]] += 1                        # pair 0
        want[u, 0, 1, GAPPED] += 1                                # pair 3
    # an X at query position 4: outside the tails of the windows 0..7 and 1..8, among the first three (2..4) of the window 2..9
    x_at_4 = {0: (MM1, FWD, REV), 1: (MM1, FWD, REV), 2: (MM1, FWD)}
    for u, classes in x_at_4.items():
        want[u, 0, 0, list(classes)] += 1                         # pair 1
        want[u, 0, 1, list(classes)] += 1                         # pair 2: strand 1, pattern index 5 is query position 4
        want[10 + u, 0, 0, list(classes)] += 1                    # pair 4
        want[u, 0, 1, list(classes)] += 1                         # pair 5
    for form in W.FORMS:
        got = W.windows_ops(queries, records, pairs, groups, 2, (8,), 1, 3, al=al, form=form)
        assert np.array_equal(got["wtable"], want), (form, np.argwhere(got["wtable"] != want).tolist())
        assert got["depth"].tolist() == [[2, 3], [1, 0], [1, 0]]
        W.invariants(got["wtable"], got["depth"], got["q_offsets"], (8,))
        # the bound: dist 1 of 10 bases is 100 permille
        at99 = W.windows_ops(queries, records, pairs, groups, 2, (8,), 1, 3, max_dist_permille=99, al=al, form=form)
        assert at99["depth"].tolist() == [[1, 0], [0, 0], [1, 0]] and int(at99["wtable"].sum()) == 3 * 3
        at100 = W.windows_ops(queries, records, pairs, groups, 2, (8,), 1, 3, max_dist_permille=100, al=al, form=form)
        assert at100["depth"].tolist() == [[2, 2], [1, 0], [1, 0]]


def _random_case(seed, n_pairs=50):
    rng = random.Random(seed)
    anc = bytes(rng.choice(b"ACGT") for _ in range(400))
    queries, records = [], []
    for _ in range(6):
        at, m = rng.randrange(0, 300), rng.choice([7, 8, 9, 31, 32, 33, 64, 65, 90])
        q = bytearray(anc[at:at + m])
        if rng.random() < 0.3:
            q[rng.randrange(m)] = ord("N")
        queries.append(bytes(q))
    queries.append(b"")
    for _ in range(4):
        r = bytearray(anc)
        for _ in range(rng.randrange(5, 40)):
            x, kind = rng.randrange(len(r)), rng.random()
            if kind < 0.6:
                r[x] = rng.choice(b"ACGTN")
            elif kind < 0.8:
                del r[x:x + rng.choice([1, 1, 2, 3])]
            else:
                r[x:x] = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([1, 1, 2, 4])))
        records.append(bytes(r) if rng.random() < 0.5 else H.revcomp(bytes(r)))
    pairs = []
    for _ in range(n_pairs):
        rec = rng.randrange(len(records))
        pairs.append((rng.randrange(len(queries)), rng.randrange(2), rec, 0, len(records[rec]) if rng.random() < 0.9 else 0))
    groups = [rng.choice([0, 1, 2, P.LEAVE_OUT]) for _ in pairs]
    return queries, records, np.array(pairs), groups


@pytest.mark.parametrize("seed,lengths,mm,c3", [(1, (8, 20, 32), 2, 3), (9, (18, 20, 22, 25), 1, 0), (3, (9, 8, 31, 10, 11, 12, 13, 14), 7, 8)])
def test_the_two_forms_agree_and_keep_the_invariants(seed, lengths, mm, c3):
    queries, records, pairs, groups = _random_case(seed)
    al = A.alignments(queries, records, pairs)
    for permille in (1000, 200):
        one = W.windows_ops(queries, records, pairs, groups, 3, lengths, mm, c3, permille, al=al, form="loops")
        two = W.windows_ops(queries, records, pairs, groups, 3, lengths, mm, c3, permille, al=al, form="prefix")
        assert np.array_equal(one["wtable"], two["wtable"]) and np.array_equal(one["depth"], two["depth"])
        assert 0 < one["piled"].sum() < len(pairs)
        t = one["wtable"]
        assert all(t[..., c].any() for c in (MM0, MM1, GAPPED, FWD, REV)), "the random pairs reach every kind of class"
        W.invariants(t, one["depth"], one["q_offsets"], lengths)
        # the pairs that count are the pileup's: the same depths
        assert np.array_equal(one["depth"], P.pile_ops(queries, records, pairs, groups, 3, permille, al=al)["depth"])
        order = list(range(len(pairs)))
        random.Random(seed).shuffle(order)
        again = W.windows_ops(queries, records, pairs[order], [groups[x] for x in order], 3, lengths, mm, c3, permille)
        assert np.array_equal(again["wtable"], t)


@pytest.mark.parametrize("seed", [4, 5])
def test_strand_symmetry(seed):
    """A pair and the pair of the reverse-complemented query on the other strand have the same pattern, hence the same script: their
    tables mirror each other, W'[m - L - u] = W[u], with FWD_OK and REV_OK swapped."""
    queries, records, pairs, groups = _random_case(seed)
    queries = [q.replace(b"N", b"A") for q in queries]             # (the reverse complement of an invalid base is invalid too, but keep it plain)
    lengths, mm, c3 = (8, 21, 32), 2, 3
    flipped = pairs.copy()
    flipped[:, 1] ^= 1
    one = W.windows_ops(queries, records, pairs, groups, 3, lengths, mm, c3)
    two = W.windows_ops([H.revcomp(q) for q in queries], records, flipped, groups, 3, lengths, mm, c3)
    assert np.array_equal(one["ops"], two["ops"]) and np.array_equal(one["depth"], two["depth"])
    offs = one["q_offsets"]
    seen = 0
    for q in range(len(queries)):
        a, b = one["wtable"][offs[q]:offs[q + 1]], two["wtable"][offs[q]:offs[q + 1]]
        for l, L in enumerate(lengths):
            n = len(a) - L + 1
            if n <= 0:
                assert not a[:, l].any() and not b[:, l].any()
                continue
            mirrored = b[:n, l][::-1]
            assert np.array_equal(a[:n, l, :, :6], mirrored[:, :, :6]), (q, L)
            assert np.array_equal(a[:n, l, :, FWD], mirrored[:, :, REV]) and np.array_equal(a[:n, l, :, REV], mirrored[:, :, FWD]), (q, L)
            seen += int((a[:n, l, :, FWD] != a[:n, l, :, REV]).sum())
    assert seen > 0, "somewhere the two orientations differ"


def test_readers():
    # query 0 = ACGTACGTAC (10 bases: three windows of 8, one of 10), query 1 has an N, query 2 is empty; groups: 0 targets, 1 non-targets
    queries = [b"ACGTACGTAC", b"", "ACGTNCGTAC"]
    offs = np.array([0, 10, 10, 20], np.uint64)
    lengths = (8, 10)
    tab = np.zeros((20, 2, 2, 8), np.uint32)
    depth = np.array([[20, 10], [0, 0], [4, 0]], np.uint32)
    tab[0, 0, 0, [MM0, FWD, REV]] = 20                          # window 0 of 8: every target perfect ...
    tab[0, 0, 1, GAPPED] = 10                                   # ... and no non-target serves: a candidate in both orientations
    tab[1, 0, 0, MM0], tab[1, 0, 0, MM1], tab[1, 0, 0, FWD], tab[1, 0, 0, REV] = 18, 2, 19, 18   # 19/20 forward, 18/20 reverse
    tab[1, 0, 1, MM2], tab[1, 0, 1, REV] = 10, 1                # non-targets: 0/10 forward, 1/10 reverse
    tab[2, 0, 0, [MM0, FWD, REV]] = 20
    tab[2, 0, 1, [MM0, FWD, REV]] = 10                          # the non-targets match as well: none
    tab[0, 1, 0, MM1], tab[0, 1, 0, FWD] = 20, 20               # the window of 10: forward only
    tab[0, 1, 1, MM4P] = 10
    tab[10, 0, 0, [MM0, FWD, REV]] = 4                          # query 2: its windows at 0 hold the N; no depth in group 1
    tab[15, 0, 0, [MM0, FWD, REV]] = 4                          # u = 5 of query 2 would not fit: the row stays out whatever it holds
    f = R.window_fraction((offs, lengths, tab), depth, FWD)
    assert f.shape == (20, 2, 2) and f[0, 0, 0] == 1 and f[1, 0, 0] == 0.95 and f[1, 0, 1] == 0 and f[3, 0, 0] == 0
    assert np.isnan(f[10, 0, 1]) and f[10, 0, 0] == 1
    assert R.window_fraction((offs, lengths, tab), depth, GAPPED)[0, 0, 1] == 1
    cand, oligos = R.candidate_oligos((offs, lengths, tab), depth, queries)
    assert [(int(c["query"]), int(c["start"]), int(c["length"]), str(c["orientation"])) for c in cand] == \
        [(0, 0, 8, "F"), (0, 0, 8, "R"), (0, 0, 10, "F"), (0, 1, 8, "F")]
    assert oligos == ["ACGTACGT", "ACGTACGT", "ACGTACGTAC", "CGTACGTA"]        # (ACGTACGT is its own reverse complement)
    assert cand["f_tar"].tolist() == [1, 1, 1, .95] and cand["f_neg"].tolist() == [0, 0, 0, 0]
    cand, oligos = R.candidate_oligos((offs, lengths, tab), depth, queries, min_tar=0.9, max_neg=0.1, orientation="reverse")
    assert [(int(c["start"]), int(c["length"])) for c in cand] == [(0, 8), (1, 8)] and oligos == ["ACGTACGT", "TACGTACG"]
    assert cand["f_tar"].tolist() == [1, .9] and cand["f_neg"].tolist() == [0, .1]
    assert len(R.candidate_oligos((offs, lengths, tab), depth, queries, orientation="forward")[0]) == 3
    # the other way round: group 1 as the targets
    assert len(R.candidate_oligos((offs, lengths, tab), depth, queries, tar=1, neg=0, min_tar=1.0, max_neg=1.0)[0]) == 2
    # no depth among the non-targets (no non-target holds the signature): f_neg reads 0 and the window stays; no depth among the
    # targets: the window goes
    lone = np.zeros((10, 2, 2, 8), np.uint32)
    lone[:3, 0, 0, [MM0, FWD, REV]] = 4
    lone[0, 1, 0, [MM0, FWD, REV]] = 4
    cand, oligos = R.candidate_oligos((offs[:2], lengths, lone), depth[2:], queries[:1], orientation="forward")
    assert [(int(c["start"]), int(c["length"])) for c in cand] == [(0, 8), (0, 10), (1, 8), (2, 8)]
    assert cand["f_tar"].tolist() == [1] * 4 and cand["f_neg"].tolist() == [0] * 4 and oligos[1] == "ACGTACGTAC"
    assert np.isnan(R.window_fraction((offs[:2], lengths, lone), depth[2:], FWD)[0, 0, 1])
    assert len(R.candidate_oligos((offs[:2], lengths, lone), depth[2:], queries[:1], tar=1, neg=0, min_tar=0.0, max_neg=1.0)[0]) == 0
    with pytest.raises(ValueError):
        R.candidate_oligos((offs, lengths, tab), depth, queries, orientation="up")
    with pytest.raises(ValueError):
        R.candidate_oligos((offs, lengths, tab), depth, queries[:2])
    with pytest.raises(ValueError):
        R.candidate_oligos((offs, lengths, tab), depth, queries, tar=2)
    with pytest.raises(ValueError):
        R.window_fraction((offs, lengths, tab), depth[:2], FWD)
    assert "off-locus" in R.candidate_oligos.__doc__ and "oligo_hits" in R.candidate_oligos.__doc__

    class WStub:
        lengths = (8, 10)

        def table(self):
            return offs, tab

    class PStub:
        def depth(self):
            return depth
    assert len(R.candidate_oligos(WStub(), PStub(), queries)[0]) == 4
    # on a restated table: the depth can also come from the pileup's own table
    qs, recs = [b"ACGTACGTAC"], [b"GGACGTACGTACGG", b"GGACGTTCGTACGG"]
    pr = np.array([(0, 0, 0, 0, 14), (0, 0, 1, 0, 14)])
    w = W.windows_ops(qs, recs, pr, [0, 1], 2, (8,), 0, 3)
    p = P.pile_ops(qs, recs, pr, [0, 1], 2)
    cand, oligos = R.candidate_oligos((w["q_offsets"], (8,), w["wtable"]), (p["q_offsets"], p["table"]), qs)
    assert oligos == ["ACGTACGT", "ACGTACGT", "CGTACGTA", "TACGTACG", "GTACGTAC", "GTACGTAC"] and cand["orientation"].tolist() == list("FRFRFR")


def test_argument_errors_are_raised_without_a_device():
    from seqwin_amd._abi import PROTOTYPES
    from seqwin_amd._core import _ptr
    from seqwin_amd._lib import c_u64, c_vp, check, lib
    from seqwin_amd.device import INFIX_PAIR_DTYPE, Batch, BestHits, _window_args
    for name in ("sw_batch_infix_windows", "sw_batch_best_hits_windows", "sw_windows_sizes", "sw_windows_lengths", "sw_windows_export", "sw_windows_stats",
                 "sw_windows_free"):
        assert name in PROTOTYPES
    offs = np.array([0, 4], np.uint64)
    pair = np.zeros(1, INFIX_PAIR_DTYPE)
    pair["stop"] = 3
    out = [np.zeros(1, np.uint32) for _ in range(6)]
    h, ph, wh = c_vp(), c_vp(), c_vp()
    lab = np.array([0], np.uint8)

    def infix(lengths, mm, c3, n_groups=2):
        lens = np.array(lengths, np.uint32)
        check(lib.sw_batch_infix_windows(None, _ptr(offs), b"ACGT", c_u64(1), _ptr(pair), c_u64(1), _ptr(lab), c_u64(n_groups), c_u64(1000),
                                         _ptr(lens) if len(lens) else None, c_u64(len(lens)), c_u64(mm), c_u64(c3), *[_ptr(x) for x in out], ctypes.byref(ph),
                                         ctypes.byref(wh), None, None))

    def hits(lengths, mm, c3, n_groups=2):
        lens = np.array(lengths, np.uint32)
        check(lib.sw_batch_best_hits_windows(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(3), c_u64(0), c_u64(1), c_u64(1), None, None, c_u64(n_groups),
                                             c_u64(1000), _ptr(lens) if len(lens) else None, c_u64(len(lens)), c_u64(mm), c_u64(c3), ctypes.byref(h),
                                             ctypes.byref(ph), ctypes.byref(wh)))

    bad = [((), 2, 3, "1..8 lengths"), (tuple(range(8, 17)), 2, 3, "1..8 lengths"), ((7,), 2, 3, "8..32"), ((20, 33), 2, 3, "8..32"),
           ((20, 18, 20), 2, 3, "twice"), ((20,), 9, 3, "max_mismatch"), ((8, 20), 8, 3, "max_mismatch"), ((20,), 1 << 40, 3, "max_mismatch"),
           ((20,), 2, 9, "three_prime")]
    for lengths, mm, c3, match in bad:
        for call in (infix, hits):
            with pytest.raises(ValueError, match=match):
                call(lengths, mm, c3)
        with pytest.raises(ValueError):
            _window_args(lengths, mm, c3)
        with pytest.raises(ValueError):
            W.check_args(lengths, mm, c3)
    for call in (infix, hits):
        with pytest.raises(ValueError, match="groups"):        # the pileup's own checks hold as before
            call((20,), 2, 3, n_groups=9)
        for lengths, mm, c3 in (((8,), 7, 8), ((32, 8, 20), 0, 0), (tuple(range(8, 16)), 7, 3), ((9,), 8, 0)):   # what is valid gets as far as the missing batch
            with pytest.raises(ValueError, match="NULL"):
                call(lengths, mm, c3)
            W.check_args(lengths, mm, c3)
    for fn in (lib.sw_windows_sizes(None, None, None, None, None, None, None), lib.sw_windows_lengths(None, None), lib.sw_windows_export(None, c_u64(0), c_u64(0), None),
               lib.sw_windows_stats(None, None, None)):
        with pytest.raises(ValueError, match="NULL"):
            check(fn)
    lib.sw_windows_free(None)
    # the Python side
    lens, mm, c3 = _window_args((18, 20, 22, 25), 2, 3)
    assert lens.dtype == np.uint32 and lens.tolist() == [18, 20, 22, 25] and (mm, c3) == (2, 3)
    with pytest.raises(ValueError):
        _window_args(20, 2, 3)
    with pytest.raises(ValueError, match="pileup"):
        Batch.best_hits(object.__new__(Batch), [b"ACGT"], 3, window_lengths=(20,))
    with pytest.raises(ValueError, match="window_lengths"):
        BestHits(None).windows()
