"""CPU: the pileup's specification in its two host restatements (tests/tools/pileup_host.py) -- against
each other, against tables written out by hand and against the invariants --, the readers of seqwin_amd/pileup.py on those tables,
and the ValueErrors a call raises before a device is touched.  The device side is compared with the same restatement in
tests/test_gpu_pileup_direct.py and tests/test_gpu_best_hits_pileup.py."""
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

from seqwin_amd import pileup as R  # noqa: E402

a, c, g, t, n, DEL, INS, INSB = range(8)
OPS = {ch: i for i, ch in enumerate("=XID")}


def _rows_of(pattern, ops):
    """(top, bottom) without the text: the pattern row only needs the ops."""
    it = iter(pattern)
    return "".join("-" if o == "D" else next(it) for o in ops)


def _both(m, strand, ops, pattern, text):
    """One script through both forms: (rows by the op array, rows by the gapped strings), [m, 1, 8] each."""
    by_ops, by_rows = np.zeros((m, 1, 8), np.uint32), np.zeros((m, 1, 8), np.uint32)
    P.add_script(by_ops, 0, strand, np.array([OPS[o] for o in ops], np.uint8), H._codes(text.replace("#", "N")))
    tx = iter(text)
    bottom = "".join("-" if o == "I" else next(tx) for o in ops)
    P.add_rows(by_rows, 0, strand, _rows_of(pattern, ops), bottom)
    return by_ops[:, 0], by_rows[:, 0]


def _table(m, *cells):
    out = np.zeros((m, 8), np.uint32)
    for u, cls, v in cells:
        out[u, cls] += v
    return out


# (strand, pattern, ops, text from a_start, the table by hand: (position, class, count))
HAND = {
    "one X": (0, "ACGTA", "==X==", "ACCTA", [(0, a, 1), (1, c, 1), (2, c, 1), (3, t, 1), (4, a, 1)]),
    "one I": (0, "ACGTA", "==I==", "ACTA", [(0, a, 1), (1, c, 1), (2, DEL, 1), (3, t, 1), (4, a, 1)]),
    "a D run of 2": (0, "ACGTA", "==DD===", "ACTTGTA", [(0, a, 1), (1, c, 1), (2, INS, 1), (2, INSB, 2), (2, g, 1), (3, t, 1), (4, a, 1)]),
    "I then D": (0, "ACGTA", "==ID==", "ACTTA", [(0, a, 1), (1, c, 1), (2, DEL, 1), (3, INS, 1), (3, INSB, 1), (3, t, 1), (4, a, 1)]),
    "D then I": (0, "ACGTA", "==DI==", "ACTTA", [(0, a, 1), (1, c, 1), (2, INS, 1), (2, INSB, 1), (2, DEL, 1), (3, t, 1), (4, a, 1)]),
    # strand 1: the pattern ACGTA is the reverse complement of the query TACGT; pattern index i' is query position 4 - i', bases complemented
    "one X, strand 1": (1, "ACGTA", "==X==", "ACCTA", [(4, t, 1), (3, g, 1), (2, g, 1), (1, a, 1), (0, t, 1)]),
    "a D run of 2, strand 1": (1, "ACGTA", "==DD===", "ACTTGTA", [(4, t, 1), (3, g, 1), (3, INS, 1), (3, INSB, 2), (2, c, 1), (1, a, 1), (0, t, 1)]),
    "I then D, strand 1": (1, "ACGTA", "==ID==", "ACTTA", [(4, t, 1), (3, g, 1), (2, DEL, 1), (2, INS, 1), (2, INSB, 1), (1, a, 1), (0, t, 1)]),
    "a text N": (0, "ACGTA", "==X==", "AC#TA", [(0, a, 1), (1, c, 1), (2, n, 1), (3, t, 1), (4, a, 1)]),
    "a text N, strand 1": (1, "ACGTA", "==X==", "AC#TA", [(4, t, 1), (3, g, 1), (2, n, 1), (1, a, 1), (0, t, 1)]),
    "an invalid query base": (0, "AC#TA", "==X==", "ACGTA", [(0, a, 1), (1, c, 1), (2, g, 1), (3, t, 1), (4, a, 1)]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_scripts(name):
    strand, pattern, ops, text, cells = HAND[name]
    want = _table(len(pattern), *cells)
    by_ops, by_rows = _both(len(pattern), strand, ops, pattern, text)
    assert np.array_equal(by_ops, want), (name, by_ops.tolist())
    assert np.array_equal(by_rows, want), (name, by_rows.tolist())


def test_a_script_neither_begins_nor_ends_with_D():
    for ops, text in (("D=====", "TACGTA"), ("=====D", "ACGTAT")):
        for strand in (0, 1):
            with pytest.raises(AssertionError):
                P.add_script(np.zeros((5, 1, 8), np.uint32), 0, strand, np.array([OPS[o] for o in ops], np.uint8), H._codes(text))
            with pytest.raises(AssertionError):
                tx = iter(text)
                P.add_rows(np.zeros((5, 1, 8), np.uint32), 0, strand, _rows_of("ACGTA", ops), "".join(next(tx) for _ in ops))


def test_hand_made_pairs_filter_and_labels():
    """Whole pairs through both forms: the scripts are section 3.2f's, the bound is met at equality and missed one below it, label
    0xFF leaves a pair out, an empty text piles m DEL, an empty query has no rows but a depth."""
    queries = [b"ACGTA", b"AACCGGTT", b""]
    records = [b"GGACCTAGG", b"TTAACCTAGGTTCC", H.revcomp(b"GGACCTAGG")]
    pairs = np.array([(0, 0, 0, 0, 9),      # ==X==, dist 1: piled iff permille * 5 >= 1000
                      (1, 0, 1, 0, 14),     # ====DD====, dist 2: piled iff permille * 8 >= 2000
                      (0, 1, 2, 0, 9),      # the same copy as pair 0 from the other strand
                      (0, 0, 0, 4, 4),      # an empty text: dist 5 = m
                      (2, 0, 0, 0, 9),      # an empty query
                      (0, 0, 0, 0, 9)])     # left out by its label
    groups = [0, 1, 1, 0, 1, P.LEAVE_OUT]
    al = A.alignments(queries, records, pairs)
    o = al["offsets"].astype(np.int64)
    scripts = ["".join(A.OPS[x] for x in al["ops"][o[i]:o[i + 1]]) for i in range(len(pairs))]
    assert scripts == ["==X==", "====DD====", "==X==", "IIIII", "", "==X=="] and al["dist"].tolist() == [1, 2, 1, 5, 0, 1]
    want = np.zeros((13, 2, 8), np.uint32)
    for u, cls in enumerate((a, c, c, t, a)):
        want[u, 0, cls] += 1
        want[u, 0, DEL] += 1
    # pair 2, strand 1: the pattern TACGT lies on the record's TAGGT, which reads ACCTA in the query's orientation
    for u, cls in enumerate((a, c, c, t, a)):
        want[u, 1, cls] += 1
    for u, cls in enumerate((a, a, c, c, g, g, t, t)):
        want[5 + u, 1, cls] += 1
    want[5 + 4, 1, INS] += 1
    want[5 + 4, 1, INSB] += 2
    for form in (P.pile_ops, P.pile_literal):
        got = form(queries, records, pairs, groups, 2)
        assert np.array_equal(got["table"], want), form.__name__
        assert got["depth"].tolist() == [[2, 1], [0, 1], [0, 1]]
    # the bound: pair 0 and pair 2 (dist 1, m 5) sit exactly on 200; pair 1 (dist 2, m 8) on 250; the empty text (dist 5, m 5) on 1000
    for permille, depth in ((1000, [[2, 1], [0, 1], [0, 1]]), (999, [[1, 1], [0, 1], [0, 1]]), (250, [[1, 1], [0, 1], [0, 1]]),
                            (249, [[1, 1], [0, 0], [0, 1]]), (200, [[1, 1], [0, 0], [0, 1]]), (199, [[0, 0], [0, 0], [0, 1]]),
                            (0, [[0, 0], [0, 0], [0, 1]])):
        for form in (P.pile_ops, P.pile_literal):
            assert form(queries, records, pairs, groups, 2, permille)["depth"].tolist() == depth, (permille, form.__name__)


def _random_case(seed, n_pairs=60):
    rng = random.Random(seed)
    anc = bytes(rng.choice(b"ACGT") for _ in range(400))
    queries, records = [], []
    for _ in range(6):
        at, m = rng.randrange(0, 300), rng.choice([1, 2, 7, 30, 64, 65, 90])
        q = bytearray(anc[at:at + m])
        if rng.random() < 0.3 and m > 3:
            q[rng.randrange(m)] = ord("N")
        queries.append(bytes(q))
    queries.append(b"")
    for _ in range(4):
        r = bytearray(anc)
        for _ in range(rng.randrange(0, 25)):
            x, kind = rng.randrange(len(r)), rng.random()
            if kind < 0.4:
                r[x] = rng.choice(b"ACGTN")
            elif kind < 0.7:
                del r[x:x + rng.choice([1, 1, 2, 3])]
            else:
                r[x:x] = bytes(rng.choice(b"ACGT") for _ in range(rng.choice([1, 1, 2, 4])))
        records.append(bytes(r) if rng.random() < 0.5 else H.revcomp(bytes(r)))
    pairs = []
    for _ in range(n_pairs):
        rec = rng.randrange(len(records))
        lo = rng.randrange(0, len(records[rec]))
        pairs.append((rng.randrange(len(queries)), rng.randrange(2), rec, lo, rng.randrange(lo, min(len(records[rec]), lo + 200) + 1)))
    groups = [rng.choice([0, 1, 2, P.LEAVE_OUT]) for _ in pairs]
    return queries, records, np.array(pairs), groups


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_two_forms_agree_and_keep_the_invariants(seed):
    queries, records, pairs, groups = _random_case(seed)
    for permille in (1000, 300):
        one = P.pile_ops(queries, records, pairs, groups, 3, permille)
        two = P.pile_literal(queries, records, pairs, groups, 3, permille)
        assert np.array_equal(one["table"], two["table"]) and np.array_equal(one["depth"], two["depth"])
        assert one["table"].any() and 0 < one["piled"].sum() < len(pairs)
        k = one["piled"]
        o = one["offsets"].astype(np.int64)
        n_i = sum(int((one["ops"][o[x]:o[x + 1]] == 2).sum()) for x in np.flatnonzero(k))
        n_d = sum(int((one["ops"][o[x]:o[x + 1]] == 3).sum()) for x in np.flatnonzero(k))
        P.invariants(one["table"], one["depth"], one["q_offsets"], one["nident"][k].sum(), one["mismatch"][k].sum(), n_i, n_d)
        assert n_i + n_d == int(one["gaps"][k].sum())
        # order independence of the definition itself
        order = list(range(len(pairs)))
        random.Random(seed).shuffle(order)
        again = P.pile_ops(queries, records, pairs[order], [groups[x] for x in order], 3, permille)
        assert np.array_equal(again["table"], one["table"]) and np.array_equal(again["depth"], one["depth"])


def test_readers():
    counts = _table(6, (0, a, 5), (0, c, 5), (1, DEL, 3), (1, g, 2), (2, n, 1), (4, t, 2), (4, INS, 9), (4, INSB, 30), (5, c, 1), (5, DEL, 1))
    assert R.consensus(counts) == "A-N.TC"
    with pytest.raises(ValueError):
        R.consensus(np.zeros((4, 2, 8)))
    queries = [b"ACg", b"", b"uNA"]
    offs = np.array([0, 3, 3, 6], np.uint64)
    tab = np.zeros((6, 2, 8), np.uint32)
    tab[0, 0, a], tab[0, 1, c] = 4, 4                     # A: all of group 0, none of group 1
    tab[1, 0, c], tab[1, 0, DEL], tab[1, 1, c] = 3, 1, 2   # C: 3/4 and 2/2
    tab[2, 0, g], tab[2, 0, INS], tab[2, 0, INSB] = 1, 7, 7   # g: 1/1; insertions are no part of the depth; group 1 has no depth
    tab[3, 0, t], tab[3, 1, a], tab[3, 1, t] = 19, 19, 1   # u reads as T: 19/19 and 1/20
    tab[4, 0, a] = 2                                      # N in the query: nan
    tab[5, 0, a], tab[5, 0, n], tab[5, 1, g] = 1, 1, 5     # A: 1/2 and 0/5
    f = R.match_fraction((offs, tab), queries)
    want = np.array([[1, 0], [.75, 1], [1, np.nan], [1, .05], [np.nan, np.nan], [.5, 0]])
    assert f.shape == (6, 2) and np.array_equal(np.isnan(f), np.isnan(want)) and np.allclose(f[~np.isnan(want)], want[~np.isnan(want)])
    assert R.diagnostic_positions((offs, tab), queries).tolist() == [0, 3]
    assert R.diagnostic_positions((offs, tab), queries, min_tar=0.5, max_neg=0.0).tolist() == [0, 5]
    assert R.diagnostic_positions((offs, tab), queries, tar=1, neg=0, min_tar=1.0, max_neg=0.75).tolist() == [1]
    with pytest.raises(ValueError):
        R.match_fraction((offs, tab), [b"ACG", b"", b"TN"])

    class Stub:
        def table(self):
            return offs, tab
    assert np.array_equal(np.isnan(R.match_fraction(Stub(), queries)), np.isnan(want))
    # on a restated pileup: the consensus of a clean copy is the query
    got = P.pile_ops([b"ACGTA"], [b"GGACGTAGG", b"GGACCTAGG"], np.array([(0, 0, 0, 0, 9), (0, 0, 1, 0, 9)]), [0, 1], 2)
    assert R.consensus(got["table"][:, 0]) == "ACGTA" and R.consensus(got["table"][:, 1]) == "ACCTA"
    assert R.diagnostic_positions((got["q_offsets"], got["table"]), [b"ACGTA"]).tolist() == [2]


def test_argument_errors_are_raised_without_a_device():
    from seqwin_amd._abi import PROTOTYPES
    from seqwin_amd._core import _ptr
    from seqwin_amd._lib import c_u64, c_vp, check, lib
    from seqwin_amd.device import INFIX_PAIR_DTYPE, BestHits, _pile_groups
    for name in ("sw_batch_infix_pileup", "sw_batch_best_hits_pileup", "sw_pileup_sizes", "sw_pileup_export", "sw_pileup_depth", "sw_pileup_stats",
                 "sw_pileup_free"):
        assert name in PROTOTYPES
    offs = np.array([0, 4], np.uint64)
    pair = np.zeros(1, INFIX_PAIR_DTYPE)
    pair["stop"] = 3
    out = [np.zeros(1, np.uint32) for _ in range(6)]
    h, ph = c_vp(), c_vp()

    def infix(label, n_groups, permille):
        lab = np.array([label], np.uint8)
        check(lib.sw_batch_infix_pileup(None, _ptr(offs), b"ACGT", c_u64(1), _ptr(pair), c_u64(1), _ptr(lab), c_u64(n_groups), c_u64(permille),
                                        *[_ptr(x) for x in out], ctypes.byref(ph), None, None))

    def hits(n_groups, permille, mode=1):
        check(lib.sw_batch_best_hits_pileup(None, _ptr(offs), b"ACGT", c_u64(1), c_u64(3), c_u64(0), c_u64(mode), c_u64(1), None, None, c_u64(n_groups),
                                            c_u64(permille), ctypes.byref(h), ctypes.byref(ph)))

    for n_groups in (0, 9, 1 << 40):
        with pytest.raises(ValueError, match="1..8"):
            infix(0, n_groups, 1000)
        with pytest.raises(ValueError, match="1..8"):
            hits(n_groups, 1000)
    with pytest.raises(ValueError, match="0..1000"):
        infix(0, 2, 1001)
    with pytest.raises(ValueError, match="0..1000"):
        hits(2, 1001)
    for label, n_groups in ((2, 2), (254, 8), (8, 8), (1, 1)):
        with pytest.raises(ValueError, match="group label"):
            infix(label, n_groups, 1000)
    with pytest.raises(ValueError, match="0..2"):
        hits(2, 1000, mode=3)
    for label in (0, 1, 255):                               # what is valid gets as far as the missing batch
        with pytest.raises(ValueError, match="NULL"):
            infix(label, 2, 1000)
    with pytest.raises(ValueError, match="NULL"):
        hits(8, 0)
    for fn in (lib.sw_pileup_sizes(None, None, None, None), lib.sw_pileup_export(None, c_u64(0), c_u64(0), None), lib.sw_pileup_depth(None, None),
               lib.sw_pileup_stats(None, None, None)):
        with pytest.raises(ValueError, match="NULL"):
            check(fn)
    lib.sw_pileup_free(None)
    # the Python side
    assert _pile_groups([0, 255, 2], 3, None, "pair")[1] == 3 and _pile_groups([255], 1, None, "pair")[1] == 1
    assert _pile_groups([], 0, None, "pair")[1] == 1 and _pile_groups([1, 0], 2, 5, "pair")[1] == 5
    for bad in ([0, 1], [0, 1, 2, 3], [[0, 1, 2]], [0, -1, 1], [0, 256, 1], [0.5, 1, 1], [True, False, True]):
        with pytest.raises(ValueError):
            _pile_groups(bad, 3, None, "assembly")
    with pytest.raises(ValueError, match="pileup"):
        BestHits(None).pileup()
    for bad in (dict(labels=[2], n_groups=2, max_dist_permille=1000), dict(labels=[0], n_groups=0, max_dist_permille=1000),
                dict(labels=[0], n_groups=9, max_dist_permille=1000), dict(labels=[0], n_groups=1, max_dist_permille=1001)):
        with pytest.raises(ValueError):
            P.check_args(**bad)
