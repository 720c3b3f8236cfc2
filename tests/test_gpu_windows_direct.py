"""GPU: the window walk of csrc/align.hip -- Batch.infix_windows, joint mismatch classes per query window, length and group over the
canonical alignments of crafted pairs -- against the host restatement (tests/tools/windows_host.py): the whole
table, element for element.  Every call also gives the pileup and the six alignment arrays, which must be bit for bit what
Batch.infix_pileup gives on the same list.  The counts are integers added by atomics and finished by one pass, so nothing may depend
on the order of the pairs, the rounds through the scratch (SEQWIN_AMD_ALN_SCRATCH_KB), the launch split (SEQWIN_AMD_SEQ_MAX_BLOCKS) or
the route of the store pass (SEQWIN_AMD_DIST_LDS_CAP)."""
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

pytestmark = pytest.mark.gpu
WINDOWS = (8, 20, 32)                                            # the shortest, the longest and one in between
LENGTHS = sorted({L + d for L in WINDOWS for d in (-1, 0, 1)} | {63, 64, 65, 129})   # L - 1, L, L + 1 and the 64-row pattern-block bounds
MM, C3 = 2, 3
OTHER = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
N_SAME = 300                                                     # with the crafted pairs: more than one workgroup of 256 lanes in a round
WALK_LANES = 256                                                 # a workgroup of the walk: one lane per pair


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d\n" % (name.encode(), i))
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def _substituted(seq, places):
    out = bytearray(seq)
    for at in places:
        out[at:at + 1] = OTHER[out[at]]
    return bytes(out)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Records: 0 the ancestor with one N; 1 the reverse complement of a stretch between random text.  Queries: the lengths of LENGTHS
    cut from the stretch (clean copies: perfect windows); 300 bases with substitutions -- alone, two 4 apart, and 3, 4 and 5 within 7
    bases --, two insertions and three deletions, one of 2 bases; 100 bases with exactly three substitutions (dist 3: on the bound at
    30 permille); one over the text's N; one with an invalid byte; an empty one.  Pairs: every query where its copy lies, on strand 0
    in record 0 and on strand 1 in record 1; empty texts; N_SAME pairs of one imperfect query on one text."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    rng = random.Random(67)
    anc = _rand(rng, 2600)
    queries = [anc[700:700 + n] for n in LENGTHS]
    long_q = bytearray(_substituted(anc[700:1000], (15, 60, 64, 100, 102, 105, 150, 151, 153, 156, 180, 200, 201, 203, 205, 206, 290)))
    two = next(x for x in range(230, 270) if anc[700 + x - 1] not in anc[700 + x:702 + x] and anc[702 + x] not in anc[700 + x:702 + x])
    for at, n in ((280, 1), (two, 2), (120, 1)):                # (from the right, so that the places to the left keep their index)
        del long_q[at:at + n]
    for at in (40, 80):
        long_q[at:at] = b"GT"
    queries.append(bytes(long_q))
    queries.append(_substituted(anc[860:960], (10, 50, 90)))
    bad = bytearray(anc[750:850])
    bad[50:51] = b"X"
    queries += [anc[1150:1250], bytes(bad), b""]
    Q_LONG, Q_BOUND, Q_N, Q_BAD, Q_EMPTY = range(len(LENGTHS), len(LENGTHS) + 5)
    rec0 = bytearray(anc)
    rec0[1200:1201] = b"N"
    rec1 = _rand(rng, 120) + H.revcomp(anc[650:1050]) + _rand(rng, 90)
    records = [bytes(rec0), rec1]
    b = Batch.from_fasta([_write(tmp_path_factory.mktemp("win"), "a0.fa", records)], n_cpu=2)
    pairs = []
    for q in list(range(len(LENGTHS))) + [Q_LONG, Q_BOUND, Q_BAD, Q_EMPTY]:
        pairs += [(q, 0, 0, 600, 1100), (q, 1, 1, 0, len(rec1))]
    q129, q33 = LENGTHS.index(129), LENGTHS.index(33)
    pairs += [(Q_N, 0, 0, 1100, 1300), (q33, 0, 0, 10, 10), (q129, 1, 1, 7, 7), (Q_BAD, 0, 0, 10, 10),
              (q129, 0, 0, 710, 1000),                                      # the window starts inside the copy: j == 0 with i > 0
              (Q_LONG, 0, 0, 700, 1000), (Q_LONG, 1, 1, 100, 500)]
    pairs += [(Q_BOUND, 0, 0, 600, 1100)] * N_SAME
    pairs = np.array(pairs, np.int64)
    groups = np.arange(len(pairs)) % 3
    groups[::11] = P.LEAVE_OUT
    groups[len(pairs) - N_SAME:] = np.arange(N_SAME) % 2                    # several waves adding to the same counters of two groups
    al = A.alignments(queries, records, pairs)
    want = W.windows_ops(queries, records, pairs, groups, 3, WINDOWS, MM, C3, al=al)
    yield dict(b=b, queries=queries, records=records, pairs=pairs, groups=groups, al=al, want=want, q_long=Q_LONG, q_bound=Q_BOUND)
    b.close()


def _check(case, order=None, groups=None, n_groups=3, permille=1000, lengths=WINDOWS, mm=MM, c3=C3, want=None):
    idx = np.arange(len(case["pairs"])) if order is None else np.asarray(order)
    groups = case["groups"] if groups is None else np.asarray(groups)
    want = case["want"] if want is None else want
    b, queries = case["b"], case["queries"]
    win, pile, arrays, al_st = b.infix_windows(queries, case["pairs"][idx], groups[idx], lengths, n_groups=n_groups, max_dist_permille=permille, max_mismatch=mm,
                                               three_prime=c3, stats=True)
    pile0, arrays0 = b.infix_pileup(queries, case["pairs"][idx], groups[idx], n_groups=n_groups, max_dist_permille=permille)
    try:
        # the pileup and the six arrays: bit for bit those of the call without windows
        for name, arr, arr0 in zip(A.FIELDS, arrays, arrays0):
            assert arr.dtype == np.uint32 and np.array_equal(arr, arr0) and np.array_equal(arr, case["al"][name][idx]), name
        assert np.array_equal(pile.table()[1], pile0.table()[1]) and np.array_equal(pile.depth(), pile0.depth())
        assert np.array_equal(pile.depth(), want["depth"])
        s, s0 = pile.stats(), pile0.stats()
        assert all(s[k] == s0[k] for k in ("piled", "filtered_by_distance", "left_out_by_label", "adds", "table_bytes"))
        # the windows
        assert win.sizes() == (len(queries), int(want["q_offsets"][-1]), n_groups, len(lengths), mm, c3) and win.lengths == tuple(lengths)
        offs, table = win.table()
        assert table.dtype == np.uint32 and table.shape == want["wtable"].shape and np.array_equal(offs.astype(np.int64), want["q_offsets"])
        bad = np.argwhere(table != want["wtable"])
        assert not len(bad), (bad[:5].tolist(), table[tuple(bad[0])], want["wtable"][tuple(bad[0])])
        q = case["q_long"]
        assert np.array_equal(win.counts(q), want["wtable"][want["q_offsets"][q]:want["q_offsets"][q + 1]])
        W.invariants(table, pile.depth(), offs, lengths)
        st = win.stats()
        assert st["table_bytes"] == table.nbytes
        # the walk visits every window of every piled pair, and adds only for the imperfect ones: once to its class, and to 6 / 7
        m = np.diff(want["q_offsets"])
        per_query = sum(np.maximum(m - L + 1, 0) for L in lengths)
        assert st["windows"] == int((pile.depth().sum(axis=1) * per_query).sum())
        perfect = int(table[..., W.MM0].sum())
        assert st["adds"] == int(table[..., 1:6].sum()) + int(table[..., 6:].sum()) - 2 * perfect
        assert al_st["pairs"] == len(idx) and al_st["rounds"] >= 1
        return table, st, al_st
    finally:
        for x in (win, pile, pile0):
            x.close()


def test_the_crafted_pairs_cover_their_bounds(case):
    """On the host: what this file is about occurs among the pairs, and the literal form of the restatement agrees."""
    al, pairs, want = case["al"], case["pairs"], case["want"]
    m = np.array([len(case["queries"][q]) for q in pairs[:, 0]])
    assert set(LENGTHS) | {0, 100} <= set(m.tolist()) and (m > 290).any() and {7, 8, 9, 19, 20, 21, 31, 32, 33} <= set(LENGTHS)
    o = al["offsets"].astype(np.int64)
    scripts = ["".join(A.OPS[c] for c in al["ops"][o[x]:o[x + 1]]) for x in range(len(pairs))]
    longs = [s for x, s in enumerate(scripts) if pairs[x, 0] == case["q_long"]]
    assert all("DD" in s and s.count("I") >= 3 and s.count("X") >= 16 for s in longs) and {int(p[1]) for p in pairs if p[0] == case["q_long"]} == {0, 1}
    assert any(s and set(s) == {"I"} for s in scripts) and any(s == "" for s in scripts)
    assert any(s.startswith("I") and "=" in s for s in scripts)             # the walk reaches j == 0 with i > 0
    t = want["wtable"]
    assert all(t[..., c].any() for c in range(8)) and t.max() >= N_SAME // 2
    # a window of the long query slides over every gap and substitution: a run of D at its slots u, u + 1, u + L - 1 and u + L, an I at
    # its first and last position, an X at distance c and c + 1 from either end, and e = max_mismatch, one above, 3, 4 and 5 all occur
    x, ins, b = W.script_arrays(al["ops"][o[len(LENGTHS) * 2]:o[len(LENGTHS) * 2 + 1]], int(m[len(LENGTHS) * 2]))
    assert pairs[len(LENGTHS) * 2, 0] == case["q_long"] and pairs[len(LENGTHS) * 2, 1] == 0
    L = 20
    cx = np.concatenate(([0], np.cumsum(x)))
    e = cx[L:] - cx[:-L]
    clean = np.array([not ins[s:s + L].any() and not b[s + 1:s + L].any() for s in range(len(x) - L + 1)])
    assert {MM, MM + 1, 3, 4, 5} <= set(e[clean].tolist())
    d = int(np.flatnonzero(b)[0])
    assert all(0 <= d - k <= len(x) - L for k in (0, 1, L - 1, L)) and clean[d] and clean[d - L] and not clean[d - 1] and not clean[d - L + 1]
    i0, i1 = int(np.flatnonzero(ins)[0]), int(np.flatnonzero(ins)[-1])
    assert not clean[i0] and not clean[i1 - L + 1] and clean[i1 + 1] and clean[i0 - L]
    # a lone X: the windows that hold it at distance c - 1 and c from either end
    one = next(int(p) for p in np.flatnonzero(x) if L <= p <= len(x) - L and cx[p + L] - cx[p - L + 1] == 1)
    assert all(e[s] == 1 and clean[s] for s in (one - C3 + 1, one - C3, one - L + C3, one - L + C3 + 1))
    short = np.flatnonzero(m <= 129)[:-N_SAME + 3]
    loops = W.windows_ops(case["queries"], case["records"], pairs[short], case["groups"][short], 3, WINDOWS, MM, C3, form="loops")
    again = W.windows_ops(case["queries"], case["records"], pairs[short], case["groups"][short], 3, WINDOWS, MM, C3, form="prefix")
    assert np.array_equal(loops["wtable"], again["wtable"]) and loops["wtable"].any()


def test_crafted_pairs(case):
    _check(case)


def test_shuffled_order(case):
    order = list(range(len(case["pairs"])))
    random.Random(5).shuffle(order)
    _check(case, order)
    _check(case, order[::-1])


@pytest.mark.parametrize("env", [{"SEQWIN_AMD_ALN_SCRATCH_KB": "16"}, {"SEQWIN_AMD_SEQ_MAX_BLOCKS": "1"}, {"SEQWIN_AMD_DIST_LDS_CAP": "1"},
                                 {"SEQWIN_AMD_ALN_SCRATCH_KB": "16", "SEQWIN_AMD_SEQ_MAX_BLOCKS": "1", "SEQWIN_AMD_DIST_LDS_CAP": "1"}])
def test_rounds_launch_split_and_striped_route(case, monkeypatch, env):
    """A lowered scratch gives several rounds.  Without it the list is one round of more than WALK_LANES pairs, which a launch bound of
    one workgroup splits into a walk launch from the round's start and one from a later pair (x0 > p0)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, _, al_st = _check(case)
    assert len(case["pairs"]) > WALK_LANES
    if "SEQWIN_AMD_ALN_SCRATCH_KB" in env:
        assert al_st["rounds"] > 2 and al_st["scratch_peak_bytes"] <= max(16 << 10, al_st["largest_pair_bytes"])
    else:
        assert al_st["rounds"] == 1
    assert (al_st["striped_pairs"] > 0) == ("SEQWIN_AMD_DIST_LDS_CAP" in env)


@pytest.mark.parametrize("lengths,mm,c3,n_groups", [((20,), 2, 0, 1), ((32, 8), 7, 8, 8), ((18, 20, 22, 25), 3, 1, 2), (tuple(range(9, 17)), 0, 3, 3)])
def test_other_lengths_bounds_tails_and_groups(case, lengths, mm, c3, n_groups):
    """three_prime 0 and 8, max_mismatch 0 and the largest, one and eight lengths (in an order that is not ascending), one and eight
    groups."""
    groups = np.arange(len(case["pairs"])) % n_groups
    groups[::7] = P.LEAVE_OUT
    want = W.windows_ops(case["queries"], case["records"], case["pairs"], groups, n_groups, lengths, mm, c3, al=case["al"])
    _check(case, groups=groups, n_groups=n_groups, lengths=lengths, mm=mm, c3=c3, want=want)


def test_a_pair_on_the_bound(case):
    """The query with exactly three substitutions in 100 bases: dist * 1000 == 30 * m.  A pair removed by the bound adds nothing."""
    x = np.flatnonzero((case["pairs"][:, 0] == case["q_bound"]) & (case["pairs"][:, 4] - case["pairs"][:, 3] > 0))
    assert len(x) == 2 + N_SAME and set(case["al"]["dist"][x].tolist()) == {3}
    depth = {}
    for permille in (30, 29):
        want = W.windows_ops(case["queries"], case["records"], case["pairs"], case["groups"], 3, WINDOWS, MM, C3, permille, al=case["al"])
        depth[permille] = int(want["depth"][case["q_bound"]].sum())
        _check(case, permille=permille, want=want)
    assert depth[30] > N_SAME // 2 and depth[29] == 0


def test_malformed_calls_raise(case):
    b, queries, pairs, groups = case["b"], case["queries"], case["pairs"], case["groups"]
    for lengths, mm, c3 in (((7,), 2, 3), ((20, 20), 2, 3), ((), 2, 3), ((20,), 9, 3), ((8,), 8, 3), ((20,), 2, 9)):
        with pytest.raises(ValueError):
            b.infix_windows(queries, pairs[:4], groups[:4] % 3, lengths, n_groups=3, max_mismatch=mm, three_prime=c3)
    with pytest.raises(ValueError, match="group label"):
        b.infix_windows(queries, pairs[:4], [0, 1, 3, 0], (20,), n_groups=3)
    win, pile, arrays = b.infix_windows(queries, np.zeros((0, 5), np.int64), [], (20, 8), n_groups=2)
    try:
        assert all(a.shape == (0,) for a in arrays) and not win.table()[1].any() and win.table()[1].shape[1:] == (2, 2, 8)
        assert win.stats()["windows"] == 0 and win.stats()["adds"] == 0
        with pytest.raises(ValueError):
            win.counts(len(queries))
    finally:
        win.close()
        pile.close()
