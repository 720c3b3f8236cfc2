"""GPU: the pile walk of csrc/align.hip -- Batch.infix_pileup, base counts per query position and group over the canonical alignments
of crafted pairs -- against the host restatement (tests/tools/pileup_host.py): the whole table, the depths and
the six alignment arrays, element for element.  The counts are integers added by atomics, so nothing may depend on the order of the
pairs, the rounds through the scratch (SEQWIN_AMD_ALN_SCRATCH_KB), the launch split (SEQWIN_AMD_SEQ_MAX_BLOCKS) or the route of the
store pass (SEQWIN_AMD_DIST_LDS_CAP)."""
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

pytestmark = pytest.mark.gpu
LENGTHS = [1, 63, 64, 65, 129]
OTHER = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
N_SAME = 300


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
    """Records: 0 the ancestor with one N and a run of 12 N; 1 the reverse complement of a stretch between random text.  Queries: the
    lengths of LENGTHS cut from the stretch; 300 bases of it with four substitutions, three 2-base insertions and three deletions;
    100 bases with exactly three substitutions (dist 3: on the bound at 30 permille); one over the single N, one across the run of
    N; one with an invalid byte; an empty one.  Pairs: every query where its copy lies, on strand 0 in record 0 and on strand 1 in
    record 1; an empty text; a copy cut by the window's start; N_SAME pairs of one query on one text."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    rng = random.Random(61)
    anc = _rand(rng, 2600)
    queries = [anc[700:700 + n] for n in LENGTHS]
    long_q = bytearray(_substituted(anc[700:1000], (15, 77, 140, 290)))
    # (scripts with `D`, one a run of two: where neither neighbour equals a base of the pair it loses, so that no match splits the run)
    two = next(x for x in range(90, 130) if anc[700 + x - 1] not in anc[700 + x:702 + x] and anc[702 + x] not in anc[700 + x:702 + x])
    for at, n in ((250, 1), (170, 1), (two, 2)):
        del long_q[at:at + n]
    for at in (40, 120, 200):
        long_q[at:at] = b"GT"
    queries.append(bytes(long_q))
    queries.append(_substituted(anc[860:960], (10, 50, 90)))
    bad = bytearray(anc[750:850])
    bad[50:51] = b"X"
    queries += [anc[1150:1250], anc[1450:1560], bytes(bad), b""]
    Q_LONG, Q_BOUND, Q_N, Q_RUN, Q_BAD, Q_EMPTY = range(len(LENGTHS), len(LENGTHS) + 6)
    rec0 = bytearray(anc)
    rec0[1200:1201] = b"N"
    rec0[1500:1512] = b"N" * 12
    rec1 = _rand(rng, 120) + H.revcomp(anc[650:1050]) + _rand(rng, 90)
    records = [bytes(rec0), rec1]
    b = Batch.from_fasta([_write(tmp_path_factory.mktemp("pile"), "a0.fa", records)], n_cpu=2)
    pairs = []
    for q in list(range(len(LENGTHS))) + [Q_LONG, Q_BOUND, Q_BAD, Q_EMPTY]:
        pairs += [(q, 0, 0, 600, 1100), (q, 1, 1, 0, len(rec1)), (q, 0, 0, 10, 10), (q, 1, 1, 7, 7)]
    q129, q65 = LENGTHS.index(129), LENGTHS.index(65)
    pairs += [(Q_N, 0, 0, 1100, 1300), (Q_RUN, 0, 0, 1400, 1600), (Q_RUN, 0, 0, 1450, 1560),
              (q129, 0, 0, 710, 1000),                                      # the window starts inside the copy: j == 0 with i > 0
              (q129, 1, 1, 0, 120 + 400 - 60),                              # the same on strand 1: the window ends inside the copy
              (Q_LONG, 0, 0, 700, 1000), (Q_LONG, 0, 0, 720, 990)]
    pairs += [(q65, 0, 0, 600, 1100)] * N_SAME
    pairs = np.array(pairs, np.int64)
    groups = np.arange(len(pairs)) % 3
    groups[::11] = P.LEAVE_OUT
    groups[len(pairs) - N_SAME:] = np.arange(N_SAME) % 2                    # several waves adding to the same counters of two groups
    al = A.alignments(queries, records, pairs)
    want = P.pile_ops(queries, records, pairs, groups, 3, al=al)
    yield dict(b=b, queries=queries, records=records, pairs=pairs, groups=groups, al=al, want=want, q_bound=Q_BOUND)
    b.close()


def _check(case, order=None, groups=None, n_groups=3, permille=1000, want=None):
    idx = np.arange(len(case["pairs"])) if order is None else np.asarray(order)
    groups = case["groups"] if groups is None else np.asarray(groups)
    want = case["want"] if want is None else want
    pile, arrays = case["b"].infix_pileup(case["queries"], case["pairs"][idx], groups[idx], n_groups=n_groups, max_dist_permille=permille)
    try:
        assert pile.sizes() == (len(case["queries"]), int(want["q_offsets"][-1]), n_groups)
        for name, arr in zip(A.FIELDS, arrays):
            assert arr.dtype == np.uint32 and np.array_equal(arr, case["al"][name][idx]), name
        offs, table = pile.table()
        assert table.dtype == np.uint32 and np.array_equal(offs.astype(np.int64), want["q_offsets"])
        bad = np.argwhere(table != want["table"])
        assert not len(bad), (bad[:5].tolist(), table[tuple(bad[0])], want["table"][tuple(bad[0])])
        assert np.array_equal(pile.depth(), want["depth"])
        q = len(LENGTHS)
        assert np.array_equal(pile.counts(q), want["table"][want["q_offsets"][q]:want["q_offsets"][q + 1]])
        st = pile.stats()
        assert st["piled"] + st["filtered_by_distance"] + st["left_out_by_label"] == len(idx)
        assert st["left_out_by_label"] == int((groups == P.LEAVE_OUT).sum()) and st["piled"] == int(want["depth"].sum())
        assert st["adds"] == int(table[:, :, :6].sum()) + 2 * int(table[:, :, P.INS].sum()) and st["table_bytes"] == table.nbytes
        return table, st
    finally:
        pile.close()


def test_the_crafted_pairs_cover_their_bounds(case):
    """On the host: what this file is about occurs among the pairs, and the literal form agrees on the short ones."""
    al, pairs, want = case["al"], case["pairs"], case["want"]
    m = np.array([len(case["queries"][q]) for q in pairs[:, 0]])
    assert set(LENGTHS) | {0, 100} <= set(m.tolist()) and (m > 300).any()
    o = al["offsets"].astype(np.int64)
    scripts = [al["ops"][o[x]:o[x + 1]] for x in range(len(pairs))]
    runs = ["".join(A.OPS[c] for c in s) for s in scripts[:-N_SAME]]
    assert sum("DD" in r for r in runs) >= 3 and sum("II" in r and "D" in r for r in runs) >= 3
    assert any(r.startswith("I") and "=" in r for r in runs)                # the walk reaches j == 0 with i > 0
    assert any(r and set(r) == {"I"} for r in runs) and any(r == "" for r in runs)
    t = want["table"]
    assert t[:, :, P.N_].sum() >= 13 and t[:, :, P.DEL].any() and t[:, :, P.INS_BASES].sum() > t[:, :, P.INS].sum() > 0
    assert t.max() >= N_SAME // 2 and (want["depth"] > 0).sum() >= 20
    short = np.flatnonzero(m <= 129)[:-N_SAME + 3]
    lit = P.pile_literal(case["queries"], case["records"], pairs[short], case["groups"][short], 3)
    again = P.pile_ops(case["queries"], case["records"], pairs[short], case["groups"][short], 3)
    assert np.array_equal(lit["table"], again["table"]) and np.array_equal(lit["depth"], again["depth"])


def test_crafted_pairs(case):
    _check(case)


def test_invariants_against_the_alignments_of_the_device(case):
    b, pairs, groups = case["b"], case["pairs"], case["groups"]
    table, st = _check(case)
    res = b.infix_alignments(case["queries"], pairs, ops=True)
    k = groups != P.LEAVE_OUT
    o = res[6].astype(np.int64)
    n_i = sum(int((res[7][o[x]:o[x + 1]] == 2).sum()) for x in np.flatnonzero(k))
    n_d = sum(int((res[7][o[x]:o[x + 1]] == 3).sum()) for x in np.flatnonzero(k))
    P.invariants(table, case["want"]["depth"], case["want"]["q_offsets"], res[3][k].sum(), res[4][k].sum(), n_i, n_d)   # (_check compared the depths)
    assert n_i + n_d == int(res[5][k].sum())


def test_shuffled_order(case):
    order = list(range(len(case["pairs"])))
    random.Random(5).shuffle(order)
    _check(case, order)
    _check(case, order[::-1])


@pytest.mark.parametrize("env", [{"SEQWIN_AMD_ALN_SCRATCH_KB": "16"}, {"SEQWIN_AMD_SEQ_MAX_BLOCKS": "1"}, {"SEQWIN_AMD_DIST_LDS_CAP": "1"},
                                 {"SEQWIN_AMD_ALN_SCRATCH_KB": "16", "SEQWIN_AMD_SEQ_MAX_BLOCKS": "1", "SEQWIN_AMD_DIST_LDS_CAP": "1"}])
def test_rounds_launch_split_and_striped_route(case, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check(case)


@pytest.mark.parametrize("n_groups", [1, 8])
def test_one_and_eight_groups(case, n_groups):
    groups = np.arange(len(case["pairs"])) % n_groups
    groups[::7] = P.LEAVE_OUT
    want = P.pile_ops(case["queries"], case["records"], case["pairs"], groups, n_groups, al=case["al"])
    _check(case, groups=groups, n_groups=n_groups, want=want)


def test_a_pair_on_the_bound(case):
    """The query with exactly three substitutions in 100 bases: dist * 1000 == 30 * m."""
    x = np.flatnonzero((case["pairs"][:, 0] == case["q_bound"]) & (case["pairs"][:, 4] - case["pairs"][:, 3] > 0))
    assert len(x) == 2 and case["al"]["dist"][x].tolist() == [3, 3] and (case["groups"][x] != P.LEAVE_OUT).all()
    piled = {}
    for permille in (30, 29):
        want = P.pile_ops(case["queries"], case["records"], case["pairs"], case["groups"], 3, permille, al=case["al"])
        piled[permille] = want["piled"][x].tolist()
        _, st = _check(case, permille=permille, want=want)
        assert st["filtered_by_distance"] == int((~want["piled"] & (case["groups"] != P.LEAVE_OUT)).sum()) > 0
    assert piled == {30: [True, True], 29: [False, False]}


def test_malformed_calls_raise(case):
    b, queries, pairs, groups = case["b"], case["queries"], case["pairs"], case["groups"]
    with pytest.raises(ValueError, match="group label"):
        b.infix_pileup(queries, pairs[:4], [0, 1, 3, 0], n_groups=3)
    with pytest.raises(ValueError, match="1..8"):
        b.infix_pileup(queries, pairs[:4], [0, 1, 3, 0], n_groups=9)
    with pytest.raises(ValueError, match="0..1000"):
        b.infix_pileup(queries, pairs[:4], groups[:4], max_dist_permille=1001)
    with pytest.raises(ValueError):
        b.infix_pileup(queries, pairs[:4], groups[:3])
    with pytest.raises(ValueError):
        b.infix_pileup(queries, [(len(queries), 0, 0, 0, 10)], [0])
    pile, arrays = b.infix_pileup(queries, np.zeros((0, 5), np.int64), [], n_groups=2)
    try:
        assert all(a.shape == (0,) for a in arrays) and not pile.table()[1].any() and pile.depth().shape == (len(queries), 2)
        with pytest.raises(ValueError):
            pile.counts(len(queries))
    finally:
        pile.close()
