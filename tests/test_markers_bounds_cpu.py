"""The bound cases of the marker step (tests/tools/marker_cases.py: bounds()) without a GPU: every case reaches what its name
says, judged from the host restatement's own result (a generator that drifts fails here instead of testing nothing on the
device); the restatement equals the live reference on them where the reference is built; and the bounds the cases are built
around are still the ones csrc/markers.hip compiles."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import marker_cases as C  # noqa: E402
import markers_host as M  # noqa: E402
from test_markers_cpu import _by_reference, _reference, assert_tables_equal  # noqa: E402

BOUNDS = C.bounds()
BY = {c["name"]: c for c in BOUNDS}
RES = {}
U32 = 1 << 32

# Left out of the comparison with the live reference, each because the reference's own arithmetic refuses the value:
NOT_BY_REFERENCE = {
    "stop_wraps_kmerlen_2p32": "numpy refuses to add the Python int 2**32 + 5 to the uint32 `pos` column (OverflowError)",
}


def _args(case):
    return {k: v for k, v in case.items() if k != "name"}


def res(name):
    if name not in RES:
        RES[name] = M.markers(**_args(BY[name]))
    return RES[name]


def groups(r, n_tar):
    """The vote of one subgraph restated from its rows: [(first target row, canonical ordering, len * count)] in order of first
    appearance, and the number of distinct orderings among the T target rows."""
    tar = [t for row, t in zip(r["rows"], r["seqs"]) if row["assembly_idx"] < n_tar]
    first, count = {}, {}
    for j, t in enumerate(tar):
        key = min(t, t[::-1])
        first.setdefault(key, j)
        count[key] = count.get(key, 0) + 1
    return [(first[k], k, len(k) * count[k]) for k in sorted(first, key=first.get)], len(set(tar)), len(tar)


def first_row_of(r, order):
    return [t for t in r["seqs"]].index(tuple(C.H(x) for x in order))


def test_the_bounds_in_the_source_are_the_ones_the_cases_are_built_for():
    src = (ROOT / "seqwin_amd" / "csrc" / "markers.hip").read_text()
    got = {n: int(re.search(r"constexpr (?:int|uint32_t) %s = (\d+);" % n, src).group(1)) for n in ("MK_LOC_CAP", "MK_VOTE_CAP", "MK_WAVE", "MK_TPB")}
    assert got == {"MK_LOC_CAP": 384, "MK_VOTE_CAP": 1536, "MK_WAVE": 64, "MK_TPB": 256}
    assert (C.LOC_CAP, C.VOTE_CAP, C.WAVE, C.TPB) == (384, 1536, 64, 256)
    # the run cut and the vote walk in steps of MK_WAVE and MK_TPB
    assert re.search(r"for \(uint32_t i0 = 0; i0 < n; i0 \+= MK_WAVE\)", src) and re.search(r"for \(uint32_t j = t; j < T; j \+= MK_TPB\)", src)


def test_case_names_are_the_issue_list():
    want = [f"pair_n{n}" for n in (63, 64, 65, 127, 128, 129, 383, 384, 385, 1000)]
    want += ["run_starts_at_64", "run_ends_at_63", "run_spans_60_70", "tie_first_chunk_wins", "later_larger_run_wins", "run_over_three_chunks",
             "many_runs", "nodes_63", "nodes_64", "nodes_65", "nodes_130", "nodes_130_ragged", "three_subgraphs_mixed"]
    want += [f"vote_T{T}" for T in (255, 256, 257, 513, 1536, 1537)]
    want += ["vote_all_equal_1537", "vote_all_distinct_600", "vote_tie_same_thread", "vote_tie_across_threads", "vote_partner_far",
             "vote_partner_far_reverse_more_common", "vote_partner_far_tie", "vote_partner_far_tie_other_first", "vote_palindromes_300",
             "vote_non_targets_after_1537", "two_votes_mixed", "stop_wraps", "stop_wraps_kmerlen_2p32", "cut_at_u32_max_one_run",
             "cut_at_u32_max_two_runs", "w_at_saturation", "w_above_saturation", "high_records", "no_subgraphs", "no_occurrences",
             "node_without_occurrences"]
    assert [c["name"] for c in BOUNDS] == want
    assert not {c["name"] for c in BOUNDS} & {c["name"] for c in C.cases()}
    assert max(len(c["kmers"]) for c in BOUNDS) < 10000


@pytest.mark.parametrize("n", (63, 64, 65, 127, 128, 129, 383, 384, 385, 1000))
def test_pairs_have_the_items_of_their_name_in_one_run(n):
    case, r = BY[f"pair_n{n}"], res(f"pair_n{n}")[0]
    assert C.pair_counts(case).tolist() == [[n, n]] and case["windowsize"] == 10
    assert len(case["nodes"]) == n                       # n distinct labels
    for a in (0, 1):
        assert tuple(int(r["rows"][a][f]) for f in ("assembly_idx", "start", "stop", "n_kmers", "n_repeats")) == (a, 0, 3 * (n - 1) + 5, n, 1)
    assert r["seqs"][0] == r["seqs"][1][::-1] and len(set(r["seqs"][0])) == n
    assert int(r["rep"]["n_rep"]) == 2
    assert (n > C.LOC_CAP) == (n in (385, 1000))


@pytest.mark.parametrize("name", list(C.RUN_LAYOUTS) + ["many_runs"])
def test_run_layouts_cut_where_their_name_says(name):
    lens = C.RUN_LAYOUTS.get(name, [1] * 200)
    case, r = BY[name], res(name)[0]
    starts, pos = C.run_starts(lens), C.run_positions(lens)
    n = sum(lens)
    assert C.pair_counts(case).tolist() == [[n, n]]
    # the cut falls exactly between the runs: 2 * 3 <= 3 * 10 < 2 * 100
    kept = [i for i in range(n) if i == 0 or 2 * (pos[i] - pos[i - 1]) > 3 * case["windowsize"]]
    assert kept == starts
    want = {"run_starts_at_64": ([0, 64], 64, 70), "run_ends_at_63": ([0, 10, 64], 10, 54), "run_spans_60_70": ([0, 10, 20, 30, 40, 50, 60, 71], 60, 11),
            "tie_first_chunk_wins": ([0, 4, 44, 64, 104], 4, 40), "later_larger_run_wins": ([0, 4, 44, 64, 105], 64, 41),
            "run_over_three_chunks": ([0, 5, 155], 5, 150), "many_runs": (list(range(200)), 0, 1)}[name]
    assert starts == want[0]
    best = want[1]
    for a in (0, 1):
        row = r["rows"][a]
        assert (int(row["n_repeats"]), int(row["n_kmers"]), int(row["start"])) == (len(lens), want[2], pos[best]), (name, a)
        assert int(row["stop"]) == pos[best + want[2] - 1] + 5
    if name == "tie_first_chunk_wins":
        assert lens[1] == lens[3] == max(lens) and 4 + 40 <= 64 <= 64 + 40 <= 128   # each wholly inside one chunk
        assert (4 + 40 - 1) % 64 != (64 + 40 - 1) % 64                                # their candidates lie in two lanes
    if name == "later_larger_run_wins":
        assert lens[3] == lens[1] + 1
    if name == "run_over_three_chunks":
        assert 5 // 64 == 0 and 154 // 64 == 2 and int(r["rows"][0]["n_repeats"]) == 3
    if name == "many_runs":
        assert int(r["rep"]["flags"]) == M.SINGLE


@pytest.mark.parametrize("n", (63, 64, 65, 130))
def test_node_cases_have_one_item_per_node_and_assembly(n):
    case, r = BY[f"nodes_{n}"], res(f"nodes_{n}")[0]
    assert len(case["nodes"]) == n == int(case["sg_offsets"][1]) and C.pair_counts(case).tolist() == [[n, n, n]]
    assert np.array_equal(case["nodes"]["stop"] - case["nodes"]["start"], np.full(n, 3, np.uint64))
    assert [int(x) for x in r["rows"]["n_kmers"]] == [n] * 3 and [int(x) for x in r["rows"]["n_repeats"]] == [1] * 3
    assert len({r["seqs"][0], r["seqs"][1], r["seqs"][2], r["seqs"][0][::-1], r["seqs"][1][::-1]}) == 5
    assert (n + C.WAVE - 1) // C.WAVE == {63: 1, 64: 1, 65: 2, 130: 3}[n]   # trips of the gather loop


def test_ragged_nodes():
    case, r = BY["nodes_130_ragged"], res("nodes_130_ragged")[0]
    assert len(case["nodes"]) == 130 and C.pair_counts(case).tolist() == [[210, 130]]
    ro = case["record_offsets"]
    per = []
    for nd in case["nodes"][case["sg_nodes"].astype(np.int64)]:
        rec = case["kmers"]["record_idx"][int(nd["start"]):int(nd["stop"])]
        per.append(int(((rec >= ro[0]) & (rec < ro[1])).sum()))
    assert sorted(per) == [0] * 19 + [1] * 110 + [100]
    assert per.index(100) > 0 and 0 in per[:64] and 0 in per[64:128]   # empty lanes in more than one trip of the gather
    assert [int(x) for x in r["rows"]["n_kmers"]] == [210, 130] and [int(x) for x in r["rows"]["n_repeats"]] == [1, 1]
    assert int(r["rep"]["assembly_idx"]) == 0 and int(r["rep"]["flags"]) == M.DUP and int(r["rep"]["n_rep"]) == 1
    assert r["order"].count(C.H(C.RAGGED_HEAVY)) == 100


def test_three_subgraphs_mixed_spills_on_either_side():
    case = BY["three_subgraphs_mixed"]
    assert C.pair_counts(case).tolist() == [[400, 400], [5, 5], [390, 390]]
    assert [[int(x) for x in r["rows"]["n_kmers"]] for r in res("three_subgraphs_mixed")] == [[400, 400], [5, 5], [390, 390]]


@pytest.mark.parametrize("T", (255, 256, 257, 513, 1536, 1537))
def test_pool_votes(T):
    case, r = BY[f"vote_T{T}"], res(f"vote_T{T}")[0]
    g, distinct, n = groups(r, case["n_tar"])
    assert n == T == case["n_tar"] == len(r["rows"]) and distinct == 4 and len(g) == 3   # forward and reverse are one group
    assert max(first for first, _, _ in g) < 64                                          # every leader is an early row
    assert int(r["rep"]["n_rep"]) == max(s for _, _, s in g) // len(r["order"])
    assert (T > C.VOTE_CAP) == (T == 1537) and (T > C.TPB) == (T >= 257)


def test_all_equal_and_all_distinct():
    r = res("vote_all_equal_1537")[0]
    g, distinct, n = groups(r, 1537)
    assert (n, distinct, len(g)) == (1537, 1, 1) and int(r["rep"]["n_rep"]) == 1537 and int(r["rep"]["assembly_idx"]) == 0
    r = res("vote_all_distinct_600")[0]
    g, distinct, n = groups(r, 600)
    assert (n, distinct, len(g)) == (600, 600, 600) and {s for _, _, s in g} == {7}
    assert int(r["rep"]["assembly_idx"]) == 0 and int(r["rep"]["n_rep"]) == 1
    assert 600 > 2 * C.TPB                                                               # every thread holds two or three leaders


@pytest.mark.parametrize("name, firsts, winner", [("vote_tie_same_thread", (3, 259), 3), ("vote_tie_across_threads", (5, 300), 5)])
def test_ties_of_the_vote(name, firsts, winner):
    case, r = BY[name], res(name)[0]
    g, _, n = groups(r, case["n_tar"])
    assert n == case["n_tar"] > max(firsts)
    top = max(s for _, _, s in g)
    tied = [(first, len(k)) for first, k, s in g if s == top]
    assert top == 12 and tied == [(firsts[0], 4 if name == "vote_tie_across_threads" else 6), (firsts[1], 6 if name == "vote_tie_across_threads" else 4)]
    assert sorted(s for _, _, s in g)[-3] == 7                                           # every other group scores less
    if name == "vote_tie_same_thread":
        assert firsts[0] % C.TPB == firsts[1] % C.TPB == 3
    else:
        assert (firsts[0] % C.TPB, firsts[1] % C.TPB) == (5, 44)
    assert int(r["rep"]["assembly_idx"]) == winner and int(r["rep"]["n_rep"]) == (2 if len(r["order"]) == 6 else 3)


def test_partner_far():
    P, Q = C.PARTNER, C.PARTNER[::-1]
    canon = min(P, Q, key=lambda o: tuple(map(C.H, o)))
    for name, rep_row, n_rep in (("vote_partner_far", 2, 3), ("vote_partner_far_reverse_more_common", 400, 3), ("vote_partner_far_tie", 2, 2),
                                 ("vote_partner_far_tie_other_first", 400, 2)):
        case, r = BY[name], res(name)[0]
        g, distinct, n = groups(r, case["n_tar"])
        assert n == 402 and max(s for _, _, s in g) == 6 * n_rep == [s for first, _, s in g if first == 2][0]
        assert sorted(s for _, _, s in g)[-2] == 7
        first_p = min(first_row_of(r, P), first_row_of(r, Q))
        first_q = max(first_row_of(r, P), first_row_of(r, Q))
        assert (first_p, first_q) == (2, 400) and first_q >= C.TPB
        assert int(r["rep"]["assembly_idx"]) == rep_row and int(r["rep"]["n_rep"]) == n_rep, name
        if "tie" in name:
            assert r["order"] == tuple(C.H(x) for x in canon)


def test_palindromes():
    r = res("vote_palindromes_300")[0]
    g, distinct, n = groups(r, 300)
    assert n == 300 > C.TPB and distinct == 6 and len(g) == 5
    pal = [j for j, t in enumerate(r["seqs"]) if t == t[::-1]]
    assert len(pal) > 150 and sum(j >= C.TPB for j in pal) > 20 and len(pal) < 300


def test_non_targets_vote_nothing():
    case, r = BY["vote_non_targets_after_1537"], res("vote_non_targets_after_1537")[0]
    assert len(r["rows"]) == 1587 and case["n_tar"] == 1537
    g, _, n = groups(r, 1537)
    assert n == 1537 and sorted(s for _, _, s in g) == [3 * 757, 3 * 780]
    g_all, _, _ = groups(r, 1587)
    assert sorted(s for _, _, s in g_all) == [3 * 780, 3 * 807]
    assert r["order"] == tuple(C.H(x) for x in (0, 1, 2)) and int(r["rep"]["n_rep"]) == 780
    everyone = M.markers(**{**_args(case), "n_tar": 1587})[0]
    assert everyone["order"] == tuple(C.H(x + 0) for x in (3, 4, 5)) and int(everyone["rep"]["n_rep"]) == 807


def test_two_votes_mixed():
    case, rs = BY["two_votes_mixed"], res("two_votes_mixed")
    assert [len(r["rows"]) for r in rs] == [1600, 4, 1540] and case["n_tar"] == 1600
    assert [len(r["rows"]) > C.VOTE_CAP for r in rs] == [True, False, True]


def test_32_bit_edges():
    for name in ("stop_wraps", "stop_wraps_kmerlen_2p32"):
        row = res(name)[0]["rows"][0]
        assert (int(row["start"]), int(row["stop"]), int(row["n_kmers"]), int(row["n_repeats"])) == (U32 - 13, 2, 3, 1)
    assert BY["stop_wraps"]["kmerlen"] == 5 and BY["stop_wraps_kmerlen_2p32"]["kmerlen"] == U32 + 5
    for name, w, n_runs in (("cut_at_u32_max_one_run", 2863311530, 1), ("cut_at_u32_max_two_runs", 2863311529, 2), ("w_at_saturation", 1 << 34, 1),
                            ("w_above_saturation", (1 << 34) + 1, 1)):
        case, row = BY[name], res(name)[0]["rows"][0]
        assert case["windowsize"] == w and sorted(int(x) for x in case["kmers"]["pos"]) == [0, U32 - 1]
        assert (int(row["n_repeats"]), int(row["n_kmers"]), int(row["start"])) == (n_runs, 3 - n_runs, 0)
        assert int(row["stop"]) == (4 if n_runs == 1 else 5)
    assert 3 * 2863311530 == 2 * (U32 - 1)
    case, r = BY["high_records"], res("high_records")[0]
    assert [int(x) for x in case["record_offsets"]] == [0, 1, 1 << 31, (1 << 31) + 1, U32 - 1]
    assert sorted({int(x) for x in case["kmers"]["record_idx"]}) == [0, 1 << 31, U32 - 2]
    assert C.pair_counts(case).tolist() == [[2, 0, 2, 2]]
    assert [tuple(int(row[f]) for f in ("assembly_idx", "record_idx", "start", "stop", "n_kmers", "n_repeats")) for row in r["rows"]] == \
        [(0, 0, 7, 17, 2, 1), (2, 0, 12, 22, 2, 1), (3, (1 << 31) - 3, 17, 27, 2, 1)]


def test_empty_shapes():
    assert res("no_subgraphs") == [] and len(BY["no_subgraphs"]["kmers"]) == 6 and BY["no_subgraphs"]["sg_offsets"].tolist() == [0]
    case = BY["no_occurrences"]
    assert res("no_occurrences") == [] and len(case["kmers"]) == 0 and len(case["nodes"]) == 3
    assert np.array_equal(case["nodes"]["start"], case["nodes"]["stop"])
    case, r = BY["node_without_occurrences"], res("node_without_occurrences")[0]
    assert (case["nodes"]["stop"] - case["nodes"]["start"]).tolist() == [2, 0, 2] and len(case["kmers"]) == 4
    assert int(case["nodes"]["stop"][-1]) == 4 and case["sg_nodes"].tolist() == [0, 1, 2]
    assert [int(x) for x in r["rows"]["n_kmers"]] == [2, 2] and C.pair_counts(case).tolist() == [[2, 2]]
    t = M.tables(res("no_subgraphs"))
    assert [len(t[k]) for k in ("reps", "rep_offsets", "rep_hashes", "row_offsets", "rows", "kmer_offsets", "row_hashes")] == [0, 1, 0, 1, 0, 1, 0]


def test_sweep_seeds_are_fixed_and_every_subgraph_has_a_target_row():
    assert len(C.SWEEP_SEEDS) == len(set(C.SWEEP_SEEDS)) == 40
    shapes = set()
    for seed in C.SWEEP_SEEDS:
        case = C.sweep(seed)
        cnt = C.pair_counts(case)
        assert (cnt[:, :case["n_tar"]].sum(axis=1) > 0).all(), seed
        assert 1 <= len(cnt) <= 4 and 1 <= cnt.shape[1] <= 300 and len(case["kmers"]) < 10000
        shapes.add((len(cnt), cnt.shape[1]))
        assert np.diff(case["sg_offsets"].astype(np.int64)).max() <= 150
    assert len(shapes) >= 35
    biggest = max(int(C.pair_counts(C.sweep(seed)).max()) for seed in C.SWEEP_SEEDS)
    assert biggest > C.WAVE                                                              # some pair needs a second chunk


@pytest.mark.parametrize("ci", range(len(BOUNDS)), ids=[c["name"] for c in BOUNDS])
def test_restatement_equals_the_live_reference_on_the_bound_cases(ci):
    ref = _reference()
    if ref is None:
        pytest.skip("the reference tree is not present")
    case = BOUNDS[ci]
    if case["name"] in NOT_BY_REFERENCE:
        with pytest.raises(OverflowError):   # (reasons above; the list goes stale loudly if the reference starts to accept the value)
            _by_reference(ref, case)
        return
    assert_tables_equal(M.tables(res(case["name"])), M.tables(_by_reference(ref, case)))
