"""Hand-made pairs of ascending lists for the MinHash pair rule, with the counts `mash dist` gives them worked out by hand
(tests/test_minhash_cpu.py checks the restatement against them, tests/test_gpu_minhash.py the device)."""

# (name, A, B, S, shared, total)
HAND_CASES = [
    # three steps, all common; nothing is left of either list
    ("identical", [1, 2, 3], [1, 2, 3], 3, 3, 3),
    ("identical_s_larger", [1, 2, 3], [1, 2, 3], 5, 3, 3),
    # 1, 2, 3, 4 are taken one by one: denom reaches S = 4 before a list runs out
    ("disjoint_stops_at_s", [1, 3, 5], [2, 4, 6], 4, 0, 4),
    # 1 .. 5 taken, A runs out at denom = 5; what is left of B ([6]) completes it to 6
    ("disjoint_runs_out", [1, 3, 5], [2, 4, 6], 10, 0, 6),
    # 1 (denom 1), 2 in both (denom 2, A runs out); [3] is left of B -> 3
    ("union_smaller_than_s", [1, 2], [2, 3], 10, 1, 3),
    # no step; 0 + 3 left of B, clamped to S = 2
    ("one_empty_clamped", [], [4, 5, 6], 3, 0, 3),
    ("one_empty", [4, 5, 6], [], 5, 0, 3),
    ("one_empty_s1", [], [7], 1, 0, 1),
    ("both_empty", [], [], 4, 0, 0),
    # 1 (denom 1), 2 (denom 2), 5 in both (denom 3 = S): the walk ends on the common element, which counts
    ("s_reached_on_common", [1, 5, 9], [2, 5, 7], 3, 1, 3),
    # 1 (denom 1), 2 (denom 2 = S): the common 5 lies behind the stop and does not count
    ("common_behind_the_stop", [1, 5], [2, 5], 2, 0, 2),
    # values that differ only in their top or only in their bottom half
    ("halves", [1 << 32, (1 << 32) + 1, 2 << 32], [1, (1 << 32) + 1, (2 << 32) + 1], 6, 1, 5),
]
