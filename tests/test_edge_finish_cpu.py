"""The generators of tests/tools/eb_finish_cases.py without a GPU: every builder asserts that its case is what its name says, and the
model of the packed form's eligibility is checked on its boundary."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import eb_cases as E  # noqa: E402
import eb_finish_cases as F  # noqa: E402

CASES = F.cases()


def test_every_case_builds_and_is_deterministic():
    again = {c.id: E.digest(c) for c in F.cases()}
    assert again == {c.id: E.digest(c) for c in CASES} and len(CASES) >= 30
    for c in CASES:
        assert c.keys.dtype == np.uint64 and 0 < len(c.keys) < 300_000 and int(c.keys.max()) <= E.sentinel(c.key_bits), c.id
        assert not c.claims["ordered"] or len(c.keys) <= E.TILE, c.id
    assert not set(c.id for c in CASES) & set(c.id for c in E.cases())


def test_step_sizes_and_routes():
    by = {c.id: c for c in CASES}
    assert {s for s in F.STEP_SIZES} == {1, 2047, 2048, 2049, 4095, 4096, 4097, 6145}
    for s in F.STEP_SIZES:
        assert E.bucket_stats(by[f"steps_{s}-kb54"].keys, 54)[0] == s
    assert not E.expected_done(by["table_over_slots64-kb54"]) and not E.expected_done(by["table_over_slots1024-kb54"])
    assert all(E.expected_done(c) for c in CASES if not c.name.startswith("table_over"))


def test_eligibility_rule_on_its_boundary():
    """packed iff shift2 + bit length of the largest sub-bucket <= 63: 2^18 - 1 keys at shift2 = 45 are in, 2^18 are out"""
    by = {c.id: c for c in CASES}
    assert E.layout(62).shift2 == 45 and F.count_bits(0) == 1 and F.count_bits((1 << 18) - 1) == 18 and F.count_bits(1 << 18) == 19
    assert F.eligible(by["packed_limit_one_key-kb62"]) and F.eligible(by["packed_limit_corners-kb62"])
    assert not F.eligible(by["packed_limit_one_key_over-kb62"])
    assert F.expected_done(by["packed_limit_one_key_over-kb62"], "plain") and F.expected_done(by["packed_limit_one_key_over-kb62"], None)
    assert not F.expected_done(by["packed_limit_one_key_over-kb62"], "packed")
    assert [c.id for c in CASES if not F.eligible(c)] == ["packed_limit_one_key_over-kb62"]


def test_forced_packed_declines_a_proper_part_of_the_cases():
    """What SEQWIN_AMD_EDGE_FINISH=packed must decline for the rule's sake, computed here.  No key width up to 62 bits leaves fewer than
    19 bits for the count (shift2 <= 45), and none of the 125 cases of eb_cases.py has a sub-bucket of 2^18 keys at such a width: among
    them alone the set is EMPTY, whatever the library does.  The sweep of the GPU module therefore runs those 125 together with this
    module's cases, where the set is not empty and far from half -- a hook that never declines fails on it, one that always declines
    fails on all the others."""
    sweep = E.cases() + CASES
    by_rule = [c.id for c in sweep if E.expected_done(c) and not F.eligible(c)]
    assert [c.id for c in E.cases() if E.expected_done(c) and not F.eligible(c)] == []
    assert 0 < len(by_rule) <= len(sweep) // 2 and by_rule == ["packed_limit_one_key_over-kb62"]


def test_the_sequence_names_known_cases():
    ids = {c.id for c in E.cases()} | {c.id for c in CASES}
    assert all(cid in ids and form in F.FORMS for cid, form in F.SEQUENCE)
    assert {"packed", "plain", None} == {f for _, f in F.SEQUENCE}
    by = {c.id: c for c in E.cases() + CASES}
    assert {by[cid].slots for cid, _ in F.SEQUENCE} == {64, 4096, 8192}
    assert any(not F.expected_done(by[cid], form) for cid, form in F.SEQUENCE)
