"""The finish kernel of the edge sort's bucket route (csrc/radix.hip: k_eb_finish<PACKED>) through sw_edge_buckets on the test library:
the double-buffered key loop at its step boundaries, the batched probes, the packed word at its limits, the list of live sub-buckets,
and both forms of the slot forced by SEQWIN_AMD_EDGE_FINISH=packed|plain.  Cases and the model of the eligibility rule
(packed iff shift2 + bit length of the largest sub-bucket <= 63) are in tests/tools/eb_finish_cases.py, the expected result is
eb_cases.reference (numpy); every comparison is exact, with guard words behind all five buffers (the direct module's `run`)."""
from __future__ import annotations

import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
sys.path.insert(0, str(ROOT / "tests"))
import eb_cases as E  # noqa: E402
import eb_finish_cases as F  # noqa: E402
from test_gpu_edge_buckets_direct import run  # noqa: E402

pytestmark = pytest.mark.gpu

OWN = F.cases()
SWEEP = E.cases() + OWN
BY_ID = {c.id: c for c in SWEEP}
_FORM = re.compile(r"\[edge buckets\] .*; (\d+) live sub-buckets, (packed|plain) slots( do not fit: radix passes instead)?, (\d+) workgroups per CU")


def check(case, got, want_done):
    import torch
    from seqwin_amd._lib import c_vp, check as ok, lib
    m = len(case.keys)
    assert got["done"] == int(want_done), (case.id, got["done"], E.bucket_stats(case.keys, case.key_bits), case.cap, case.slots)
    want_sorted = np.sort(case.keys)
    assert np.array_equal(np.sort(got["multiset"]), want_sorted), case.id   # the input multiset, sentinels included, either way
    if got["done"]:
        uk, uc = E.reference(case.keys, case.key_bits)
        assert got["n_runs"] == len(uk), (case.id, got["n_runs"], len(uk))
        assert np.array_equal(got["ukeys"], uk), case.id
        assert got["ucnt"].dtype == uc.dtype and np.array_equal(got["ucnt"], uc), case.id
        return
    assert got["n_runs"] == 0
    buf, src = got["buffers"], got["in_alt"]   # declined: the buffer the caller was left with sorts to the input
    flag = ctypes.c_int(-1)
    ok(lib.sw_sort_keys64(c_vp(buf[src].data_ptr()), c_vp(buf[1 - src].data_ptr()), m, 0, case.key_bits, None, ctypes.byref(flag), None))
    torch.cuda.synchronize()
    assert np.array_equal(buf[1 - src if flag.value else src][:m].cpu().numpy().view(np.uint64), want_sorted), case.id


def run_form(case, form, monkeypatch, capfd, hist=False):
    """one call under a forced form (None: the routine's choice); the form that ran is read from the debug line"""
    monkeypatch.setenv("SEQWIN_AMD_DEBUG_EDGE_REPAIR", "1")
    if case.claims.get("ordered"):   # (ranked by ballots, the passes keep the order inside a sub-bucket: eb_finish_cases.py)
        monkeypatch.setenv("SEQWIN_AMD_RADIX_RANK", "ballot")
    else:
        monkeypatch.delenv("SEQWIN_AMD_RADIX_RANK", raising=False)
    if form:
        monkeypatch.setenv("SEQWIN_AMD_EDGE_FINISH", form)
    else:
        monkeypatch.delenv("SEQWIN_AMD_EDGE_FINISH", raising=False)
    capfd.readouterr()
    got = run(case, hist=hist)
    err = capfd.readouterr().err
    check(case, got, F.expected_done(case, form))
    m = _FORM.search(err)
    if E.layout(case.key_bits).n_passes >= 2 and E.slots_valid(case.slots) and len(case.keys):
        assert m, err[-1500:]
        assert m.group(2) == (form or F.chosen_form(case)), (case.id, form, m.group(0))
        assert (m.group(3) is not None) == (form == "packed" and not F.eligible(case)), m.group(0)
        assert int(m.group(1)) == len(np.unique(E.sub_bucket(case.keys, E.layout(case.key_bits)))), m.group(0)
        assert int(m.group(4)) >= 1
    return got, m


@pytest.mark.parametrize("case", OWN, ids=[c.id for c in OWN])
def test_case_under_both_forms(case, monkeypatch, capfd):
    """every case of this module under the routine's own choice and both forced forms; where the packed form does not fit, the forced
    packed call is declined with the multiset untouched.  All forms give the same arrays."""
    got = {form: run_form(case, form, monkeypatch, capfd, hist=(form == "plain"))[0] for form in F.FORMS}
    for form in ("packed", "plain"):
        if got[form]["done"] and got[None]["done"]:
            assert got[form]["n_runs"] == got[None]["n_runs"] and np.array_equal(got[form]["ukeys"], got[None]["ukeys"])
            assert np.array_equal(got[form]["ucnt"], got[None]["ucnt"])


def test_the_limit_of_the_packed_word_from_the_debug_line(monkeypatch, capfd):
    """2^18 - 1 copies of one key at 62 bits: shift2 + cb = 45 + 18 = 63, packed, the count field all ones; one more key: plain"""
    _, m = run_form(BY_ID["packed_limit_one_key-kb62"], None, monkeypatch, capfd)
    assert m.group(2) == "packed"
    _, m = run_form(BY_ID["packed_limit_one_key_over-kb62"], None, monkeypatch, capfd)
    assert m.group(2) == "plain"
    got, m = run_form(BY_ID["packed_limit_one_key_over-kb62"], "packed", monkeypatch, capfd)
    assert got["done"] == 0 and m.group(3)


def test_workgroups_per_cu_at_the_default_table(monkeypatch, capfd):
    """4096 slots: 10 bytes a slot leave room for three workgroups on a CU, 14 bytes for two"""
    _, m = run_form(BY_ID["steps_4097-kb54"], "packed", monkeypatch, capfd)
    assert int(m.group(4)) == 3, m.group(0)
    _, m = run_form(BY_ID["steps_4097-kb54"], "plain", monkeypatch, capfd)
    assert int(m.group(4)) == 2, m.group(0)


@pytest.mark.parametrize("case", E.cases(), ids=[c.id for c in E.cases()])
def test_all_cases_of_the_direct_module_forced_packed(case, monkeypatch, capfd):
    """declined exactly where the case declines for its own reasons or the rule says the word does not fit (no such case among these
    125: tests/test_edge_finish_cpu.py; the sweep's non-empty part is this module's packed_limit_one_key_over, run above)"""
    run_form(case, "packed", monkeypatch, capfd)


def test_the_declined_set_of_the_sweep_is_the_models():
    by_rule = {c.id for c in SWEEP if E.expected_done(c) and not F.eligible(c)}
    declined = {c.id for c in SWEEP if not F.expected_done(c, "packed")}
    assert by_rule == declined - {c.id for c in SWEEP if not E.expected_done(c)}
    assert 0 < len(by_rule) <= len(SWEEP) // 2


def test_a_sequence_of_calls_alternating_forms(monkeypatch, capfd):
    """the dynamic LDS attribute is state of the process: forms, 64 / 4096 / 8192 slots and declined calls in turn"""
    first = {}
    for cid, form in F.SEQUENCE:
        got, _ = run_form(BY_ID[cid], form, monkeypatch, capfd)
        if got["done"]:
            if cid in first:
                assert np.array_equal(first[cid]["ukeys"], got["ukeys"]) and np.array_equal(first[cid]["ucnt"], got["ucnt"]), (cid, form)
            first.setdefault(cid, got)
