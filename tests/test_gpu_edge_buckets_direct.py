"""The bucket route of the edge sort (radix_edge_buckets, csrc/radix.hip) on its own, through sw_edge_buckets, on the crafted key
multisets of tests/tools/eb_cases.py -- every width of the key from 10 to 62 bits, tiles, chunks, the LDS table and the capacities
at their bounds, sentinels in every mix -- against numpy: np.unique of the real keys, the exclusive cumulative sum of the counts.

What each case is and which route it must take are facts about the input, checked without a GPU in tests/test_edge_buckets_cpu.py;
nothing here reads the routine's debug line.  Every comparison is exact."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import eb_cases as E  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = E.cases()
BY_ID = {c.id: c for c in CASES}
PAD = 16                       # guard words behind every buffer
GUARD64, GUARD32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
_device_ms = [0.0, 0]          # device time of all sw_edge_buckets calls of this module, and their number


@pytest.fixture(scope="module", autouse=True)
def _report_device_time():
    yield
    print(f"\n[edge buckets, direct] {_device_ms[1]} calls, {_device_ms[0]:.1f} ms of device time")


def run(case, hist=False):
    """one call on fresh device buffers -> dict(done, n_runs, in_alt, ukeys, ucnt, multiset)"""
    import torch
    from seqwin_amd._lib import c_vp, check, lib
    m, L = len(case.keys), E.layout(case.key_bits)
    dev = "cuda"
    buf = [torch.full((m + PAD,), GUARD64, dtype=torch.int64, device=dev) for _ in range(2)]   # (each its own allocation, like the library's)
    buf[0][:m] = torch.from_numpy(case.keys.view(np.int64)).to(dev)
    ukeys = torch.full((m + PAD,), GUARD64, dtype=torch.int64, device=dev)
    ucnt = torch.full((m + 1 + PAD,), GUARD32, dtype=torch.int32, device=dev)
    h = torch.from_numpy(E.hist_top(case.keys, L).view(np.int64)).to(dev) if hist else None
    n_runs, done, in_alt = ctypes.c_uint64(1 << 40), ctypes.c_int(-1), ctypes.c_int(-1)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    check(lib.sw_edge_buckets(c_vp(buf[0].data_ptr()), c_vp(buf[1].data_ptr()), m, case.key_bits, case.cap, case.slots,
                              c_vp(h.data_ptr()) if hist else None, c_vp(ukeys.data_ptr()), c_vp(ucnt.data_ptr()), ctypes.byref(n_runs),
                              ctypes.byref(done), ctypes.byref(in_alt), None))
    e1.record()
    torch.cuda.synchronize()
    _device_ms[0] += e0.elapsed_time(e1)
    _device_ms[1] += 1
    assert done.value in (0, 1) and in_alt.value in (0, 1) and n_runs.value <= m
    # nothing was written behind the buffers
    assert all(bool((b[m:] == GUARD64).all()) for b in buf) and bool((ukeys[m:] == GUARD64).all()) and bool((ucnt[m + 1:] == GUARD32).all())
    n = n_runs.value
    return dict(done=done.value, n_runs=n, in_alt=in_alt.value, ukeys=ukeys[:n].cpu().numpy().view(np.uint64),
                ucnt=ucnt[:n + 1].cpu().numpy().view(np.uint32), multiset=buf[in_alt.value][:m].cpu().numpy().view(np.uint64), buffers=buf)


def check_result(case, got):
    """the route the model expects, then the numpy reference (done) or the fallback contract (declined)"""
    import torch
    from seqwin_amd._lib import c_vp, check, lib
    m = len(case.keys)
    assert got["done"] == int(E.expected_done(case)), (case.id, got["done"], E.bucket_stats(case.keys, case.key_bits), case.cap, case.slots)
    want_sorted = np.sort(case.keys)
    assert np.array_equal(np.sort(got["multiset"]), want_sorted), case.id   # the input multiset, sentinels included, either way
    if got["done"]:
        uk, uc = E.reference(case.keys, case.key_bits)
        assert got["n_runs"] == len(uk), (case.id, got["n_runs"], len(uk))
        assert np.array_equal(got["ukeys"], uk), case.id
        assert got["ucnt"].dtype == uc.dtype and np.array_equal(got["ucnt"], uc), case.id   # all run starts and the final total
        return
    assert got["n_runs"] == 0
    # declined: the caller sorts the buffer it was left with by radix passes over all key bits
    buf, src = got["buffers"], got["in_alt"]
    flag = ctypes.c_int(-1)
    check(lib.sw_sort_keys64(c_vp(buf[src].data_ptr()), c_vp(buf[1 - src].data_ptr()), m, 0, case.key_bits, None, ctypes.byref(flag), None))
    torch.cuda.synchronize()
    out = buf[1 - src if flag.value else src][:m].cpu().numpy().view(np.uint64)
    assert np.array_equal(out, want_sorted), case.id


def same(a, b):
    return all(a[f] == b[f] for f in ("done", "n_runs")) and np.array_equal(a["ukeys"], b["ukeys"]) and np.array_equal(a["ucnt"], b["ucnt"])


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_against_numpy(case, monkeypatch):
    """the top-digit counts counted by the routine and handed in (np.bincount of the model's level-1 digit, 2^digit width entries):
    both against the reference, and identical"""
    monkeypatch.delenv("SEQWIN_AMD_RADIX_RANK", raising=False)
    counted = run(case, hist=False)
    check_result(case, counted)
    given = run(case, hist=True)
    check_result(case, given)
    assert same(counted, given) and counted["in_alt"] == given["in_alt"], case.id


RANK_SUBSET = ["mixed-kb16", "mixed-kb18", "mixed-kb22", "mixed-kb54", "mixed-kb62", "l1_tiles-kb22", "l1_tiles-kb54", f"m_{E.TILE + 1}-kb54",
               "chunk_2049-kb30", "l1_every_bucket_one_key-kb54", "l1_single_bucket-kb22", "distinct_eq_slots8192-kb54",
               "distinct_over_slots64-kb22", "one_key_2pow20-kb54", "interleaved_copies-kb54", "all_distinct-kb30", "sentinels_shared-kb62",
               "sentinels_only-kb22", "cap_sent_at-kb22", "cap_sent_above-kb54", "cap_other_above-kb22", "mixed_sorted-kb54"]


@pytest.mark.parametrize("cid", RANK_SUBSET)
def test_both_rank_modes_give_the_same(cid, monkeypatch):
    """SEQWIN_AMD_RADIX_RANK=ballot|atomic (test library): the bucket passes rank inside a wave by ballots or by LDS atomics"""
    case, got = BY_ID[cid], {}
    for mode in ("ballot", "atomic"):
        monkeypatch.setenv("SEQWIN_AMD_RADIX_RANK", mode)
        got[mode] = run(case, hist=(mode == "ballot"))
        check_result(case, got[mode])
    assert same(got["ballot"], got["atomic"]), cid


def test_a_case_twice_and_between_others():
    """scratch from the pool, tickets, flags and tables are fresh on every call: the same case again after a different geometry, after
    a declined call and after an overflowing table gives the same answer"""
    order = ["mixed-kb54", "mixed-kb54", "distinct_over_slots8192-kb54", "mixed-kb54", "cap_sent_above-kb22", "mixed-kb22", "mixed-kb22",
             "one_key_2pow20-kb54", "mixed-kb54", "sentinels_only-kb54", "mixed-kb22", "mixed-kb8", "mixed-kb54"]
    first = {}
    for cid in order:
        got = run(BY_ID[cid], hist=False)
        check_result(BY_ID[cid], got)
        if cid in first:
            assert same(first[cid], got), cid
        first.setdefault(cid, got)


_RELEASE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests"); sys.path.insert(0, sys.argv[1] + "/tests/tools")
from seqwin_amd._lib import LIB_PATH
assert str(LIB_PATH).endswith("libseqwin_hip.so"), LIB_PATH
import test_gpu_edge_buckets_direct as T
for cid in sys.argv[2:]:
    for hist in (False, True):
        T.check_result(T.BY_ID[cid], T.run(T.BY_ID[cid], hist=hist))
    print("ok", cid)
"""


def test_through_the_release_library():
    """sw_edge_buckets is exported by the release library too (no test hooks): a done case and both kinds of declined ones, in a fresh
    interpreter without the suite's SEQWIN_AMD_LIB"""
    ids = ["mixed-kb54", "l1_tiles-kb22", "cap_other_above-kb22", "distinct_over_slots64-kb54"]
    env = {k: v for k, v in os.environ.items() if k not in ("SEQWIN_AMD_LIB", "SEQWIN_AMD_RADIX_RANK")}
    r = subprocess.run([sys.executable, "-c", _RELEASE_CHILD, str(ROOT)] + ids, capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    assert [ln for ln in r.stdout.split("\n") if ln.startswith("ok ")] == [f"ok {c}" for c in ids], r.stdout
