"""CPU: the crafted inputs of the edge bucket sort (tests/tools/eb_cases.py) are what their names say, and the model of the bucket
geometry they are built on is right.

tests/test_gpu_edge_buckets_direct.py runs every case through sw_edge_buckets and expects the route expected_done() gives.  That
expectation must be a fact about the input: here every case's claims (written down from the builder's intent) are checked against
the model (sub-bucket, bin and digit of every key), the model's layout against hand-derived literals, the generator's output against
pinned digests, and the generator's sizes against the constants in the source text of csrc/radix.hip and csrc/index.hip.  The new
entry point's argument validation is checked too: it happens before a device is touched."""
import ctypes
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import eb_cases as E  # noqa: E402

from seqwin_amd._lib import c_vp, check, lib  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "edge_buckets" / "cases.json"
CASES = E.cases()
BY_ID = {c.id: c for c in CASES}


def test_layout_against_hand_derived_values():
    """ceil(bits / 8) and ceil(bits / 9) by hand, then the digits from the top: e.g. 54 bits are 7 digits of 8 or 6 of 9 -> 9-bit
    digits, the top one at bit 45 is full, nine bits below it, nine below those, bins end at bit 27; 22 bits are 3 digits either way
    -> 8-bit digits, the top one at bit 16 has 6 bits, the level-2 digit the nine bits [7, 16), the bins the seven bits left."""
    want = {   # key_bits: digit, n_passes, shift1, bits1, bits2, shift2, bin_bits, bin_shift
        10: (8, 2, 8, 2, 8, 0, 0, 0),
        16: (8, 2, 8, 8, 8, 0, 0, 0),
        18: (9, 2, 9, 9, 9, 0, 0, 0),
        20: (8, 3, 16, 4, 9, 7, 7, 0),
        22: (8, 3, 16, 6, 9, 7, 7, 0),
        30: (8, 4, 24, 6, 9, 15, 9, 6),
        54: (9, 6, 45, 9, 9, 36, 9, 27),
        62: (9, 7, 54, 8, 9, 45, 9, 36),
    }
    for kb, t in want.items():
        assert tuple(E.layout(kb))[1:] == t, kb
    assert [E.layout(kb).n_passes for kb in (1, 8, 9)] == [1, 1, 1]
    assert sorted({E.layout(kb).bits1 for kb in E.SWEEP_BITS}) == [2, 4, 5, 6, 7, 8, 9] and [E.layout(kb).bits1 for kb in E.ODD_BITS] == [3, 3]
    assert {E.layout(kb).digit for kb in E.SWEEP_BITS} == {8, 9}
    assert min(E.layout(kb).bits1 for kb in range(10, 63)) == 2   # (8 k + 1 bits take 9-bit digits, 9 j + 1 bits 8-bit ones)
    for kb in range(1, 63):
        L = E.layout(kb)
        assert L.shift1 + L.bits1 == kb and L.shift2 + L.bits2 == L.shift1 and L.bin_shift + L.bin_bits == L.shift2
        assert 1 <= L.bits1 <= L.digit and L.bits2 <= 9 and L.bin_bits <= 9 and L.bin_shift >= 0


def test_model_places_a_hand_made_key():
    """key_bits 30: level-1 digit = bits [24, 30), level-2 = [15, 24), bin = [6, 15)"""
    L = E.layout(30)
    k = (0b101101 << 24) | (0b110000011 << 15) | (0b000000111 << 6) | 0b101010
    assert int(E.digit1([k], L)[0]) == 0b101101 and int(E.digit2([k], L)[0]) == 0b110000011
    assert int(E.sub_bucket([k], L)[0]) == 0b101101 * 512 + 0b110000011 and int(E.bin_of([k], L)[0]) == 0b111
    assert int(E.compose(L, 0b101101, 0b110000011, 0b111, 0b101010)) == k
    assert E.sentinel(30) == 0x3FFFFFFF and int(E.sub_bucket([E.sentinel(30)], L)[0]) == 63 * 512 + 511
    # the multiplicative hash, by Python integers
    for key in (k, 1, (1 << 54) - 2):
        assert int(E.hash_slot([key], 1024)[0]) == ((key * 0x9E3779B97F4A7C15) % (1 << 64) >> 40) % 1024
    uk, uc = E.reference(np.array([5, 3, 5, E.sentinel(30), 3, 5, 9], np.uint64), 30)
    assert uk.tolist() == [3, 5, 9] and uc.tolist() == [0, 2, 5, 6]


def test_generator_constants_follow_the_source():
    """the tile, chunk, table and slot sizes the cases are built around are those of the kernels today"""
    radix = (ROOT / "seqwin_amd" / "csrc" / "radix.hip").read_text()
    index = (ROOT / "seqwin_amd" / "csrc" / "index.hip").read_text()
    body = radix[radix.index("int radix_edge_buckets("):]
    items = int(re.search(r"constexpr int RS_ITEMS = (\d+);", radix).group(1))
    threads, bits = (int(x) for x in re.search(r"constexpr int THREADS = (\d+), BITS = (\d+);", body).groups())
    assert items * threads == E.TILE and 1 << bits == E.RADIX and re.search(r"TILE = THREADS \* RS_ITEMS", body)
    eb_radix, eb_threads = (int(x) for x in re.search(r"EB_RADIX = (\d+), EB_TABLE = EB_RADIX \* EB_RADIX, EB_THREADS = (\d+);", radix).groups())
    assert eb_radix == E.RADIX and re.search(r"j0 \+= 4 \* EB_THREADS", radix) and 4 * eb_threads == E.CHUNK
    lo, hi = (int(x) for x in re.search(r"slots < (\d+) \|\| slots > (\d+) \|\| \(slots & \(slots - 1\)\)", body).groups())
    assert (lo, hi) == (E.SLOTS_MIN, E.SLOTS_MAX)
    mul, shift = re.search(r"\(k \* (0x[0-9A-Fa-f]+)ull\) >> (\d+)\) & mask", radix).groups()
    assert int(mul, 16) == E.HASH_MUL and int(shift) == E.HASH_SHIFT
    cap, slots = re.search(r"EDGE_BUCKET_CAP = 1u << (\d+), EDGE_BUCKET_SLOTS = (\d+);", index).groups()
    assert 1 << int(cap) == E.DEFAULT_CAP and int(slots) == E.DEFAULT_SLOTS
    assert re.search(r"\(bits \+ 8\) / 9 < \(bits \+ 7\) / 8", radix)   # (9-bit digits where they save a pass)


def test_the_sweep_and_the_list_of_cases():
    assert E.SWEEP_BITS == tuple(range(10, 63, 2))
    swept = {c.key_bits for c in CASES if c.name == "mixed"}
    assert swept == set(E.SWEEP_BITS) | set(E.DECLINED_BITS) | set(E.ODD_BITS)
    names = {c.name for c in CASES}
    for want in ("l1_tiles", "m_1_real", "m_1_sentinel", "m_2", "m_100", f"m_{E.TILE}", f"m_{E.TILE + 1}", "chunk_2047", "chunk_2048",
                 "chunk_2049", "l1_every_bucket_one_key", "l1_single_bucket", "distinct_eq_slots64", "distinct_eq_slots8192",
                 "distinct_over_slots64", "distinct_over_slots8192", "probe_chain_slots64", "probe_chain_slots1024", "one_bin", "all_bins",
                 "differ_bit0", "one_key_2pow20", "interleaved_copies", "all_distinct", "sentinels_shared", "sentinels_alone",
                 "sentinels_none", "sentinels_only", "cap_sent_at", "cap_sent_above", "cap_sent_below", "cap_other_at", "cap_other_above",
                 "cap_other_below", "mixed_sorted", "mixed_reversed", "mixed_shuffled", "bad_slots63"):
        assert want in names, want
    assert max(len(c.keys) for c in CASES) <= (1 << 20) + 64 and sum(len(c.keys) for c in CASES) < 8_000_000


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_is_what_its_name_says(case):
    L, S = E.layout(case.key_bits), np.uint64(E.sentinel(case.key_bits))
    keys, cl = case.keys, case.claims
    assert keys.dtype == np.uint64 and keys.ndim == 1 and len(keys) < (1 << 32) - 1
    assert len(keys) == 0 or int(keys.max()) <= int(S)   # inside the routine's preconditions
    real = E.real_keys(keys, case.key_bits)
    n_sent = len(keys) - len(real)
    largest, distinct = E.bucket_stats(keys, case.key_bits)
    l1 = np.bincount(E.digit1(keys, L), minlength=1 << L.digit) if len(keys) else np.zeros(1 << L.digit, np.int64)
    assert int(E.hist_top(keys, L).sum()) == len(keys) and len(E.hist_top(keys, L)) == 1 << L.digit
    if "sentinels" in cl:
        assert n_sent == cl["sentinels"]
    if "real" in cl:
        assert len(real) == cl["real"]
    if "m" in cl:
        assert len(keys) == cl["m"]
    if "largest" in cl:
        assert largest == cl["largest"]
    if "distinct" in cl:
        assert distinct == cl["distinct"]
    if "l1_sizes" in cl:
        for d, size in cl["l1_sizes"].items():
            assert int(l1[d]) == size, (d, int(l1[d]))
    if "l1_occupied" in cl:
        assert int((l1 > 0).sum()) == cl["l1_occupied"]
    if "l1_all_ones" in cl:
        assert cl["l1_all_ones"] == 1 << L.bits1 and l1[: 1 << L.bits1].tolist() == [1] * (1 << L.bits1)
    if "real_with_sentinels" in cl:
        assert int((E.sub_bucket(real, L) == int(E.sub_bucket([S], L)[0])).sum()) == cl["real_with_sentinels"]
    if "bins" in cl:   # the distinct keys of the fullest sub-bucket over its bins
        u = np.unique(real)
        sb = E.sub_bucket(u, L)
        ids, counts = np.unique(sb, return_counts=True)
        fullest = u[sb == ids[counts.argmax()]]
        assert len(np.unique(E.bin_of(fullest, L))) == cl["bins"] and len(fullest) == cl["distinct"]
        if cl["bins"] == 1:
            assert len(fullest) > 1 and len(np.unique(fullest >> np.uint64(L.bin_shift))) == 1   # they differ only below bin_shift
    if "hash_span" in cl:
        at, width = cl["hash_span"]
        u = np.unique(real)
        assert ((E.hash_slot(u, case.slots) - at) % case.slots < width).all() and len(u) == cl["distinct"] and len(u) > 0.9 * case.slots
    if cl.get("bit0_pairs"):
        u = np.unique(real)
        assert np.array_equal(np.unique(u ^ np.uint64(1)), u) and len(np.unique(E.bin_of(u, L))) >= min(64, 1 << L.bin_bits)
    if cl.get("all_distinct"):
        assert len(np.unique(real)) == len(real) > 50000
    if "order" in cl:
        d = np.diff(keys.astype(np.int64))
        assert {"sorted": (d >= 0).all(), "reversed": (d <= 0).all(), "shuffled": (d < 0).any() and (d > 0).any()}[cl["order"]]
        assert np.array_equal(np.sort(keys), np.sort(BY_ID[f"mixed-kb{case.key_bits}"].keys))
    if "slots_valid" in cl:
        assert E.slots_valid(case.slots) == cl["slots_valid"]
    # the expected route, from the name
    n = case.name
    if n.startswith("distinct_eq"):
        assert distinct == case.slots and E.expected_done(case)
    elif n.startswith("distinct_over"):
        assert distinct == case.slots + 1 and largest <= case.cap and not E.expected_done(case)
    elif n.startswith("cap_"):
        delta = {"at": 0, "above": 1, "below": -1}[n.split("_")[2]]
        assert largest == case.cap + delta and distinct <= case.slots and n_sent > case.cap
        in_sent = cl["real_with_sentinels"]
        assert (in_sent == largest) == (n.split("_")[1] == "sent")
        assert E.expected_done(case) == (delta <= 0)
    elif n.startswith("bad_slots"):
        assert not E.expected_done(case) and E.expected_done(BY_ID[f"mixed-kb{case.key_bits}"])
    elif case.key_bits in E.DECLINED_BITS:
        assert not E.expected_done(case)
    else:
        assert E.expected_done(case), (largest, distinct)
    if n.startswith("chunk_"):
        assert largest == int(n.split("_")[1]) and largest - E.CHUNK in (-1, 0, 1)
    if n == "l1_tiles":
        assert sorted(int(x) for x in l1[:4]) == sorted([E.TILE - 1, E.TILE, E.TILE + 1, 2 * E.TILE]) and int(l1[(1 << L.bits1) - 1]) == n_sent
    if n == "one_key_2pow20":
        assert int(np.unique(real, return_counts=True)[1].max()) == 1 << 20
    if n == "interleaved_copies":
        rows = keys.reshape(-1, 64)
        rest = rows[:, 1:]
        assert len(np.unique(rows[:, 0])) == len(rows) and not np.isin(rows[:, 0], rest).any() and len(np.unique(rest)) == 4
    if n == "sentinels_only":
        assert len(real) == 0 and E.reference(keys, case.key_bits)[1].tolist() == [0]


def test_generator_output_is_pinned():
    """a sha256 per case (tests/golden/edge_buckets/cases.json; `python tests/tools/eb_cases.py --pin` rewrites it, on purpose only)"""
    pinned = json.loads(GOLDEN.read_text())
    assert sorted(pinned) == sorted(BY_ID)
    for cid, c in BY_ID.items():
        assert E.digest(c) == pinned[cid], cid
    again = {c.id: E.digest(c) for c in E.cases()}
    assert again == pinned


def _call(keys=1, alt=1, m=1, key_bits=22, cap=1000, slots=4096, ukeys=1, ucnt=1, outs=True):
    n_runs, done, in_alt = ctypes.c_uint64(77), ctypes.c_int(77), ctypes.c_int(77)
    refs = [ctypes.byref(x) for x in (n_runs, done, in_alt)] if outs else [None, None, None]
    rc = lib.sw_edge_buckets(c_vp(keys), c_vp(alt), m, key_bits, cap, slots, None, c_vp(ukeys), c_vp(ucnt), *refs, None)
    return rc, n_runs.value, done.value, in_alt.value


def test_sw_edge_buckets_validates_its_arguments_before_touching_a_device():
    """SW_ERR_VALUE (ValueError) for a key width outside [1, 62], a capacity of 2^32 or more, missing result pointers and NULL buffers
    with m > 0 -- with or without a GPU, the buffers are never looked at; m = 0 is declined without a device"""
    for bad in (dict(key_bits=0), dict(key_bits=63), dict(key_bits=64), dict(key_bits=1 << 40), dict(cap=1 << 32), dict(outs=False),
                dict(keys=None), dict(alt=None), dict(ukeys=None), dict(ucnt=None)):
        rc = _call(**bad)[0]
        assert rc == 2, bad
        with pytest.raises(ValueError):
            check(rc)
    assert b"key_bits" in lib.sw_last_error() or _call(key_bits=63)[0] == 2 and b"key_bits" in lib.sw_last_error()
    assert _call(keys=None, alt=None, ukeys=None, ucnt=None, m=0) == (0, 0, 0, 0)
