"""The node stage's yardstick and case generator (tests/tools/nodes_host.py) on the host: reference() against the oracle on real
indexes, and every crafted case of tests/test_gpu_nodes_direct.py against the bound it aims at (no GPU)."""
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import oracle

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import nodes_host as H  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
SMOKE = [GOLDEN / "smoke" / p for p in ("targets/target-1.fasta", "targets/target-2.fasta", "non-targets/non-target-1.fasta",
                                        "non-targets/non-target-2.fasta")]
PAN = sorted((GOLDEN / "synth").glob("pan_*.fa"))
REAL = {"smoke_k17_w10": (SMOKE, 17, 10, [True, True, False, False]),
        "pan_k15_w20": (PAN, 15, 20, [i % 2 == 0 for i in range(len(PAN))])}


@pytest.mark.parametrize("name", sorted(REAL))
def test_reference_returns_the_oracles_index(name):
    paths, k, w, tar = REAL[name]
    assert len(paths) == len(tar) >= 4
    ek, en, _, eo, _ = oracle.build(paths, k, w)
    oracle.get_penalty(ek, en, eo, tar)
    assert len(ek) > 1_000 and (en["n_tar"] > 1).any() and (en["n_neg"] > 1).any()
    # the rows the index came from: a row's hash is its node's, and the rows go back to (record, pos) order
    h_sorted = np.repeat(en["hash"], (en["stop"] - en["start"]).astype(np.int64))
    back = np.lexsort((ek["pos"], ek["record_idx"]))
    rows = np.stack([h_sorted[back], ek["pos"][back].astype(np.uint64) | (ek["record_idx"][back].astype(np.uint64) << np.uint64(32))],
                    axis=1)
    kmers, nodes, ranks = H.reference(rows, 0, eo, tar)
    assert kmers.dtype == ek.dtype and np.array_equal(kmers, ek)
    assert nodes.dtype == en.dtype
    for f in ("hash", "start", "stop", "n_tar", "n_neg"):
        assert np.array_equal(nodes[f], en[f]), f
    assert np.array_equal(nodes["penalty"].view(np.uint64), en["penalty"].view(np.uint64))
    node_of = np.searchsorted(en["hash"], rows[:, 0])
    assert ranks.dtype == np.uint32 and np.array_equal(ranks & np.uint32(0x7FFFFFFF), node_of.astype(np.uint32))
    # bit 31, counted the slow way: the row's node holds more than one row of the row's assembly (rare or absent in these indexes:
    # test_reference_on_a_hand_made_index has marked rows)
    asm = np.searchsorted(eo.astype(np.int64), (rows[:, 1] >> np.uint64(32)).astype(np.int64), side="right") - 1
    seen = Counter(zip(node_of.tolist(), asm.tolist()))
    want = np.array([seen[(a, b)] > 1 for a, b in zip(node_of.tolist(), asm.tolist())])
    assert not want.all() and np.array_equal(ranks >> np.uint32(31), want.astype(np.uint32))
    # without targets: the same arrays, counts and penalty zero, the marks unchanged; a base moves start / stop only
    k2, n2, r2 = H.reference(rows, 2**32 - 5, eo, None)
    assert np.array_equal(k2, ek) and np.array_equal(r2, ranks) and np.array_equal(n2["hash"], en["hash"])
    assert np.array_equal(n2["start"], en["start"] + np.uintp(2**32 - 5)) and np.array_equal(n2["stop"], en["stop"] + np.uintp(2**32 - 5))
    assert not n2["n_tar"].any() and not n2["n_neg"].any() and not n2["penalty"].view(np.uint64).any()


def test_reference_on_a_hand_made_index():
    """Three assemblies (records 0 | 1, 2 | 3; the first a target), hashes 7, 7, 9, 7, 9, 5 arriving in record order."""
    rows = np.array([[7, 0 | 0 << 32], [7, 1 | 0 << 32], [9, 0 | 1 << 32], [7, 0 | 2 << 32], [9, 0 | 3 << 32], [5, 1 | 3 << 32]], np.uint64)
    kmers, nodes, ranks = H.reference(rows, 10, [0, 1, 3, 4], [True, False, False])
    assert kmers.tolist() == [(1, 3), (0, 0), (1, 0), (0, 2), (0, 1), (0, 3)]
    assert nodes["hash"].tolist() == [5, 7, 9] and nodes["start"].tolist() == [10, 11, 14] and nodes["stop"].tolist() == [11, 14, 16]
    assert nodes["n_tar"].tolist() == [0, 1, 0] and nodes["n_neg"].tolist() == [1, 1, 2]
    assert nodes["penalty"].tolist() == [np.sqrt(1 + 0.25), np.sqrt(0.25), np.sqrt(1 + 1)]
    assert ranks.tolist() == [1 | 1 << 31, 1 | 1 << 31, 2, 1, 2, 0]


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_every_case_puts_its_runs_where_it_says(name):
    c = H.case(name)
    assert len(c.claims) >= 1 and ("n", c.n) in c.claims
    H.check_claims(c)
    if c.is_targets is not None:
        assert len(c.is_targets) == len(c.record_offsets) - 1 and 0 < sum(c.is_targets) < len(c.is_targets)


def test_the_cases_stand_on_the_bounds_they_name():
    """The geometry, stated here once more and checked against the layouts (not against what the generator says of itself)."""
    assert (H.LANE, H.WORD, H.WAVE_ROW, H.ROW, H.TILE, H.LOOK) == (2, 64, 128, 2048, 8192, 64)
    assert [H.case(f"sizes_{n}").n for n in (0,) + H.SIZES] == [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 8191, 8192,
                                                                8193, 3 * 8192 + 2049]
    for v in H.BOUNDARY_VARIANTS:
        c = H.case(f"boundaries_{v}")
        head, hs, _ = H.check_claims(c)
        assert c.n == 5 * 8192 + 777 and int(hs[0]) == 0 and int(hs[-1]) == 2**64 - 1
        for p in (64, 128, 2048, 8192, 2 * 8192, 4 * 8192):
            got = head[p - 2:p + 2].tolist()                 # (p - 2 belongs to the layout in the first form only)
            assert got[v != "head":] == {"head": [True, False, True, False], "straddle": [True, False, True],
                                         "singles": [True, True, True]}[v], (v, p, got)
            tops = (hs[p - 2:p + 2] >> np.uint64(32)).tolist()
            assert len(set(tops)) == 1, (v, p)              # the heads here differ from their predecessors in the low half only
        # elsewhere: neighbouring runs share the low half and differ in the top
        far = np.flatnonzero(head)[100:140]        # (places 200 .. 700: between the layouts at 128 and at 2048)
        assert ((hs[far] & np.uint64(0xFFFFFFFF)) == (hs[far - 1] & np.uint64(0xFFFFFFFF))).all()
        assert ((hs[far] >> np.uint64(32)) != (hs[far - 1] >> np.uint64(32))).all()
    for name, mirror in (("asm_plain_even", False), ("asm_mirror_odd", True)):
        c = H.case(name)
        head, _, asm = H.check_claims(c)
        assert c.n % 128 == (127 if mirror else 0) and not head[c.n - 300:].any() and len(c.record_offsets) == 10
        n_cross = 0
        for s in range(128, c.n, 128):
            if head[s - 3:s + 4].any() or not (H.TILE <= s - 4 and s + 4 <= 2 * H.TILE + 600):
                continue
            ln = int(np.flatnonzero(head[s:])[0]) + s - int(np.flatnonzero(head[:s + 1])[-1])
            if ln < 300:
                continue
            assert ln <= 700
            change = (asm[s - 3:s + 4] != asm[s - 4:s + 3]).tolist()    # between s - 4 | s - 3, ..., s + 2 | s + 3
            assert change == ([False, False, True, False, True, False, False] if mirror else [False, False, False, True, False, False, False]), (s, change)
            n_cross += 1
        assert n_cross >= 11
        crossed = {s % H.TILE for s in range(128, c.n, 128) if not head[s - 3:s + 4].any() and s < 2 * H.TILE + 600 and s > H.TILE}
        assert {0, H.ROW} <= crossed                         # a row bound and the tile bound lie inside long runs
    for t in (63, 64, 65):
        c = H.case(f"bitmap_tail{t}")
        head, _, asm = H.check_claims(c)
        assert c.n % 128 == t
        nodes = set(zip(np.flatnonzero(head).tolist(), np.flatnonzero(head).tolist()[1:] + [c.n]))
        assert {(192, 256), (384, 512), (703, 704), (895, 897), (1025, 1215), (8128, 8384)} <= nodes
        big = [(a, b) for a, b in nodes if b - a == 1000]
        assert len(big) == 1 and len(set(asm[big[0][0]:big[0][1]].tolist())) == 9
        assert head[c.n - 2] and not head[c.n - 1] and asm[c.n - 1] != asm[c.n - 2]
    head, _, _ = H.check_claims(H.case("headless_tiles"))
    assert head[2 * 8192 - 5] and head[5 * 8192 + 5] and not head[2 * 8192 - 4:5 * 8192 + 5].any()
    for name, h0 in (("all_equal", False), ("all_equal_hash0", True)):
        head, hs, _ = H.check_claims(H.case(name))
        assert int(head.sum()) == 1 and len(head) > 2 * 8192 and (int(hs[0]) == 0) == h0
    head, _, _ = H.check_claims(H.case("all_distinct"))
    assert head.all() and len(head) > 2 * 8192
    c = H.case("long_look_back")
    head, _, _ = H.check_claims(c)
    assert c.n == 130 * 8192 + 1 and head[30 * 8192 + 7] and head[100 * 8192 + 7] and not head[30 * 8192 + 8:100 * 8192 + 7].any()
    assert H.case("base_offset").kmer_base == 2**32 - 5 and H.case("base_offset").n == 20_000
    c = H.case("without_targets")
    assert c.is_targets is None and len(c.record_offsets) == 5
    c = H.case("large")
    head, hs, asm = H.check_claims(c)
    assert c.n == 2**22 + 3 * 8192 + 1 and H.case("second_large").n > 2**22 and H.case("second_large").n != c.n
    one = [(a, b) for a, b in zip(c.starts.tolist(), (c.starts + c.lengths).tolist()) if b - a == 20_000]
    assert len(one) == 1 and len(set(asm[one[0][0]:one[0][1]].tolist())) == 1
    assert H.ROUTE_SIZES["one bucket"] <= 2**14 and 2**15 < H.ROUTE_SIZES["sort"] <= 2**16
    for name in H.CASES:
        if name.startswith("routed_"):
            assert H.case(name).n == H.ROUTE_SIZES["one bucket" if "one_bucket" in name else "sort"]
