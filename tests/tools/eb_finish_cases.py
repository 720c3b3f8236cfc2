"""Key multisets aimed at the finish kernel of the bucket route (csrc/radix.hip: k_eb_finish<PACKED>), on top of eb_cases.py.

The model of what is new in the kernel, restated from its description:
  count_bits(largest)   cb: the bit length of the largest count of real keys in a sub-bucket, at least 1;
  eligible(case)        the packed slot -- (key bits below shift2) << cb | copies in ONE word -- is used iff shift2 + cb <= 63;
  expected_done(case, form)   eb_cases.expected_done, and declined as well when form == "packed" is forced on a call that is
                        not eligible (form: None = the routine chooses, "packed", "plain").
A step of the kernel is CHUNK = 4 x 512 keys, lane t of the workgroup holding positions j0 + i * 512 + t (i = 0 .. 3) of its
sub-bucket.  The two bucket passes in front of the kernel keep the input order inside a sub-bucket when they rank by ballots
(SEQWIN_AMD_RADIX_RANK=ballot) and the whole input is one tile (at most TILE keys); the cases that place keys by position stay below
that size and are run in that mode.  The cases whose claim does not depend on the order say so with `ordered = False`.

Every builder asserts that the case is what its name says; tests/test_edge_finish_cpu.py builds them all without a GPU.
"""
from __future__ import annotations

import numpy as np

import eb_cases as E
from eb_cases import U

LANES = 512               # EB_THREADS
FORMS = (None, "packed", "plain")


def count_bits(largest: int) -> int:
    return max(1, int(largest).bit_length())


def eligible(case) -> bool:
    largest, _ = E.bucket_stats(case.keys, case.key_bits)
    return E.layout(case.key_bits).shift2 + count_bits(largest) <= 63


def chosen_form(case) -> str:
    return "packed" if eligible(case) else "plain"


def expected_done(case, form=None) -> bool:
    return E.expected_done(case) and not (form == "packed" and not eligible(case))


def _case(name, kb, bucket_keys, sent=3, ordered=True, extra=(), **kw):
    """the keys of the case's sub-bucket in the given order, then `extra`, the sentinels last (none of them moves the others)"""
    L = E.layout(kb)
    claims = kw.pop("claims", {})
    claims["ordered"] = ordered
    keys = np.concatenate([np.asarray(bucket_keys, U), np.asarray(extra, U), E._sentinels(L, sent)])
    assert not ordered or len(keys) <= E.TILE
    return E.Case(name, kb, np.ascontiguousarray(keys, U), claims=claims, **kw)


def _one_sub_bucket(case, n):
    L = E.layout(case.key_bits)
    real = E.real_keys(case.keys, case.key_bits)
    ids, counts = np.unique(E.sub_bucket(real, L), return_counts=True)
    assert counts.max() == n and (counts == n).sum() == 1, (case.id, counts)


# ---- step boundaries of the double-buffered loop ------------------------------------------------------------------------------------
STEP_SIZES = (1, 2047, 2048, 2049, 4095, 4096, 4097, 6145)


def steps(kb, size, distinct=700):
    """one sub-bucket of `size` keys, about 700 distinct; 2049, 4097 and 6145 end in a step of ONE key"""
    rng, L = E._rng(f"steps{size}", kb), E.layout(kb)
    pool = E.in_bucket(L, 2, 9, E.distinct_below(rng, min(size, distinct), L.shift2))
    keys = rng.permutation(E._with_copies(rng, pool, size))
    c = _case(f"steps_{size}", kb, keys, sent=5, ordered=False, claims={"largest": size, "distinct": min(size, distinct)})
    _one_sub_bucket(c, size)
    assert len(np.unique(keys)) == min(size, distinct)
    assert (size % E.CHUNK == 1) == (size in (1, 2049, 4097, 6145))
    return c


# ---- batched probes -----------------------------------------------------------------------------------------------------------------
def lane_equal(kb):
    """the four keys of every lane are equal: 512 different keys with period 512, one step"""
    rng, L = E._rng("lane_equal", kb), E.layout(kb)
    k512 = E.in_bucket(L, 1, 7, E.distinct_below(rng, LANES, L.shift2))
    keys = np.tile(k512, 4)
    c = _case("lane_equal", kb, keys, claims={"distinct": LANES})
    assert len(keys) == E.CHUNK and len(np.unique(k512)) == LANES
    assert all(np.array_equal(keys[i * LANES:(i + 1) * LANES], keys[:LANES]) for i in range(4))
    assert all(len(np.unique(keys[w * 64:(w + 1) * 64])) == 64 for w in range(8))   # (no wave merges anything)
    return c


def lane_collide(kb, slots=4096):
    """the four keys of every lane differ and hash to one slot (a different slot for every lane)"""
    rng, L = E._rng("lane_collide", kb), E.layout(kb)
    cand = E.in_bucket(L, 1, 7, E.distinct_below(rng, min(1 << 21, 1 << L.shift2), L.shift2))
    hs = E.hash_slot(cand, slots)
    order = np.argsort(hs, kind="stable")
    cand, hs = cand[order], hs[order]
    first = np.searchsorted(hs, np.arange(slots))
    room = np.diff(np.append(first, len(hs)))
    use = np.flatnonzero(room >= 4)[::max(1, slots // LANES // 2)][:LANES]
    assert len(use) == LANES, (len(use), kb)
    groups = np.stack([cand[first[s]:first[s] + 4] for s in use])          # [lane, i]
    keys = groups.T.reshape(-1).copy()                                     # position i * 512 + lane
    c = _case("lane_collide", kb, keys, slots=slots, claims={"distinct": 4 * LANES})
    assert len(np.unique(keys)) == 4 * LANES <= slots
    for t in (0, 1, 63, 64, 511):
        mine = keys[[i * LANES + t for i in range(4)]]
        assert len(set(E.hash_slot(mine, slots).tolist())) == 1 and len(set(mine.tolist())) == 4
    return c


def chain_one_step(kb, slots=64, n=60, width=2):
    """60 distinct keys whose hashes fall on two slots that wrap round the table's end, all inside the first step"""
    base = E.probe_chain(kb, slots, n, width)
    L = E.layout(kb)
    real = E.real_keys(base.keys, kb)
    pool = np.unique(real)
    rng = E._rng("chain_one_step", kb)
    keys = np.concatenate([rng.permutation(pool), rng.permutation(real)[: 2 * n]])
    c = _case("chain_one_step", kb, keys, slots=slots, ordered=False, claims={"distinct": n})
    at = slots - width // 2
    assert len(pool) == n and len(keys) <= E.CHUNK and ((E.hash_slot(pool, slots) - at) % slots < width).all()
    assert set((E.hash_slot(pool, slots)).tolist()) == {slots - 1, 0}
    assert len(np.unique(E.sub_bucket(keys, L))) == 1
    return c


def hub_and_singles(kb):
    """a hub key that fills whole waves (the wave merge adds 64 copies at once), waves of singles, and waves that mix both"""
    rng, L = E._rng("hub", kb), E.layout(kb)
    below = E.distinct_below(rng, 1 + 900, L.shift2)
    hub, singles = E.in_bucket(L, 1, 2, below[:1])[0], E.in_bucket(L, 1, 2, below[1:])
    rows = np.full((48, 64), hub, U)                   # 3072 keys: a step and a half
    rows[16:24, :] = singles[:512].reshape(8, 64)      # waves of keys that occur once
    rows[24:36, 1] = singles[512:524]                  # the hub leads the wave, one single inside
    rows[36:48, 0] = singles[524:536]                  # a single leads the wave: the hub is not merged there
    keys = rows.reshape(-1)
    c = _case("hub_and_singles", kb, keys, claims={"distinct": 537})
    assert sum(bool((r == hub).all()) for r in rows) >= 16
    uk, cnt = np.unique(keys, return_counts=True)
    assert len(uk) == 537 and (cnt[uk != hub] == 1).all() and cnt[uk == hub][0] == 3072 - 536
    return c


def table_full(kb, slots, over):
    """exactly `slots` distinct keys in ONE step (done), or slots + 1 with the extra one in the same step (declined)"""
    rng, L = E._rng(f"full{slots}{over}", kb), E.layout(kb)
    n = slots + (1 if over else 0)
    assert n <= E.CHUNK
    keys = E.in_bucket(L, 1, 7, E.distinct_below(rng, n, L.shift2))
    c = _case(f"table_{'over' if over else 'full'}_slots{slots}", kb, keys, slots=slots, ordered=False, claims={"distinct": n})
    assert len(np.unique(keys)) == n and len(keys) <= E.CHUNK and E.expected_done(c) == (not over)
    return c


# ---- packed word limits: 62 key bits, shift2 = 45 ------------------------------------------------------------------------------------
def packed_limit(which):
    """the largest sub-bucket holds 2^18 - 1 keys (cb = 18, shift2 + cb = 63: packed) or 2^18 (cb = 19: plain)
    one_key        2^18 - 1 copies of ONE key: the count field ends all ones
    one_key_over   2^18 copies
    corners        2^18 - 1 keys: a hub, the key whose 45 low bits are all ones (once), and a, a ^ 1, a ^ (1 << 44)"""
    kb = 62
    rng, L = E._rng("packed_limit" + which, kb), E.layout(kb)
    assert L.shift2 == 45
    full = (1 << 18) - 1
    hub = int(E.in_bucket(L, 3, 5, [0x0AAAAAAAAAAA & ((1 << 45) - 1)])[0])
    if which == "one_key":
        keys = np.full(full, hub, U)
    elif which == "one_key_over":
        keys = np.full(full + 1, hub, U)
    else:
        ones = int(E.in_bucket(L, 3, 5, [(1 << 45) - 1])[0])
        a = int(E.in_bucket(L, 3, 5, [0x0123456789AB & ((1 << 44) - 2)])[0])
        rest = np.array([ones, a, a, a ^ 1, a ^ (1 << 44), a ^ (1 << 44)], U)
        keys = rng.permutation(np.concatenate([np.full(full - len(rest), hub, U), rest]))
        assert (np.unique(keys) == np.sort(np.array([hub, ones, a, a ^ 1, a ^ (1 << 44)], U))).all()
        assert int(np.sum(keys == U(ones))) == 1 and ones & ((1 << 45) - 1) == (1 << 45) - 1
    c = _case(f"packed_limit_{which}", kb, keys, sent=7, ordered=False, claims={"largest": len(keys)})
    largest, _ = E.bucket_stats(c.keys, kb)
    assert largest == len(keys) and count_bits(largest) == (19 if which == "one_key_over" else 18)
    assert eligible(c) == (which != "one_key_over") and L.shift2 + count_bits(largest) == (64 if which == "one_key_over" else 63)
    return c


def packed_corners_small(kb):
    """the same corner keys with small counts: all low bits set (once), a, a ^ 1, a ^ (1 << (shift2 - 1))"""
    rng, L = E._rng("corners_small", kb), E.layout(kb)
    low = (1 << L.shift2) - 1
    a = 0x0123456789ABCDEF & (low >> 1) & ~1
    lows = np.array([low, a, a, a ^ 1, a ^ 1, a ^ 1, a ^ (1 << (L.shift2 - 1))], U)
    keys = E.in_bucket(L, 2, 2, rng.permutation(lows))
    c = _case("packed_corners_small", kb, keys, ordered=False, claims={"distinct": 4})
    assert len(np.unique(keys)) == 4 and eligible(c)
    return c


# ---- the list of live sub-buckets ----------------------------------------------------------------------------------------------------
def live(kb, which):
    rng, L = E._rng("live" + which, kb), E.layout(kb)
    t1, t2 = E._top(L)
    n_sub = 1 << (L.bits1 + L.bits2)

    def some(d1, d2, n=40, top=False):
        pool = E.in_bucket(L, d1, d2, E.distinct_below(rng, min(n, (1 << L.shift2) - 1), L.shift2, exclude_top=top))
        return E._with_copies(rng, pool, 3 * len(pool))

    if which == "first_only":
        parts, sent, want = [some(0, 0)], 0, [0]
    elif which == "last_with_sentinels":
        parts, sent, want = [some(t1, t2, top=True)], 50, [t1 * E.RADIX + t2]
    elif which == "last_below_sentinels":
        parts, sent, want = [some(t1, t2 - 1)], 50, [t1 * E.RADIX + t2 - 1, t1 * E.RADIX + t2]
    elif which == "one_level1_bucket":
        parts, sent = [some(5 % (1 << L.bits1), d2, 6) for d2 in range(1 << L.bits2)], 0
        want = [(5 % (1 << L.bits1)) * E.RADIX + d2 for d2 in range(1 << L.bits2)]
    elif which == "sentinels_only":
        parts, sent, want = [], 700, [t1 * E.RADIX + t2]
    elif which == "no_sentinels":
        ids = [(1, 3), (1, 4), (2, 0), (t1, t2 - 1)]
        parts, sent, want = [some(a, b) for a, b in ids], 0, [a * E.RADIX + b for a, b in ids]
    else:
        assert which == "alternate" and n_sub >= 2048
        ids = [(2 * i >> L.bits2, 2 * i & ((1 << L.bits2) - 1)) for i in range(1024)]
        parts, sent, want = [some(a, b, 5) for a, b in ids], 0, [a * E.RADIX + b for a, b in ids]
    c = E._finish(rng, f"live_{which}", kb, parts + [E._sentinels(L, sent)], claims={"sentinels": sent, "live": len(want), "ordered": False})
    got = np.unique(E.sub_bucket(c.keys, L))   # (sentinels included: their sub-bucket is launched too)
    assert np.array_equal(got, np.sort(np.array(want, np.int64))), (c.id, got[:8], want[:8])
    if which == "alternate":
        assert len(got) == 1024 and (np.diff(got) >= 2).all() and (got[:512] % 2 == 0).all()
    return c


LIVE_KINDS = ("first_only", "last_with_sentinels", "last_below_sentinels", "one_level1_bucket", "sentinels_only", "no_sentinels", "alternate")


def cases() -> list:
    out = [steps(54, s) for s in STEP_SIZES] + [steps(62, s) for s in (2049, 4096)]
    out += [lane_equal(kb) for kb in (54, 30)] + [lane_collide(54)]
    out += [chain_one_step(kb) for kb in (54, 30)] + [hub_and_singles(kb) for kb in (54, 30)]
    out += [table_full(54, s, over) for s in (64, 1024) for over in (False, True)]
    out += [packed_limit(w) for w in ("one_key", "one_key_over", "corners")]
    out += [packed_corners_small(kb) for kb in (62, 54, 30)]
    out += [live(54, w) for w in LIVE_KINDS] + [live(22, w) for w in ("first_only", "last_below_sentinels", "alternate")]
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


SEQUENCE = [("steps_4097-kb54", "packed"), ("table_full_slots64-kb54", "plain"), ("table_over_slots64-kb54", "packed"),
            ("steps_4097-kb54", "plain"), ("distinct_eq_slots8192-kb54", "packed"), ("packed_limit_one_key_over-kb62", "packed"),
            ("distinct_eq_slots8192-kb54", "plain"), ("table_full_slots64-kb54", "packed"), ("steps_4097-kb54", None),
            ("distinct_eq_slots4096-kb54", "plain"), ("distinct_eq_slots4096-kb54", "packed"), ("steps_4097-kb54", "packed")]
