"""Crafted key multisets for the bucket route of the edge sort (csrc/radix.hip: radix_edge_buckets) and a model of its geometry.

Pure numpy; nothing here is read back from the library.  The model restates, from the description of the route:
  layout(key_bits)   the digit width (9 where ceil(bits / 9) < ceil(bits / 8), else 8), the level-1 digit [shift1, key_bits), the
                     level-2 digit [shift2, shift1) of at most nine bits below it, the finish kernel's bins [bin_shift, shift2) of at
                     most nine bits below that;
  sub_bucket / bin_of / digit1   where a key goes;
  reference(keys, key_bits)      np.unique of the real keys, the exclusive cumulative sum of the counts, the total last;
  expected_done(case)            the route: declined iff there are fewer than two digits, m = 0, `slots` is no power of two in
                                 [64, 8192], the largest count of real keys in a sub-bucket exceeds `cap`, or a sub-bucket holds
                                 more than `slots` distinct real keys.
The sentinel (a record boundary) is 2^key_bits - 1; it is counted in no sub-bucket's size and appears in no output.

Builders place keys by (level-1 digit, level-2 digit, bin, low bits) through compose(), so a case means the same thing at every
geometry; each takes key_bits and asserts that the geometry has the room it needs.  cases() lists every case, digest() pins its
bytes (tests/golden/edge_buckets/cases.json).  Every Case carries `claims`: the properties its name promises, written down from
the builder's intent; tests/test_edge_buckets_cpu.py checks them against the model, so a GPU test's expected route is a fact about
the input.  The sizes below (TILE, CHUNK, RADIX, SLOTS_MIN / SLOTS_MAX) restate constants of radix.hip; the CPU test compares them
with the source text.
"""
from __future__ import annotations

import hashlib
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

TILE = 16 * 1024          # RS_ITEMS x 1024 threads: a tile of the bucket passes
CHUNK = 4 * 512           # 4 x EB_THREADS: what the finish kernel reads per step
RADIX = 512               # EB_RADIX: level-1 / level-2 buckets, bins
SLOTS_MIN, SLOTS_MAX = 64, 8192
HASH_MUL = 0x9E3779B97F4A7C15   # the finish kernel's multiplicative hash: (key * HASH_MUL mod 2^64) >> 40, masked to the table
HASH_SHIFT = 40
DEFAULT_CAP, DEFAULT_SLOTS = 1 << 20, 4096

SWEEP_BITS = tuple(range(10, 63, 2))   # every even key width with two digits or more
DECLINED_BITS = (8, 9)                 # one digit: the routine declines
ODD_BITS = (11, 19)                    # a top digit of three bits (even widths give 2 and 4 .. 9; no width with two digits gives 1)

Layout = namedtuple("Layout", "key_bits digit n_passes shift1 bits1 bits2 shift2 bin_bits bin_shift")
U = np.uint64


def layout(key_bits: int) -> Layout:
    n8, n9 = -(-key_bits // 8), -(-key_bits // 9)
    digit = 9 if n9 < n8 else 8
    n_passes = -(-key_bits // digit)
    shift1 = (n_passes - 1) * digit
    bits1 = key_bits - shift1
    bits2 = min(9, shift1)
    shift2 = shift1 - bits2
    bin_bits = min(9, shift2)
    return Layout(key_bits, digit, n_passes, shift1, bits1, bits2, shift2, bin_bits, shift2 - bin_bits)


def sentinel(key_bits: int) -> int:
    return (1 << key_bits) - 1


def digit1(keys, L: Layout):
    return (np.asarray(keys, U) >> U(L.shift1)).astype(np.int64)


def digit2(keys, L: Layout):
    return ((np.asarray(keys, U) >> U(L.shift2)) & U((1 << L.bits2) - 1)).astype(np.int64)


def sub_bucket(keys, L: Layout):
    return digit1(keys, L) * RADIX + digit2(keys, L)


def bin_of(keys, L: Layout):
    return ((np.asarray(keys, U) >> U(L.bin_shift)) & U((1 << L.bin_bits) - 1)).astype(np.int64)


def hash_slot(keys, slots: int):
    return (((np.asarray(keys, U) * U(HASH_MUL)) >> U(HASH_SHIFT)) & U(slots - 1)).astype(np.int64)


def hist_top(keys, L: Layout):
    """the counts of the level-1 digit as the producer of the keys hands them in: 2^digit entries, sentinels included"""
    return np.bincount(digit1(keys, L), minlength=1 << L.digit).astype(U)


def real_keys(keys, key_bits: int):
    keys = np.asarray(keys, U)
    return keys[keys != U(sentinel(key_bits))]


def reference(keys, key_bits: int):
    """(ukeys u64[n_runs], ucnt u32[n_runs + 1]): distinct real keys ascending, run starts, the number of real keys last"""
    real = real_keys(keys, key_bits)
    uk, counts = np.unique(real, return_counts=True)
    ucnt = np.zeros(len(uk) + 1, np.int64)
    np.cumsum(counts, out=ucnt[1:])
    return uk.astype(U), ucnt.astype(np.uint32)


def bucket_stats(keys, key_bits: int):
    """(largest count of real keys in a sub-bucket, most distinct real keys in a sub-bucket)"""
    L = layout(key_bits)
    real = real_keys(keys, key_bits)
    if len(real) == 0:
        return 0, 0
    largest = int(np.unique(sub_bucket(real, L), return_counts=True)[1].max())
    distinct = int(np.unique(sub_bucket(np.unique(real), L), return_counts=True)[1].max())
    return largest, distinct


def slots_valid(slots: int) -> bool:
    return SLOTS_MIN <= slots <= SLOTS_MAX and slots & (slots - 1) == 0


@dataclass
class Case:
    name: str
    key_bits: int
    keys: np.ndarray
    cap: int = DEFAULT_CAP
    slots: int = DEFAULT_SLOTS
    claims: dict = field(default_factory=dict)

    @property
    def id(self) -> str:
        return f"{self.name}-kb{self.key_bits}"


def expected_done(case: Case) -> bool:
    if layout(case.key_bits).n_passes < 2 or len(case.keys) == 0 or not slots_valid(case.slots):
        return False
    largest, distinct = bucket_stats(case.keys, case.key_bits)
    return largest <= case.cap and distinct <= case.slots


def digest(case: Case) -> str:
    h = hashlib.sha256()
    h.update(f"{case.key_bits} {case.cap} {case.slots} {len(case.keys)}|".encode())
    h.update(np.ascontiguousarray(case.keys, dtype="<u8").tobytes())
    return h.hexdigest()


# ---- placing keys -----------------------------------------------------------------------------------------------------------------
def compose(L: Layout, d1, d2, b=0, low=0):
    """key = d1 << shift1 | d2 << shift2 | bin << bin_shift | low, every field inside its width"""
    d1, d2, b, low = (np.asarray(x, U) for x in (d1, d2, b, low))
    assert (d1 < U(1 << L.bits1)).all() and (d2 < U(1 << L.bits2)).all() and (b < U(1 << L.bin_bits)).all() and (low < U(1 << L.bin_shift)).all()
    return (d1 << U(L.shift1)) | (d2 << U(L.shift2)) | (b << U(L.bin_shift)) | low


def in_bucket(L: Layout, d1, d2, below):
    """keys of sub-bucket (d1, d2) from the shift2 bits below the level-2 digit"""
    below = np.asarray(below, U)
    assert (below < U(1 << L.shift2)).all()
    return compose(L, d1, d2) | below


def distinct_below(rng, n: int, bits: int, exclude_top: bool = False):
    """n distinct values below 2^bits (not the all-ones value if exclude_top), in random order"""
    room = (1 << bits) - (1 if exclude_top else 0)
    assert n <= room, (n, bits)
    if bits <= 22:
        return rng.permutation(room)[:n].astype(U)
    got = np.unique(rng.integers(0, room, 2 * n + 16, dtype=np.uint64))
    assert len(got) >= n
    return rng.permutation(got)[:n].astype(U)


def _top(L):   # the sentinel's sub-bucket
    return (1 << L.bits1) - 1, (1 << L.bits2) - 1


def _sentinels(L, n):
    return np.full(n, sentinel(L.key_bits), U)


def _with_copies(rng, distinct, total):
    """`total` keys drawn from `distinct`, every one of them at least once"""
    assert total >= len(distinct)
    extra = distinct[rng.integers(0, len(distinct), total - len(distinct))]
    return np.concatenate([distinct, extra])


def _finish(rng, name, kb, parts, shuffle=True, **kw):
    keys = np.concatenate([np.asarray(p, U) for p in parts]) if parts else np.zeros(0, U)
    if shuffle and len(keys) > 1:
        keys = rng.permutation(keys)
    return Case(name, kb, np.ascontiguousarray(keys, U), **kw)


def _rng(name, kb):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(f"{name}/{kb}".encode()).digest()[:8], "little"))


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def mixed(kb, n=60000, n_buckets=64, per_bucket=300, sent=600):
    """the generic case of the sweep: about n_buckets sub-buckets (the sentinels' among them) of up to per_bucket distinct keys with
    skewed numbers of copies, and sentinels"""
    rng, L = _rng("mixed", kb), layout(kb)
    S = sentinel(kb)
    if L.n_passes < 2:   # (one digit: nothing to place by, any keys below the sentinel do)
        pool = distinct_below(rng, min(200, S), kb, exclude_top=True)
    else:
        nb = min(n_buckets, 1 << (L.bits1 + L.bits2))
        which = distinct_below(rng, nb - 1, L.bits1 + L.bits2, exclude_top=True)
        which = np.concatenate([which, [U((1 << (L.bits1 + L.bits2)) - 1)]])
        pool = []
        for j, sb in enumerate(which):
            top = j == len(which) - 1
            cnt = min(per_bucket, (1 << L.shift2) - (1 if top else 0))
            pool.append((sb << U(L.shift2)) | distinct_below(rng, cnt, L.shift2, exclude_top=top))
        pool = np.concatenate(pool)
    pool = rng.permutation(pool)
    draw = pool[rng.integers(0, len(pool), n) * rng.integers(0, len(pool), n) // len(pool)]   # (skewed: a few keys with many copies)
    return _finish(rng, "mixed", kb, [pool, draw, _sentinels(L, sent)], claims={"sentinels": sent, "real": n + len(pool)})


def ordered(kb, order):
    base = mixed(kb)
    keys = {"sorted": np.sort(base.keys), "reversed": np.sort(base.keys)[::-1].copy(), "shuffled": base.keys[::-1].copy()}[order]
    return Case(f"mixed_{order}", kb, keys, claims=dict(base.claims, order=order))


L1_SIZES = (TILE, TILE - 1, TILE + 1, 2 * TILE)


def l1_tiles(kb):
    """level-1 buckets of exactly one tile, one key less, one more, and two tiles (digits 0 .. 3), the sentinels in the top digit"""
    rng, L = _rng("l1_tiles", kb), layout(kb)
    assert L.bits1 >= 3
    parts = []
    for d1, size in enumerate(L1_SIZES):
        d2 = rng.integers(0, 1 << L.bits2, 40)
        pool = np.concatenate([in_bucket(L, d1, x, distinct_below(rng, min(50, 1 << L.shift2), L.shift2)) for x in np.unique(d2)])
        parts.append(_with_copies(rng, pool, size))
    return _finish(rng, "l1_tiles", kb, parts + [_sentinels(L, 77)], claims={"l1_sizes": {d: s for d, s in enumerate(L1_SIZES)}, "sentinels": 77})


def m_small(kb, which):
    rng, L = _rng("m_small" + which, kb), layout(kb)
    S = _sentinels(L, 1)
    one = compose(L, 1, 5)[None]
    if which == "1_real":
        parts, m = [one], 1
    elif which == "1_sentinel":
        parts, m = [S], 1
    elif which == "2":
        parts, m = [one, S], 2
    else:
        m = int(which)
        pool = np.concatenate([in_bucket(L, d1, 3, distinct_below(rng, min(20, 1 << L.shift2), L.shift2)) for d1 in range(1 << min(L.bits1, 2))])
        parts = [_with_copies(rng, pool, m - 5), _sentinels(L, 5)]
    return _finish(rng, f"m_{which}", kb, parts, claims={"m": m})


def chunk(kb, size, distinct=700):
    """one sub-bucket of `size` real keys (the finish kernel reads 4 x 512 per step), a few keys around it"""
    rng, L = _rng(f"chunk{size}", kb), layout(kb)
    pool = in_bucket(L, 2, 9, distinct_below(rng, distinct, L.shift2))
    other = in_bucket(L, 2, 10, distinct_below(rng, 30, L.shift2))
    return _finish(rng, f"chunk_{size}", kb, [_with_copies(rng, pool, size), _with_copies(rng, other, 200), _sentinels(L, 9)],
                   claims={"largest": size, "distinct": distinct})


def l1_every_bucket_one_key(kb):
    """every level-1 bucket holds exactly one key (the top one a real key, not a sentinel): one tile-table entry each"""
    rng, L = _rng("l1_every", kb), layout(kb)
    n = 1 << L.bits1
    keys = compose(L, np.arange(n), rng.integers(0, (1 << L.bits2) - 1, n))
    return _finish(rng, "l1_every_bucket_one_key", kb, [keys], claims={"l1_all_ones": n, "sentinels": 0})


def l1_single_bucket(kb, n=50000):
    """all keys in one level-1 bucket (three tiles and a bit), over all of its level-2 digits"""
    rng, L = _rng("l1_single", kb), layout(kb)
    d1 = (1 << L.bits1) - 2 if L.bits1 > 1 else 0
    pool = np.concatenate([in_bucket(L, d1, d2, distinct_below(rng, min(12, 1 << L.shift2), L.shift2)) for d2 in range(1 << L.bits2)])
    return _finish(rng, "l1_single_bucket", kb, [_with_copies(rng, pool, n)], claims={"l1_sizes": {d1: n}, "l1_occupied": 1, "sentinels": 0})


def distinct_keys(kb, slots, over):
    """a sub-bucket of exactly slots (+ 1 if over) distinct keys with one to three copies, smaller ones beside it"""
    rng, L = _rng(f"distinct{slots}{over}", kb), layout(kb)
    n = slots + (1 if over else 0)
    pool = in_bucket(L, 1, 7, distinct_below(rng, n, L.shift2))
    side = in_bucket(L, 1, 8, distinct_below(rng, min(slots - 1, 40), L.shift2))
    return _finish(rng, f"distinct_{'over' if over else 'eq'}_slots{slots}", kb,
                   [_with_copies(rng, pool, 2 * n), _with_copies(rng, side, 100), _sentinels(L, 13)], slots=slots, claims={"distinct": n})


def probe_chain(kb, slots, n, width):
    """n distinct keys of one sub-bucket whose hash falls into `width` neighbouring slots of the table: probe chains of about n"""
    rng, L = _rng(f"probe{slots}", kb), layout(kb)
    assert n < slots
    cand = in_bucket(L, 3, 3, distinct_below(rng, min(1 << 21, 1 << L.shift2), L.shift2))
    at = slots - width // 2   # (the chain wraps round the end of the table)
    hit = cand[((hash_slot(cand, slots) - at) % slots) < width]
    assert len(hit) >= n, (len(hit), n)
    pool = hit[:n]
    return _finish(rng, f"probe_chain_slots{slots}", kb, [_with_copies(rng, pool, 3 * n), _sentinels(L, 3)], slots=slots,
                   claims={"distinct": n, "hash_span": (at % slots, width)})


def one_bin(kb, n=2000):
    """all distinct keys of a sub-bucket in one bin: they differ only below bin_shift, and are ranked by the quadratic loop"""
    rng, L = _rng("one_bin", kb), layout(kb)
    assert L.bin_shift >= 6
    n = min(n, 1 << L.bin_shift)
    b = (1 << L.bin_bits) - 1
    pool = compose(L, 2, 2, b, distinct_below(rng, n, L.bin_shift))
    return _finish(rng, "one_bin", kb, [_with_copies(rng, pool, 3 * n), _sentinels(L, 4)], claims={"distinct": n, "bins": 1})


def all_bins(kb):
    """a sub-bucket with exactly one distinct key in each of its 2^bin_bits bins"""
    rng, L = _rng("all_bins", kb), layout(kb)
    n = 1 << L.bin_bits
    pool = compose(L, 1, 1, np.arange(n), rng.integers(0, 1 << L.bin_shift, n, dtype=np.uint64))
    return _finish(rng, "all_bins", kb, [_with_copies(rng, pool, 4 * n)], claims={"distinct": n, "bins": n, "sentinels": 0})


def differ_bit0(kb, pairs=1500):
    """pairs k, k ^ 1 in many bins of a few sub-buckets"""
    rng, L = _rng("bit0", kb), layout(kb)
    parts = []
    for d2 in (0, 1, (1 << L.bits2) - 1):
        half = distinct_below(rng, min(pairs, 1 << (L.shift2 - 1)), L.shift2 - 1) << U(1)
        even = in_bucket(L, 0, d2, half)
        parts += [even, even | U(1), even[: len(even) // 3]]
    return _finish(rng, "differ_bit0", kb, parts + [_sentinels(L, 11)], claims={"bit0_pairs": True})


def one_key_many(kb, copies=1 << 20):
    """one key 2^20 times, a smaller and a larger key of the same sub-bucket beside it"""
    rng, L = _rng("one_key", kb), layout(kb)
    k = int(in_bucket(L, 4, 4, [1 << (L.shift2 - 1)])[0])
    parts = [np.full(copies, k, U), np.full(3, k - 1, U), np.full(5, k + 1, U), _sentinels(L, 6)]
    return _finish(rng, "one_key_2pow20", kb, parts, cap=1 << 21, claims={"largest": copies + 8, "distinct": 3})


def interleaved(kb, groups=600):
    """waves of 64 keys that open with a key occurring once, the rest copies of a common key (input left in this order)"""
    rng, L = _rng("interleaved", kb), layout(kb)
    below = distinct_below(rng, min(groups + 4, 1 << L.shift2), L.shift2)
    rare, common = in_bucket(L, 1, 2, below[4:]), in_bucket(L, 1, 2, below[:4])
    rows = np.empty((len(rare), 64), U)
    rows[:, 0] = rare
    rows[:, 1:] = common[rng.integers(0, 4, (len(rare), 63))]
    rows[:, 1] = common[0]
    return _finish(rng, "interleaved_copies", kb, [rows.reshape(-1)], shuffle=False, claims={"distinct": len(below), "sentinels": 0})


def all_distinct(kb, n=100000):
    """every key once, spread over sub-buckets of at most 1500 keys"""
    rng, L = _rng("all_distinct", kb), layout(kb)
    per = min(1500, 1 << L.shift2)
    nb = -(-n // per)
    sbs = distinct_below(rng, nb, L.bits1 + L.bits2, exclude_top=True)
    keys = np.concatenate([(sb << U(L.shift2)) | distinct_below(rng, per, L.shift2) for sb in sbs])[:n]
    return _finish(rng, "all_distinct", kb, [keys, _sentinels(L, 50)], claims={"all_distinct": True})


def sentinels(kb, which):
    rng, L = _rng("sent" + which, kb), layout(kb)
    t1, t2 = _top(L)
    room = min(60, (1 << L.shift2) - 1)
    shared = in_bucket(L, t1, t2, distinct_below(rng, room, L.shift2, exclude_top=True))
    other = in_bucket(L, 0, 0, distinct_below(rng, min(60, 1 << L.shift2), L.shift2))
    parts, claims = {
        "shared": ([_with_copies(rng, shared, 500), _with_copies(rng, other, 300), _sentinels(L, 800)], {"sentinels": 800, "real_with_sentinels": 500}),
        "alone": ([_with_copies(rng, other, 700), _sentinels(L, 800)], {"sentinels": 800, "real_with_sentinels": 0}),
        "none": ([_with_copies(rng, shared, 500), _with_copies(rng, other, 300)], {"sentinels": 0, "real_with_sentinels": 500}),
        "only": ([_sentinels(L, 5000)], {"sentinels": 5000, "real": 0}),
    }[which]
    return _finish(rng, f"sentinels_{which}", kb, parts, claims=claims)


def capacity(kb, where, delta, cap=1000):
    """the largest sub-bucket of real keys holds cap + delta keys and is the sentinels' own (where = "sent", with more sentinels than
    cap beside them) or another one ("other", the sentinels' own then holds cap - 50 real keys)"""
    rng, L = _rng(f"cap{where}{delta}", kb), layout(kb)
    t1, t2 = _top(L)
    room = min(100, (1 << L.shift2) - 1)
    with_s = in_bucket(L, t1, t2, distinct_below(rng, room, L.shift2, exclude_top=True))
    other = in_bucket(L, 0, 3, distinct_below(rng, room, L.shift2))
    big = cap + delta
    sizes = (big, cap - 50) if where == "sent" else (cap - 50, big)
    return _finish(rng, f"cap_{where}_{'at' if delta == 0 else 'above' if delta > 0 else 'below'}", kb,
                   [_with_copies(rng, with_s, sizes[0]), _with_copies(rng, other, sizes[1]), _sentinels(L, cap + 500)], cap=cap,
                   claims={"largest": big, "real_with_sentinels": sizes[0], "sentinels": cap + 500})


def bad_slots(kb, slots):
    c = mixed(kb)
    return Case(f"bad_slots{slots}", kb, c.keys, slots=slots, claims={"slots_valid": False})


# ---- the list ---------------------------------------------------------------------------------------------------------------------
def cases() -> list[Case]:
    out = [mixed(kb) for kb in DECLINED_BITS + SWEEP_BITS + ODD_BITS]
    out += [ordered(kb, o) for kb in (22, 54) for o in ("shuffled", "sorted", "reversed")]
    out += [l1_tiles(kb) for kb in (22, 54, 62)]
    out += [m_small(kb, w) for kb in (22, 54) for w in ("1_real", "1_sentinel", "2", "100", str(TILE), str(TILE + 1))]
    out += [chunk(kb, s) for kb in (30, 54) for s in (CHUNK - 1, CHUNK, CHUNK + 1)]
    out += [l1_every_bucket_one_key(kb) for kb in (18, 22, 54, 62)]
    out += [l1_single_bucket(kb) for kb in (22, 54)]
    out += [distinct_keys(kb, 64, False) for kb in (22, 30, 54)] + [distinct_keys(kb, 4096, False) for kb in (30, 54)]
    out += [distinct_keys(kb, 8192, False) for kb in (28, 54, 62)]
    out += [distinct_keys(kb, 64, True) for kb in (22, 54)] + [distinct_keys(kb, 4096, True) for kb in (30,)]
    out += [distinct_keys(kb, 8192, True) for kb in (30, 54, 62)]
    out += [probe_chain(kb, 64, 60, 2) for kb in (30, 54)] + [probe_chain(kb, 1024, 1000, 4) for kb in (54, 62)]
    out += [one_bin(kb) for kb in (30, 54, 62)]
    out += [all_bins(kb) for kb in (22, 30, 54)]
    out += [differ_bit0(kb) for kb in (22, 30, 54)]
    out += [one_key_many(54)]
    out += [interleaved(kb) for kb in (22, 54)]
    out += [all_distinct(kb) for kb in (30, 54)]
    out += [sentinels(kb, w) for kb in (22, 54, 62) for w in ("shared", "alone", "none", "only")]
    out += [capacity(kb, where, d) for kb in (22, 54) for where in ("sent", "other") for d in (0, 1, -1)]
    out += [bad_slots(22, s) for s in (0, 32, 63, 96, 16384)]
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return out


if __name__ == "__main__":   # `python tests/tools/eb_cases.py --pin` rewrites the pinned digests (on purpose only)
    import json
    import sys
    from pathlib import Path

    table = {c.id: digest(c) for c in cases()}
    if "--pin" in sys.argv:
        out = Path(__file__).resolve().parent.parent / "golden" / "edge_buckets" / "cases.json"
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(table, indent=0, sort_keys=True) + "\n")
    for cid, c in ((c.id, c) for c in cases()):
        print(f"{cid:36s} m {len(c.keys):8d} cap {c.cap:8d} slots {c.slots:5d} done {int(expected_done(c))} stats {bucket_stats(c.keys, c.key_bits)}")
