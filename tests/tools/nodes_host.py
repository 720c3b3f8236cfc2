"""The node stage's yardstick and its crafted inputs (plain NumPy; no device, nothing of the library under test).

group_occurrences (csrc/index.hip: the pair sort, k_nodes, an unsort route, k_finish_nodes) takes rows (hash, pos | record << 32)
in (record, pos) order with assembly-major records, and leaves kmers in stable hash order, one node per distinct hash with its
distinct target / non-target assemblies and penalty, and for every row its node with bit 31 set where the node recurs in the row's
assembly.  reference() restates that with argsort / unique; make_rows() builds rows LAYOUT-FIRST: the caller lists the runs of
equal hashes in ascending hash order with the assembly of every occurrence, so the place of every run -- and of every assembly
change inside it -- in the sorted array is known before a row exists, and a case can put them on the bounds of k_nodes:

    lane = 2 occurrences, wave row = 128, bitmap word = 64, row = 2048, tile = 8192, look-back step = 64 tiles.

CASES maps a name to a builder of a Case; a Case carries `claims` about its own layout (a head here, no head there, an assembly
change here ...), stated from those constants, which tests/test_nodes_host_cpu.py checks against the rows themselves.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

LANE, WORD, WAVE_ROW, ROW, TILE, LOOK = 2, 64, 128, 2048, 8192, 64
RANK_REP = np.uint32(0x80000000)
U64_MAX = (1 << 64) - 1

KMER_DTYPE = np.dtype([("pos", np.uint32), ("record_idx", np.uint32)])
NODE_DTYPE = np.dtype([("hash", np.uint64), ("start", np.uintp), ("stop", np.uintp), ("n_tar", np.uint32), ("n_neg", np.uint32),
                       ("penalty", np.float64)])


def split_rows(rows):
    rows = np.asarray(rows, np.uint64).reshape(-1, 2)
    return rows[:, 0], (rows[:, 1] & np.uint64(0xFFFFFFFF)).astype(np.uint32), (rows[:, 1] >> np.uint64(32)).astype(np.uint32)


def reference(rows, kmer_base, record_offsets, is_targets):
    """-> (kmers, nodes, ranks) of a slice build over `rows` ((n, 2) uint64: hash, pos | record << 32)."""
    h, pos, rec = split_rows(rows)
    n = len(h)
    offs = np.asarray(record_offsets, np.int64)
    n_asm = len(offs) - 1
    order = np.argsort(h, kind="stable")
    kmers = np.empty(n, KMER_DTYPE)
    kmers["pos"], kmers["record_idx"] = pos[order], rec[order]
    uh, start, cnt = np.unique(h[order], return_index=True, return_counts=True)
    nn = len(uh)
    nodes = np.zeros(nn, NODE_DTYPE)
    nodes["hash"], nodes["start"], nodes["stop"] = uh, start, start + cnt
    node_sorted = np.repeat(np.arange(nn, dtype=np.int64), cnt)
    asm_sorted = np.searchsorted(offs, rec[order].astype(np.int64), side="right") - 1
    assert n == 0 or (asm_sorted.min() >= 0 and asm_sorted.max() < n_asm)
    # (node, assembly) pairs: how many distinct ones a node has of either kind, and which of them hold more than one row
    pair, pair_inv, pair_cnt = np.unique(node_sorted * n_asm + asm_sorted, return_inverse=True, return_counts=True)
    if is_targets is not None:
        tar = np.asarray(is_targets, np.bool_)
        assert len(tar) == n_asm
        pt = tar[pair % n_asm]
        nodes["n_tar"] = np.bincount(pair[pt] // n_asm, minlength=nn)[:nn]
        nodes["n_neg"] = np.bincount(pair[~pt] // n_asm, minlength=nn)[:nn]
        if nn:
            import oracle   # the committed C restatement of get_penalty: the bit-exact yardstick of the penalty
            pen = nodes.copy()
            pen["n_tar"] = pen["n_neg"] = 0
            oracle.get_penalty(kmers, pen, np.asarray(record_offsets, np.uint32), tar)
            assert np.array_equal(pen["n_tar"], nodes["n_tar"]) and np.array_equal(pen["n_neg"], nodes["n_neg"])
            nodes["penalty"] = pen["penalty"]
    nodes["start"] += np.uintp(kmer_base)
    nodes["stop"] += np.uintp(kmer_base)
    ranks = np.empty(n, np.uint32)
    word = node_sorted.astype(np.uint32)
    word[pair_cnt[pair_inv.ravel()] > 1] |= RANK_REP
    ranks[order] = word
    return kmers, nodes, ranks


def spread_hashes(n_runs, low_only=(), seed=0, first_zero=True, last_max=True):
    """Ascending distinct hashes, one per run.  Run i in `low_only` shares the top 32 bits of run i - 1 and differs in the low half
    only; every other run keeps its predecessor's low half and differs in the top (random steps that spread the tops over the whole
    32-bit range, so that the sort's passes see every digit).  first_zero / last_max: the hashes 0 and 2^64 - 1."""
    rng = np.random.default_rng(seed)
    lo = np.zeros(n_runs, bool)
    lo[np.asarray(list(low_only), np.int64)] = True
    if n_runs:
        lo[0] = False
    room = max(1, (2**32 - 2) // max(n_runs, 1))
    step = rng.integers(1, room + 1, n_runs, dtype=np.uint64)
    step[lo] = 0
    if n_runs and first_zero:
        step[0] = 0
    top = np.cumsum(step, dtype=np.uint64)
    low = np.cumsum(lo, dtype=np.uint64) + np.uint64(0 if first_zero else 0x9E3779B9)
    assert n_runs == 0 or (int(top[-1]) < 2**32 - 1 and int(low[-1]) < 2**32)
    h = (top << np.uint64(32)) | low
    if n_runs > 1 and last_max:
        h[-1] = np.uint64(U64_MAX)
    return h


@dataclass
class Case:
    rows: np.ndarray            # (n, 2) uint64 in arrival = (record, pos) order
    record_offsets: np.ndarray  # uint32, assemblies + 1
    starts: np.ndarray          # expected sorted place of every run (int64, ascending)
    lengths: np.ndarray
    asm_sorted: np.ndarray      # expected assembly of every sorted place
    is_targets: object = None
    kmer_base: int = 0
    claims: list = field(default_factory=list)

    @property
    def n(self):
        return len(self.rows)


def make_rows(runs, assemblies, seed, hashes=None, low_only=()):
    """runs: [(length, assemblies of its occurrences), ...] in ascending hash order -- or (lengths, assemblies of all occurrences
    run after run) as two arrays.  A run's assemblies are taken in ascending order (its occurrences arrive assembly by assembly).
    Rows arrive by (assembly, shuffled within the assembly); an assembly owns one or two consecutive records, the first taking the
    first part of its rows; pos counts up within a record.  -> Case (rows, record_offsets, the sorted place of every run ...)."""
    if isinstance(runs, tuple) and len(runs) == 2 and isinstance(runs[0], np.ndarray):
        lengths, asm_flat = np.asarray(runs[0], np.int64), np.asarray(runs[1], np.int64)
    else:
        lengths = np.array([r[0] for r in runs], np.int64)
        asm_flat = (np.concatenate([np.broadcast_to(np.asarray(r[1], np.int64), (r[0],)) for r in runs]) if len(runs)
                    else np.zeros(0, np.int64))
    n_runs, n = len(lengths), int(lengths.sum())
    assert len(asm_flat) == n and (lengths > 0).all() and (n == 0 or (0 <= asm_flat.min() and asm_flat.max() < assemblies))
    rng = np.random.default_rng(seed)
    starts = np.cumsum(lengths) - lengths
    run_sorted = np.repeat(np.arange(n_runs, dtype=np.int64), lengths)
    asm_sorted = asm_flat[np.lexsort((asm_flat, run_sorted))]
    if hashes is None:
        hashes = spread_hashes(n_runs, low_only, seed)
    hashes = np.asarray(hashes, np.uint64)
    assert len(hashes) == n_runs and (n_runs < 2 or (hashes[1:] > hashes[:-1]).all())
    # arrival: a shuffle of the sorted places, then (stably) by assembly
    perm = rng.permutation(n)
    arrival = perm[np.argsort(asm_sorted[perm], kind="stable")]
    asm_arr = asm_sorted[arrival]
    per_asm = np.bincount(asm_arr, minlength=assemblies)
    n_rec = 1 + (rng.integers(0, 2, assemblies) if assemblies > 1 else np.zeros(1, np.int64))   # one or two records each
    if assemblies > 1:
        n_rec[0], n_rec[1] = 1, 2                                                                # (both kinds in every case)
    record_offsets = np.concatenate([[0], np.cumsum(n_rec)]).astype(np.uint32)
    first = np.where(n_rec == 2, rng.integers(0, per_asm + 1), per_asm)      # rows of an assembly's first record: 0 .. all
    per_rec = np.zeros(int(record_offsets[-1]), np.int64)
    per_rec[record_offsets[:-1]] = first
    two = np.flatnonzero(n_rec == 2)
    per_rec[record_offsets[:-1][two] + 1] = (per_asm - first)[two]
    rec_arr = np.repeat(np.arange(len(per_rec), dtype=np.int64), per_rec)
    pos_arr = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(per_rec) - per_rec, per_rec)
    rows = np.empty((n, 2), np.uint64)
    rows[:, 0] = hashes[run_sorted[arrival]]
    rows[:, 1] = pos_arr.astype(np.uint64) | (rec_arr.astype(np.uint64) << np.uint64(32))
    return Case(rows, record_offsets, starts, lengths, asm_sorted)


class Layout:
    """Runs appended in ascending hash order; `at` is the sorted place of the next one."""

    def __init__(self, assemblies, seed):
        self.assemblies, self.seed = assemblies, seed
        self.rng = np.random.default_rng(seed ^ 0x5EED)
        self.len, self.asm, self.low_only, self.claims = [], [], [], []
        self.at, self.n_runs = 0, 0

    def run(self, length, asms=None, low_only=False):
        """One run; asms: one assembly, a list of `length` assemblies, or None (random over all).  -> its sorted place."""
        if asms is None:
            asms = self.rng.integers(0, self.assemblies, length)
        a = np.sort(np.broadcast_to(np.asarray(asms, np.int64), (length,)))
        if low_only:
            self.low_only.append(self.n_runs)
        self.len.append(np.array([length], np.int64))
        self.asm.append(a)
        start = self.at
        self.at += length
        self.n_runs += 1
        self.claims.append(("node", start, start + length))
        return start

    def pad(self, total, longest=5):
        """Random runs of 1 .. longest occurrences, `total` occurrences in all."""
        if total <= 0:
            assert total == 0, total
            return
        ln = self.rng.integers(1, longest + 1, total)
        cut = int(np.searchsorted(np.cumsum(ln), total, side="left")) + 1
        ln = ln[:cut].astype(np.int64)
        ln[-1] -= int(ln.sum()) - total
        assert ln[-1] > 0 and int(ln.sum()) == total
        self.len.append(ln)
        self.asm.append(self.rng.integers(0, self.assemblies, total))
        self.at += total
        self.n_runs += len(ln)

    def pad_to(self, place, longest=5):
        assert place >= self.at, (place, self.at)
        self.pad(place - self.at, longest)

    def build(self, is_targets="half", kmer_base=0, hashes=None, **hash_args):
        lengths = np.concatenate(self.len) if self.len else np.zeros(0, np.int64)
        asm = np.concatenate(self.asm) if self.asm else np.zeros(0, np.int64)
        if hashes is None:
            hashes = spread_hashes(len(lengths), self.low_only, self.seed, **hash_args)
        c = make_rows((lengths, asm), self.assemblies, self.seed, hashes=hashes)
        if isinstance(is_targets, str):      # every second assembly a target (an odd number leaves one more target)
            is_targets = [a % 2 == 0 for a in range(self.assemblies)]
        c.is_targets, c.kmer_base = is_targets, kmer_base
        c.claims = self.claims + [("n", self.at)]
        return c


# ---- the cases ------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 8191, 8192, 8193, 3 * TILE + 2049)
BOUNDARIES = (64, 128, 2048, 8192, 2 * 8192, 4 * 8192)
BOUNDARY_VARIANTS = ("head", "straddle", "singles")


def sizes(n):
    """Random runs of 1 .. 5 occurrences over 6 assemblies (3 targets)."""
    lay = Layout(6, 1000 + n)
    lay.pad(n)
    return lay.build(first_zero=False, last_max=False)


def _boundary(lay, p, variant):
    """variant "head": a run [p - 2, p) ends at p - 1 and a run starts at p; "straddle": the run [p - 1, p + 1); "singles":
    one-occurrence nodes at p - 1 and at p.  Every head placed here differs from its predecessor in the low half only."""
    if variant == "head":
        lay.pad_to(p - 2)
        lay.run(2, [0, 1], low_only=True)
        lay.run(3, [1, 1, 4], low_only=True)
        lay.claims += [("head", p), ("nohead", p - 1), ("low_only", p)]
    elif variant == "straddle":
        lay.pad_to(p - 1)
        lay.run(2, [2, 2], low_only=True)
        lay.run(1, 2, low_only=True)
        lay.claims += [("head", p - 1), ("nohead", p), ("head", p + 1), ("low_only", p - 1), ("low_only", p + 1)]
    else:
        lay.pad_to(p - 1)
        lay.run(1, 3, low_only=True)
        lay.run(1, 3, low_only=True)
        lay.run(1, 5, low_only=True)
        lay.claims += [("head", p - 1), ("head", p), ("head", p + 1), ("low_only", p), ("low_only", p + 1)]


def run_boundaries(variant, n=5 * TILE + 777):
    """The three layouts around every p of BOUNDARIES that fits into n (the one-bucket route holds 2^14 rows: p <= 8192 there)."""
    lay = Layout(6, 2000 + BOUNDARY_VARIANTS.index(variant) + n)
    ps = [p for p in BOUNDARIES if p + 8 <= n]
    assert len(ps) >= 4
    lay.run(1, 0)                                           # (the hash 0 is a node of its own)
    for p in ps:
        _boundary(lay, p, variant)
    lay.pad_to(n - 1)
    lay.run(1, 5)                                           # (and 2^64 - 1)
    return lay.build()


def _long_run(lay, start, crossings, mirror, tail=0):
    """A run from `start` that crosses `crossings` multiples of 128 (<= 4 in mirror form: two fresh assemblies each, of 9) and goes
    on for `tail` occurrences (>= 4) behind the last one.  Plain form: the assembly changes exactly between s - 1 and s at every
    crossed multiple s of 128 -- the place where lane 0 reloads its predecessor and lane 63 its successor.  Mirror form: s - 1 and s
    are of ONE assembly, s - 2 and s + 1 of two others: the pair (s - 1, s) is all that its assembly has in the run."""
    lay.pad_to(start)
    first = -(-(start + 4) // WAVE_ROW) * WAVE_ROW          # first crossed multiple: at least 4 occurrences in front of it
    cross = [first + i * WAVE_ROW for i in range(crossings)]
    stop = cross[-1] + max(tail, 4)
    asm = np.empty(stop - start, np.int64)
    if mirror:
        assert crossings <= 4
        a, at = 0, start
        for s in cross:
            asm[at - start:s - 1 - start] = a
            asm[s - 1 - start:s + 1 - start] = a + 1
            a, at = a + 2, s + 1
        asm[at - start:] = a
    else:
        assert crossings <= 8
        for i, s in enumerate([start] + cross):
            asm[s - start:] = i
    lay.run(stop - start, asm)
    for s in cross:
        if mirror:
            lay.claims += [("asm_same", s), ("asm_change", s - 1), ("asm_change", s + 1)]
            lay.claims += [("asm_same", s + d) for d in (-2, 2, 3)]
        else:
            lay.claims += [("asm_change", s)] + [("asm_same", s + d) for d in (-3, -2, -1, 1, 2, 3)]
    return stop


def _asm_runs(lay, start, mirror):
    """Long runs (300 .. 700 occurrences) from `start` (a multiple of the tile): inside a tile, across a row and across a tile."""
    assert start % TILE == 0
    at = _long_run(lay, start + 100, 3, mirror, tail=50)                          # 128-boundaries inside a row
    at = _long_run(lay, start + ROW - 300, 4, mirror, tail=100)                   # across the row boundary
    at = _long_run(lay, start + TILE - 200, 4 if mirror else 5, mirror, tail=60)  # across the tile boundary
    lay.claims += [("inside", start + ROW), ("inside", start + TILE)]
    return at


def asm_changes(mirror):
    """9 assemblies.  The last run ends at n - 1: n = 128 m (plain form: lane 63 holds the last two occurrences, s + 2 == n) or
    n = 128 m + 127 (mirror form: lane 63 holds one occurrence, s + 1 == n)."""
    lay = Layout(9, 3000 + int(mirror))
    _asm_runs(lay, TILE, mirror)
    n = 3 * TILE + (WAVE_ROW - 1 if mirror else 0)
    assert lay.at + 400 < n
    lay.pad_to(n - 330)
    # the last occurrence alone in its assembly: nothing before it (odd n) or behind it (even n) may mark it
    lay.run(330, [2] * 200 + [6] * 129 + [7] if mirror else [1] * 300 + [4] * 29 + [8])
    lay.claims += [("node", n - 330, n), ("asm_change", n - 1), ("asm_same", n - 2)]
    return lay.build()


BITMAP_TAILS = (63, 64, 65)


def bitmap_words(tail):
    """Nodes on bitmap word bounds -- [64 a, 64 b), [64 a + 63, 64 a + 64), [64 a + 63, 64 a + 65), [64 a + 1, 64 (a + 3) - 1) --, a
    node of 1000 occurrences of 9 assemblies, and n mod 128 = tail: the last wave row writes one word, one word exactly, or two."""
    lay = Layout(9, 4000 + tail)
    for a, b in ((3, 4), (6, 8)):                            # [64 a, 64 b): one word, two
        lay.pad_to(WORD * a)
        lay.run(WORD * (b - a))
    lay.pad_to(WORD * 10 + 63)
    lay.run(1, 7)                                            # [64 a + 63, 64 a + 64)
    lay.pad_to(WORD * 13 + 63)
    lay.run(2, [3, 8])                                       # [64 a + 63, 64 a + 65)
    lay.pad_to(WORD * 16 + 1)
    lay.run(WORD * 3 - 2)                                    # [64 a + 1, 64 (a + 3) - 1)
    lay.pad_to(WORD * 40 + 17)
    lay.run(1000)
    lay.pad_to(WORD * 127)
    lay.run(WORD * 4)                                        # four words, across the tile bound at 64 * 128
    n = TILE + 5 * WAVE_ROW + tail
    lay.pad_to(n - 3)
    lay.run(1, 0)
    lay.run(2, [4, 5])                                       # first-of-assembly bits in the last two places
    return lay.build()


def headless_tiles():
    """One node of three whole tiles and 5 occurrences on either side: the tiles inside it publish no head."""
    lay = Layout(9, 5000)
    lay.pad_to(2 * TILE - 5)
    lay.run(3 * TILE + 10)
    lay.pad_to(6 * TILE + 300)
    c = lay.build()
    c.claims += [("nohead_range", 2 * TILE, 5 * TILE)]
    return c


def all_equal(zero):
    lay = Layout(9, 5100 + int(zero))
    lay.run(2 * TILE + 100)
    return lay.build(hashes=np.array([0 if zero else 0xC0FFEE0123456789], np.uint64))


def all_distinct():
    n = 20_001
    lay = Layout(6, 5200)
    lay.pad(n, longest=1)
    c = lay.build()
    c.claims += [("nodes", n)]
    return c


def long_look_back():
    """130 tiles and one occurrence; a node of 70 tiles in the middle: the walk of the tile behind it passes more than 64 tiles
    without a head, the last tile walks three steps and holds one occurrence."""
    lay = Layout(9, 5300)
    lay.pad_to(30 * TILE + 7)
    lay.run(70 * TILE)
    lay.pad_to(130 * TILE + 1)
    c = lay.build()
    c.claims += [("nohead_range", 31 * TILE, 100 * TILE)]
    return c


def base_offset():
    lay = Layout(6, 5400)
    lay.pad(20_000)
    return lay.build(kmer_base=2**32 - 5)


def without_targets():
    lay = Layout(4, 5500)
    lay.pad(3000)
    lay.run(300, [0] * 100 + [2] * 199 + [3])
    lay.pad(1000)
    return lay.build(is_targets=None)


# the two routes above 2^22 rows share one input: every boundary layout (the second and third a multiple of 64 tiles further on, so
# p keeps its alignment), both forms of the assembly changes, a node of 20 000 occurrences of one assembly (whole tiles of marked
# words in one digit of the scatter), short runs everywhere else; the last tile holds one occurrence
LARGE_N = (1 << 22) + 3 * TILE + 1
SECOND_N = (1 << 22) + 5 * TILE + 2049                       # ("twice in a row": another size on the same routes)


def large():
    lay = Layout(9, 6000)
    lay.run(1, 0)
    for v, variant in enumerate(BOUNDARY_VARIANTS):
        for p in BOUNDARIES:
            _boundary(lay, p + v * LOOK * TILE, variant)
    _asm_runs(lay, 200 * TILE, False)
    _asm_runs(lay, 300 * TILE, True)
    lay.pad_to(400 * TILE + 1000)
    lay.run(20_000, 3)
    lay.pad_to(LARGE_N - 1)
    lay.run(1, 5)
    return lay.build()


def second_large():
    lay = Layout(6, 6100)
    lay.pad(SECOND_N)
    return lay.build()


def routed(kind, variant, n):
    """The run-boundary (variant: one of BOUNDARY_VARIANTS) or assembly-change (variant: mirror or not) case at the size a route
    needs: the same layout, more short runs behind it."""
    if kind == "boundaries":
        return run_boundaries(variant, n)
    lay = Layout(9, 7000 + int(variant) + n)
    if n >= 3 * TILE:
        _asm_runs(lay, TILE, variant)
    else:                                                    # 2^14 rows: the runs of the first row bound and of the tile bound
        _long_run(lay, 100, 3, variant, tail=50)
        _long_run(lay, ROW - 300, 4, variant, tail=100)
        _long_run(lay, TILE - 200, 4, variant, tail=60)
        lay.claims += [("inside", ROW), ("inside", TILE)]
    lay.pad_to(n)
    return lay.build()


CASES = {}
for _n in (0,) + SIZES:
    CASES[f"sizes_{_n}"] = (sizes, (_n,))
for _v in BOUNDARY_VARIANTS:
    CASES[f"boundaries_{_v}"] = (run_boundaries, (_v,))
CASES["asm_plain_even"] = (asm_changes, (False,))
CASES["asm_mirror_odd"] = (asm_changes, (True,))
for _t in BITMAP_TAILS:
    CASES[f"bitmap_tail{_t}"] = (bitmap_words, (_t,))
CASES.update(headless_tiles=(headless_tiles, ()), all_equal=(all_equal, (False,)), all_equal_hash0=(all_equal, (True,)),
             all_distinct=(all_distinct, ()), long_look_back=(long_look_back, ()), base_offset=(base_offset, ()),
             without_targets=(without_targets, ()), large=(large, ()), second_large=(second_large, ()))
ROUTE_SIZES = {"one bucket": 1 << 14, "sort": 3 * (1 << 14) + 777}
for _r, _n in ROUTE_SIZES.items():
    for _v in BOUNDARY_VARIANTS:
        CASES[f"routed_{_r.replace(' ', '_')}_boundaries_{_v}"] = (routed, ("boundaries", _v, _n))
    for _m in (False, True):
        CASES[f"routed_{_r.replace(' ', '_')}_asm_{'mirror' if _m else 'plain'}"] = (routed, ("asm", _m, _n))
_BUILT = {}


def case(name):
    """The Case of a name of CASES (built once per process; treat it as read-only)."""
    if name not in _BUILT:
        f, args = CASES[name]
        _BUILT[name] = f(*args)
        _BUILT[name].rows.setflags(write=False)
    return _BUILT[name]


def check_claims(c):
    """A case's claims against its own rows (no reference(): the sorted hashes and assemblies only)."""
    h, pos, rec = split_rows(c.rows)
    n = len(h)
    # the contract of the entry: rows in (record, pos) order, pos counting up from 0 within a record
    key = (rec.astype(np.int64) << 32) | pos
    assert (np.diff(key) > 0).all()
    new_rec = np.concatenate([[True], rec[1:] != rec[:-1]]) if n else np.zeros(0, bool)
    assert (pos[new_rec] == 0).all() and (np.diff(pos)[~new_rec[1:]] == 1).all()
    assert n == 0 or int(rec.max()) < int(c.record_offsets[-1])
    per_asm = np.diff(c.record_offsets.astype(np.int64))
    assert ((per_asm == 1) | (per_asm == 2)).all()
    order = np.argsort(h, kind="stable")
    hs = h[order]
    asm = np.searchsorted(c.record_offsets.astype(np.int64), rec[order].astype(np.int64), side="right") - 1
    head = np.concatenate([[True], hs[1:] != hs[:-1]]) if n else np.zeros(0, bool)
    assert np.array_equal(np.flatnonzero(head), c.starts) and np.array_equal(asm, c.asm_sorted)
    assert int(c.lengths.sum()) == n
    for cl in c.claims:
        kind, a = cl[0], cl[1]
        if kind == "n":
            assert n == a, cl
        elif kind == "nodes":
            assert int(head.sum()) == a, cl
        elif kind == "head":
            assert head[a], cl
        elif kind == "nohead":
            assert not head[a], cl
        elif kind == "low_only":      # a head that differs from its predecessor in the low half only
            assert head[a] and hs[a] >> np.uint64(32) == hs[a - 1] >> np.uint64(32), cl
        elif kind == "node":
            assert head[a] and (cl[2] == n or head[cl[2]]) and not head[a + 1:cl[2]].any(), cl
        elif kind == "nohead_range":
            assert not head[a:cl[2]].any(), cl
        elif kind == "inside":        # no head: the place lies inside a run
            assert not head[a], cl
        elif kind == "asm_change":    # inside a run, the assembly changes between a - 1 and a
            assert not head[a] and asm[a] != asm[a - 1], cl
        elif kind == "asm_same":
            assert not head[a] and asm[a] == asm[a - 1], cl
        else:
            raise AssertionError(cl)
    return head, hs, asm
