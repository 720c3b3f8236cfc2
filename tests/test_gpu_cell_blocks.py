"""GPU: the block export every cell table of the query layer goes through (csrc/device.hpp: export_cells; seqwin_amd/device.py:
_cell_block) at its edges, for every accessor of BestHits (with align, loci and local), OligoHits (Hamming, edit and thermo form)
and Screen: every sub-block [r0, r1) x [c0, c1) of a 2 x 3 table equals the NumPy slice of the full table, the empty ones included;
an empty block leaves the caller's array as it was; a bound one past the table and an accessor of a part the result was made
without are ValueErrors."""
import ctypes
import itertools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NQ, NA, K = 2, 3, 11
ROWS = [(a, b) for a in range(NQ + 1) for b in range(a, NQ + 1)]
COLS = [(a, b) for a in range(NA + 1) for b in range(a, NA + 1)]
COMP = bytes.maketrans(b"ACGT", b"TGCA")

HITS = ("seeds", "record", "strand", "end", "dist")
ALIGN = ("start", "nident", "mismatch", "gaps")
LOCAL = ("score", "qstart", "qend", "sstart", "send", "local_nident", "local_mismatch", "local_gapopen", "local_gaps")
LOCI = ("n_loci", "sum_nident")
OLIGO = ("n_sites", "best_dist", "best_record", "best_pos", "best_strand", "best_end", "best_mismatch", "best_gaps")
THERMO = ("n_stable", "stable_dg", "stable_dh", "stable_ds", "stable_record", "stable_pos", "stable_strand", "stable_mm")


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _mutate(rng, seq, n):
    s = bytearray(seq)
    for i in rng.sample(range(len(s)), n):
        s[i] = ord("ACGT"["ACGT".index(chr(s[i])) ^ rng.randrange(1, 4)])
    return bytes(s)


class World:
    """the batch and one result of each kind, made once"""

    def __init__(self, d):
        from seqwin_amd.device import Batch, set_device
        from seqwin_amd.oligos import santalucia98
        set_device(0)
        rng = random.Random(77)
        R = _rand(rng, 500)
        queries = [R[100:130], R[300:330]]
        asms = [[R],
                [_mutate(rng, R[:250], 6), _mutate(rng, R[250:], 6)],                       # near copies: other counts, other distances
                [_rand(rng, 200) + R[290:340].translate(COMP)[::-1] + _rand(rng, 100)]]     # query 1 alone, on the other strand
        paths = []
        for i, recs in enumerate(asms):
            p = d / f"a{i}.fa"
            with open(p, "wb") as f:
                for j, r in enumerate(recs):
                    f.write(b">a%d_r%d\n" % (i, j) + r + b"\n")
            paths.append(p)
        self.batch = b = Batch.from_fasta(paths, n_cpu=2)
        self.full = b.best_hits(queries, K, align=True, loci=True, local=True)
        self.bare = b.best_hits(queries, K)
        self.hamming = b.oligo_hits(queries, 2)
        self.edit = b.oligo_hits(queries, max_edits=1)
        self.thermo = b.oligo_hits(queries, 2, thermo=santalucia98())
        self.screen = b.screen(queries, K)
        self.all = (self.full, self.bare, self.hamming, self.edit, self.thermo, self.screen)
        for x in self.all:
            assert x.sizes()[:2] == (NQ, NA)

    def close(self):
        for x in self.all + (self.batch,):
            x.close()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("cellblocks"))
    yield w
    w.close()


def _accessors(w):
    """(label, bound method) of every block accessor of every result"""
    out = [(f"best_hits.{n}", getattr(w.full, n)) for n in HITS + ALIGN + LOCAL + LOCI]
    out += [(f"hamming.{n}", getattr(w.hamming, n)) for n in OLIGO + ("best_mm",)]
    out += [(f"edit.{n}", getattr(w.edit, n)) for n in OLIGO]
    out += [(f"thermo.{n}", getattr(w.thermo, n)) for n in OLIGO + ("best_mm",) + THERMO]
    return out + [("screen.counts", w.screen.counts)]


def test_results_are_not_blank(world):
    """the tables the slices are taken from hold different cells, so that a block from the wrong place is seen"""
    for table in (world.full.seeds(), world.full.n_loci(), world.full.score(), world.hamming.n_sites(), world.edit.n_sites(), world.thermo.n_stable(),
                  world.thermo.stable_dg(), world.screen.counts()):
        assert table.shape == (NQ, NA) and len(np.unique(table)) > 1


def test_every_sub_block_is_the_slice_of_the_full_table(world):
    for label, get in _accessors(world):
        whole = get()
        assert whole.shape == (NQ, NA), label
        for (r0, r1), (c0, c1) in itertools.product(ROWS, COLS):
            got = get((r0, r1), (c0, c1))
            assert got.dtype == whole.dtype and got.shape == (r1 - r0, c1 - c0), (label, r0, r1, c0, c1)
            assert np.array_equal(got, whole[r0:r1, c0:c1]), (label, r0, r1, c0, c1)
        assert np.array_equal(get(slice(1, None), range(1, 3)), whole[1:, 1:3]), label


def test_a_bound_past_the_table_is_a_value_error(world):
    for label, get in _accessors(world):
        for rows, cols in (((0, NQ + 1), None), ((NQ + 1, NQ + 1), None), (None, (0, NA + 1)), (None, (NA + 1, NA + 1)), ((1, 0), None), (None, (2, 1))):
            with pytest.raises(ValueError, match="lie outside"):
                get(rows, cols)


def test_a_part_the_result_was_made_without_is_a_value_error(world):
    for n in ALIGN + LOCAL + LOCI:
        with pytest.raises(ValueError, match="made without"):
            getattr(world.bare, n)()
    for o in (world.hamming, world.edit):
        for n in THERMO:
            with pytest.raises(ValueError, match="made without"):
                getattr(o, n)((0, 1), (0, 1))


def test_the_library_refuses_the_same_and_an_empty_block_touches_nothing(world):
    """straight at the C ABI, where no Python guard stands in front: the "made without" errors, and an empty block -- valid with a
    NULL array -- that leaves the caller's array as it was"""
    from seqwin_amd._lib import check, lib
    u = ctypes.c_uint64
    buf = np.full(NQ * NA, 0xA5A5A5A5, np.uint32)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)
    with_field = [(lib.sw_hits_block, world.full), (lib.sw_hits_align_block, world.full), (lib.sw_hits_local_block, world.full),
                  (lib.sw_hits_loci_block, world.full), (lib.sw_oligos_block, world.hamming), (lib.sw_oligos_block, world.edit),
                  (lib.sw_oligos_thermo_block, world.thermo)]
    for (r0, r1), (c0, c1) in itertools.product(ROWS, COLS):
        if r0 < r1 and c0 < c1:
            continue
        for fn, obj in with_field:
            check(fn(obj._h, u(0), u(r0), u(r1), u(c0), u(c1), ptr))
            check(fn(obj._h, u(0), u(r0), u(r1), u(c0), u(c1), None))
        check(lib.sw_screen_counts(world.screen._h, u(r0), u(r1), u(c0), u(c1), ptr))
        check(lib.sw_screen_counts(world.screen._h, u(r0), u(r1), u(c0), u(c1), None))
    assert np.all(buf == 0xA5A5A5A5)
    # the order of the checks: the field before the range, the range before the NULL array -- which only a block with cells needs
    calls = [(lambda *a, fn=fn, h=obj._h: fn(h, *a), 99) for fn, obj in with_field]
    calls.append((lambda f, *a: lib.sw_screen_counts(world.screen._h, *a), None))
    for call, bad_field in calls:
        for f in (0, 1):
            with pytest.raises(ValueError, match="a NULL handle or array"):
                check(call(u(f), u(0), u(NQ), u(1), u(NA), None))
        with pytest.raises(ValueError, match="lie outside"):
            check(call(u(0), u(0), u(NQ + 1), u(0), u(NA), None))
        if bad_field is not None:
            with pytest.raises(ValueError, match="field 99"):
                check(call(u(bad_field), u(0), u(NQ + 1), u(0), u(NA), None))
    for fn, obj in ((lib.sw_hits_align_block, world.bare), (lib.sw_hits_local_block, world.bare), (lib.sw_hits_loci_block, world.bare),
                    (lib.sw_oligos_thermo_block, world.hamming), (lib.sw_oligos_thermo_block, world.edit)):
        with pytest.raises(ValueError, match="made without"):
            check(fn(obj._h, u(0), u(0), u(1), u(0), u(1), ptr))
    assert np.all(buf == 0xA5A5A5A5)
