"""GPU: the nearest-neighbour sums of the oligo search (Batch.oligo_hits(..., thermo=, max_dg=); csrc/oligo.hip, DESIGN.md section
3.2o) against the host restatement (tests/tools/oligo_thermo_host.py on top of tests/tools/oligo_host.py) on the same text: n_stable,
the seven stable fields and dh, ds, dg of the whole site list, exactly -- and every field of the search without a model, unchanged.
The models are random int16 tables: asymmetric, so that an index-order or strand mistake changes a sum."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oligo_host as H  # noqa: E402
import oligo_thermo_host as TH  # noqa: E402

pytestmark = pytest.mark.gpu
TILE, LANE, LMIN = 1024, 16, 8
NO_HIT = 0xFFFFFFFF
FIELDS = ("n_sites", "best_mm", "best_record", "best_pos", "best_strand")
SITE_FIELDS = ("oligo", "assembly", "record", "pos", "strand", "mm")
SIGNED = ("stable_dg", "stable_dh", "stable_ds")


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, seq, n):
    s = bytearray(seq)
    for i in rng.sample(range(len(s)), n):
        s[i] = ord("ACGT"["ACGT".index(chr(s[i])) ^ rng.randrange(1, 4)])
    return bytes(s)


def _model(stack, end, init):
    from seqwin_amd.oligos import ThermoModel
    return ThermoModel(stack, end, init)


class World:
    """the batch, its text, the oligos, and every reference, each computed once and never changed"""

    def __init__(self, d):
        from seqwin_amd.device import Batch
        rng = random.Random(2024)
        R = _rand(rng, 2300)                                       # one run of three tiles: window ends are counted from LMIN on
        at = 1500
        text31 = bytearray(R[at + 100:at + 131])
        text31[3], text31[17] = ord("A"), ord("C")
        R = R[:at + 100] + bytes(text31) + R[at + 131:]
        cut = {8: (63, 64, 1023, 1024), 9: (1024,), 20: (1023, 1024), 31: (1024, 2047), 32: (63, 64, 1023, 1024, 2048)}
        oligos = []
        for L, ends in cut.items():                                # the text itself, at the last end of a lane / a tile and the first of the next
            for idx in ends:
                e = idx + LMIN - 1
                oligos.append(R[e - L + 1:e + 1])
        plant = {L: _rand(rng, L) for L in (8, 9, 20, 31, 32)}     # at a run's first possible end (e + 1 == L) and at its last base
        runs = [plant[L] + _rand(rng, 40) + _mutate(rng, plant[L], 1) + _rand(rng, 30) + plant[L] for L in plant]
        X = _rand(rng, 20)                                         # two exact copies in one record and one in the next: a tie on dg
        half = _rand(rng, 10)
        pal = half + H.revcomp(half)                               # its own reverse complement: two hits at one place
        assert H.revcomp(pal) == pal
        deg20 = R[at:at + 20].replace(b"A", b"R").replace(b"C", b"Y")                    # every set holds the partner
        deg31 = bytearray(R[at + 100:at + 131])
        for j, c in ((3, b"B"), (17, b"D"), (29, b"N")):           # B without its partner where the text is A, D where it is C: the least member
            deg31[j] = c[0]
        oligos += [plant[L] for L in plant] + [X, pal, deg20, bytes(deg31), b"ACGTNNRY", b"GGWCCYRAK", H.revcomp(R[700:731])]
        self.asms = [
            [R],
            [b"N".join(runs[:3]) + b"NNN" + runs[3], runs[4] + b"N" + _rand(rng, 200)],
            [H.revcomp(R[900:1300]) + b"NNNNN" + _rand(rng, 300), _rand(rng, 500)],
            [_rand(rng, 300) + X + _rand(rng, 150) + X + _rand(rng, 50), _rand(rng, 150) + X + _rand(rng, 100) + pal + _rand(rng, 60)],
            [_mutate(rng, R[:1500], 60)],
            [b"ACGTACG", b"N" * 40],                                # nothing of LMIN valid bases: a column without a hit
        ]
        self.oligos = oligos
        assert sorted({len(o) for o in oligos}) == [8, 9, 20, 31, 32]
        paths = []
        for i, recs in enumerate(self.asms):
            p = d / f"t{i}.fa"
            with open(p, "wb") as f:
                for j, r in enumerate(recs):
                    f.write(b">t%d_r%d\n" % (i, j) + b"\n".join(r[k:k + 70] for k in range(0, len(r), 70)) + b"\n")
            paths.append(p)
        self.batch = Batch.from_fasta(paths, n_cpu=2)
        self.random = TH.random_model(np.random.default_rng(7))
        self._plain, self._thermo = {}, {}

    def plain(self, mm, clamp):
        if (mm, clamp) not in self._plain:
            self._plain[mm, clamp] = H.search(self.oligos, self.asms, mm, clamp)
        return self._plain[mm, clamp]

    def want(self, mm, clamp, name, model, max_dg=None):
        key = (mm, clamp, name, max_dg)
        if key not in self._thermo:
            if max_dg is None:
                self._thermo[key] = TH.search(self.oligos, self.asms, mm, clamp, model, plain=self.plain(mm, clamp))
            else:                                                  # the sums do not depend on max_dg: they are taken from the call without it
                sums = self.want(mm, clamp, name, model)["sites"]
                self._thermo[key] = TH.search(self.oligos, self.asms, mm, clamp, model, max_dg, plain=self.plain(mm, clamp),
                                              form=lambda *a: (sums["dh"], sums["ds"], sums["dg"]))
        return self._thermo[key]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(tmp_path_factory.mktemp("olthermo"))
    yield w
    w.batch.close()


def _compare_plain(o, want, sites=True):
    for f in FIELDS:
        got = getattr(o, f)()
        assert got.dtype == np.uint32 and np.array_equal(got, want[f]), f
    if sites:
        S = o.sites()
        for f in SITE_FIELDS:
            assert S[f].dtype == np.uint32 and np.array_equal(S[f], want["sites"][f]), f
        assert np.array_equal(S["cell_offsets"], want["sites"]["cell_offsets"])
        return S


def _compare_thermo(o, want, sites=True):
    """every array of a result made with thermo= against the restatement, whole; returns the stats"""
    S = _compare_plain(o, want, sites)
    got = o.n_stable()
    assert got.dtype == np.uint32 and np.array_equal(got, want["n_stable"]), "n_stable"
    for f in TH.STABLE_FIELDS:
        got = getattr(o, f)()
        assert got.dtype == (np.int32 if f in SIGNED else np.uint32) and got.shape == want[f].shape, f
        assert np.array_equal(got, want[f]), f
    if sites:
        for f in ("dh", "ds", "dg"):
            assert S[f].dtype == np.int32 and np.array_equal(S[f], want["sites"][f]), f
    st = o.stats()
    assert st["hits"] == int(want["n_sites"].sum()) and st["stable_hits"] == int(want["n_stable"].sum())
    return st


def _check(w, mm, clamp, name, model, max_dg=None, sites=True):
    want = w.want(mm, clamp, name, model, max_dg)
    o = w.batch.oligo_hits(w.oligos, mm, clamp, sites=sites, thermo=_model(*model), max_dg=max_dg)
    try:
        assert o.sizes() == (len(w.oligos), len(w.asms), mm, clamp)
        return want, _compare_thermo(o, want, sites)
    finally:
        o.close()


# ---- every sum, the stable fields, and the search itself unchanged ------------------------------------------------------------------------

@pytest.mark.parametrize("mm,clamp", [(0, 0), (2, 0), (3, 0), (0, 3), (2, 3), (3, 3)])
def test_sums_and_stable_sites(world, mm, clamp):
    w = world
    want, st = _check(w, mm, clamp, "random", w.random)
    assert st["passes"] == 1 and st["chunks"] == 1 and st["launches"] == 1 and st["thermo_ms"] >= 0 and st["site_thermo_ms"] >= 0
    assert np.array_equal(want["n_stable"], want["n_sites"])                      # max_dg=None: every hit counts
    none = want["n_sites"] == 0
    assert none[:, 5].all() and (want["stable_dg"][none] == -2 ** 31).all() and (want["stable_pos"][none] == NO_HIT).all()
    o = w.batch.oligo_hits(w.oligos, mm, clamp, sites=True)                       # the same call without a model: every field as before
    try:
        _compare_plain(o, w.plain(mm, clamp))
        st0 = o.stats()
        assert (st0["stable_hits"], st0["thermo_ms"], st0["site_thermo_ms"]) == (0, 0.0, 0.0)
        for k in ("windows", "passes", "chunks", "launches", "hits", "buffer_doublings", "chunk_splits", "comparisons"):
            assert st0[k] == st[k], k
    finally:
        o.close()
    if mm == 3 and clamp == 0:
        # the most stable site is not always the least-mm one: that is the point of the feature
        other = (want["n_sites"] > 0) & ((want["stable_pos"] != want["best_pos"]) | (want["stable_record"] != want["best_record"])) & \
                (want["stable_mm"] > want["best_mm"])
        assert other.sum() >= 3
    if mm == 0 and clamp == 0:
        q_x, q_pal = len(w.oligos) - 7, len(w.oligos) - 6
        # three exact copies: all have one dg, the tie goes to the record, then the position
        assert want["n_sites"][q_x, 3] == 3 and (want["stable_record"][q_x, 3], want["stable_pos"][q_x, 3]) == (want["best_record"][q_x, 3], 300)
        assert want["n_sites"][q_pal, 3] == 2                                     # the palindrome: two strands at one place
        e = want["sites"]["cell_offsets"]
        c = q_pal * 6 + 3
        assert want["sites"]["strand"][int(e[c]):int(e[c + 1])].tolist() == [0, 1]


def test_santalucia98_and_the_summary(world):
    from seqwin_amd import oligos as O
    w = world
    m = O.santalucia98()
    model = (m.stack, m.end, m.init)
    want = w.want(2, 0, "sl98", model, -9000)
    o = w.batch.oligo_hits(w.oligos, 2, 0, sites=True, thermo=m, max_dg=-9000)
    try:
        _compare_thermo(o, want)
        assert 0 < want["n_stable"].sum() < want["n_sites"].sum()                 # an exact 20-mer is far below -9 kcal/mol, most 8-mers above
        got, ref = O.thermo_summary(o, 3), O.thermo_summary(want, 3)
        for k in ("f_tar_stable", "f_neg_stable", "mean_stable_dg_tar", "min_stable_dg_neg"):
            assert np.array_equal(got[k], ref[k], equal_nan=True), k
        S = o.sites()
        tm = O.melting_temperature(S["dh"], S["ds"], o.lengths[S["oligo"]])
        assert tm.shape == S["dg"].shape and np.isfinite(tm[S["mm"] == 0]).all()
    finally:
        o.close()


@pytest.mark.parametrize("sign", [1, -1])
def test_the_key_bias_on_both_signs(world, sign):
    """every dg entry and init at +-15000: a 32-mer's dg is +-510000, the widest the stable key's 20 biased bits must hold; all sites of
    one length tie, so the key's position bits decide"""
    w = world
    stack, end, init = (a.copy() for a in w.random)
    stack[2], end[2], init[2] = sign * 15000, sign * 15000, sign * 15000
    want, _ = _check(w, 2, 0, f"bias{sign}", (stack, end, init))
    q32 = [q for q, o in enumerate(w.oligos) if len(o) == 32]
    has = want["n_sites"][q32] > 0
    assert has.sum() >= 5 and (want["stable_dg"][q32][has] == sign * 34 * 15000).all()
    _check(w, 2, 0, f"bias{sign}", (stack, end, init), max_dg=sign * 34 * 15000)  # the threshold at the bound itself


def test_max_dg_counts_a_site_of_exactly_that_dg(world):
    w = world
    base = w.want(2, 0, "random", w.random)
    dg = np.sort(base["sites"]["dg"])
    for t in (int(dg[len(dg) // 2]), int(dg[0]), int(dg[0]) - 1, int(dg[-1])):
        want, _ = _check(w, 2, 0, "random", w.random, max_dg=t)
        assert want["n_stable"].sum() == int((dg <= t).sum())
        for f in TH.STABLE_FIELDS:                                                # the most stable hit is chosen among all hits
            assert np.array_equal(want[f], base[f])
    assert int((dg <= dg[len(dg) // 2]).sum()) > int((dg < dg[len(dg) // 2]).sum())
    _check(w, 2, 0, "random", w.random, max_dg=int(dg[len(dg) // 2]), sites=False)


# ---- the hooks ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", [1, 3])
def test_groups_of_oligos(world, monkeypatch, group):
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_GROUP", str(group))
    _, st = _check(world, 2, 3, "random", world.random)
    assert st["passes"] == -(-len(world.oligos) // group)
    _check(world, 2, 3, "random", world.random, sites=False)


def test_a_small_site_buffer_splits_and_doubles(world, monkeypatch):
    """1 KiB holds 128 sites: the six assemblies together overflow it and are split, the first alone overflows it and the buffer
    doubles.  A chunk that is redone must not count its stable hits twice."""
    w = world
    want = w.want(2, 0, "random", w.random)
    assert want["n_sites"][:, 0].sum() > 128
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", "1")
    _, st = _check(w, 2, 0, "random", w.random)
    assert st["chunk_splits"] >= 1 and st["buffer_doublings"] >= 1 and st["chunks"] >= 3, st
    dg = np.sort(want["sites"]["dg"])
    _check(w, 2, 0, "random", w.random, max_dg=int(dg[len(dg) // 3]))
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_GROUP", "3")
    _, st = _check(w, 2, 0, "random", w.random)
    assert st["chunk_splits"] >= 1 and st["passes"] == -(-len(w.oligos) // 3)


def test_a_launch_split(world, monkeypatch):
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_MAX_BLOCKS", "1")
    _, st = _check(world, 3, 0, "random", world.random)
    assert st["launches"] > 1


# ---- blocks and refusals --------------------------------------------------------------------------------------------------------------

def test_blocks(world):
    w = world
    want = w.want(2, 0, "random", w.random)
    o = w.batch.oligo_hits(w.oligos, 2, 0, thermo=_model(*w.random))
    try:
        nq, na = len(w.oligos), len(w.asms)
        for rows, cols in (((0, nq), (0, na)), ((2, 9), (1, 4)), ((nq - 1, nq), (0, 1)), ((4, 4), (0, na)), ((0, nq), (5, 6))):
            for f in ("n_stable",) + TH.STABLE_FIELDS:
                assert np.array_equal(getattr(o, f)(rows, cols), want[f][rows[0]:rows[1], cols[0]:cols[1]]), f
        with pytest.raises(ValueError, match="outside"):
            o.stable_dg((0, nq + 1), (0, 1))
        with pytest.raises(ValueError, match="sites=True"):
            o.sites()
    finally:
        o.close()


def test_refusals(world):
    from seqwin_amd import oligos as O
    w = world
    m = _model(*w.random)
    with pytest.raises(ValueError, match="max_edits"):
        w.batch.oligo_hits(w.oligos, 0, 0, max_edits=1, thermo=m)
    with pytest.raises(ValueError, match="ThermoModel"):
        w.batch.oligo_hits(w.oligos, 2, 0, thermo=w.random)
    with pytest.raises(ValueError, match="ThermoModel"):
        w.batch.oligo_hits(w.oligos, 2, 0, max_dg=-5000)
    with pytest.raises(ValueError, match="max_dg"):
        w.batch.oligo_hits(w.oligos, 2, 0, thermo=m, max_dg=-0.5)
    for bad in ("x", [1], 2 ** 31, -2 ** 31 - 1):
        with pytest.raises(ValueError, match="max_dg"):
            w.batch.oligo_hits(w.oligos, 2, 0, thermo=m, max_dg=bad)
    o = w.batch.oligo_hits(w.oligos[:3], 0, 0, thermo=m, max_dg=-2 ** 31)    # the least int32 is a threshold like any other: nothing is stable
    try:
        assert o.n_stable().sum() == 0 and o.n_sites().sum() > 0
    finally:
        o.close()
    m2 = _model(*(a.copy() for a in w.random))
    m2.stack[2, 0, 0, 0, 0] = 15001                                # changed behind the constructor's back: the library checks again
    with pytest.raises(ValueError, match="15000"):
        w.batch.oligo_hits(w.oligos, 2, 0, thermo=m2)
    o = w.batch.oligo_hits(w.oligos[:3], 0, 0, sites=True)
    try:
        for f in ("n_stable",) + TH.STABLE_FIELDS:
            with pytest.raises(ValueError, match="thermo"):
                getattr(o, f)()
        assert "dg" not in o.sites()
        with pytest.raises(ValueError, match="n_stable|thermo"):
            O.thermo_summary(o, 3)
    finally:
        o.close()
