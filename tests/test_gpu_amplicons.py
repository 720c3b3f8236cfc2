"""GPU: the amplicon stage of csrc/amplicons.hip (OligoHits.amplicons) against the host restatement of its specification
(tests/tools/amplicons_host.py) on the site list of the same result: both count matrices, the nine columns of the list and its cell
offsets, whole; without probe and filter also against seqwin_amd.oligos.amplicons.  A handful of records with planted primer and
probe sites at the places where the stage can go wrong: the length bounds, equal positions, record and assembly boundaries, ranges
around the wave (63, 64, 65) and far above it, interleaved orientations, probes flush against and one base into a primer site, edit
sites whose end is not pos + L, the dg filter."""
import ctypes
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import amplicons_host as A  # noqa: E402
import oligo_host as H  # noqa: E402

from seqwin_amd import oligos as O  # noqa: E402

pytestmark = pytest.mark.gpu
L = 20


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _plant(rng, n, places):
    """a random record of n bases with `places` = [(pos, text)] written over it"""
    s = bytearray(_rand(rng, n))
    for pos, text in places:
        assert 0 <= pos and pos + len(text) <= n
        s[pos:pos + len(text)] = text
    return bytes(s)


def _batch(d, assemblies):
    from seqwin_amd.device import Batch
    paths = []
    for i, recs in enumerate(assemblies):
        p = d / f"a{i}.fa"
        with open(p, "wb") as f:
            for j, r in enumerate(recs):
                f.write(b">a%d_r%d\n" % (i, j) + b"\n".join(r[k:k + 70] for k in range(0, len(r), 70)) + b"\n")
        paths.append(p)
    return Batch.from_fasta(paths, n_cpu=2)


def _check(o, pairs, lo, hi, probes=None, max_dg=None, loop=True):
    """every array of o.amplicons(...) against the restatement on o.sites(); returns (the restatement's result, the call's stats)"""
    S, na = o.sites(), o.sizes()[1]
    want = A.amplicons_merge(S, pairs, lo, hi, na, probes, max_dg)
    if loop:
        other = A.amplicons_loop(S, pairs, lo, hi, na, probes, max_dg)
        for f in A.FIELDS + ("cell_offsets", "n_amplicons", "n_detected"):
            assert np.array_equal(want[f], other[f]), f
    am = o.amplicons(pairs, lo, hi, probes=probes, max_dg=max_dg)
    try:
        assert am.sizes() == (len(pairs), na, lo, hi)
        for name in ("n_amplicons", "n_detected"):
            got = getattr(am, name)()
            assert got.dtype == np.uint32 and got.shape == (len(pairs), na), name
            assert np.array_equal(got, want[name]), name
        P = am.products()
        for f in A.FIELDS:
            assert P[f].dtype == np.uint32 and np.array_equal(P[f], want[f]), f
        assert P["cell_offsets"].dtype == np.uint64 and np.array_equal(P["cell_offsets"], want["cell_offsets"])
        iv = am.intervals()
        assert np.array_equal(iv["record"], want["record"]) and np.array_equal(iv["start"], want["start"]) and np.array_equal(iv["stop"], want["end"])
        st = am.stats()
        assert st["products"] == len(want["pair"]) and st["detected"] == int(want["n_detected"].sum())
        assert np.array_equal(am.n_amplicons((0, 1), (0, na)), want["n_amplicons"][:1])
    finally:
        am.close()
    if probes is None and max_dg is None:
        prod, n_amp = O.amplicons(o, o.lengths, pairs, lo, hi)
        for f in O.AMPLICON_FIELDS:
            assert np.array_equal(prod[f].astype(np.uint32), want[f]), f
        assert np.array_equal(n_amp, want["n_amplicons"])
    # products=False: the same matrices, and nothing emitted or ordered
    am = o.amplicons(pairs, lo, hi, probes=probes, max_dg=max_dg, products=False)
    try:
        assert np.array_equal(am.n_amplicons(), want["n_amplicons"]) and np.array_equal(am.n_detected(), want["n_detected"])
        s2 = am.stats()
        assert s2["products"] == st["products"] and s2["emit_ms"] == 0.0 and s2["order_ms"] == 0.0
        assert s2["launches"] < st["launches"] or st["products"] == 0
        with pytest.raises(ValueError):
            am.products()
    finally:
        am.close()
    return want, st


@pytest.fixture(scope="module")
def primers():
    rng = random.Random(7)
    f, r = _rand(rng, L), _rand(rng, L)
    half = _rand(rng, L // 2)
    pal = half + H.revcomp(half)                                   # its own reverse complement
    probe = f[-1:] + _rand(rng, L - 2) + H.revcomp(r)[:1]           # may overlap either primer's site by one base
    return dict(f=f, r=r, rc_f=H.revcomp(f), rc_r=H.revcomp(r), pal=pal, probe=probe, rc_probe=H.revcomp(probe), absent=_rand(rng, L))


# ---- 1-4: bounds, equal positions, boundaries, empty and repeated cases ------------------------------------------------------------

@pytest.fixture(scope="module")
def small(tmp_path_factory, primers):
    p = primers
    rng = random.Random(11)
    f, rc_r = p["f"], p["rc_r"]
    lo, hi = 100, 160
    bounds = [_plant(rng, 300, [(50, f), (50 + n - L, rc_r)]) for n in (lo - 1, lo, hi, hi + 1)]          # records 0..3
    equal = [_plant(rng, 200, [(30, p["pal"])]), _plant(rng, 260, [(40, p["pal"]), (120, p["rc_r"])])]      # records 4, 5
    # record 6 ends with f, record 7 starts with rc_r: adjacent in the batch-wide base index; then the same across the assembly boundary
    edge = [_plant(rng, 256, [(256 - L, f)]), _plant(rng, 320, [(8, rc_r), (150, f), (280 - L, rc_r), (320 - L, f)])]
    nxt = [_plant(rng, 200, [(4, rc_r)])]                                                                # assembly 1: record 8
    empty = [_rand(rng, 300)]                                                                            # assembly 2: no site at all
    asms = [bounds + equal + edge, nxt, empty]
    b = _batch(tmp_path_factory.mktemp("ampsmall"), asms)
    oligos = [p["f"], p["r"], p["pal"], p["absent"]]
    o = b.oligo_hits(oligos, 0, 0, sites=True)
    yield o, (lo, hi)
    o.close()
    b.close()


def test_length_bounds(small):
    o, (lo, hi) = small
    want, _ = _check(o, [(0, 1)], lo, hi)
    rows = [(int(want["record"][i]), int(want["end"][i] - want["start"][i])) for i in range(len(want["pair"]))]
    assert (1, lo) in rows and (2, hi) in rows and not any(r in (0, 3) for r, _ in rows)
    wider, _ = _check(o, [(0, 1)], lo - 1, hi + 1)
    assert {0, 1, 2, 3} <= set(wider["record"].tolist())


def test_equal_positions_and_self_pairs(small):
    o, _ = small
    want, _ = _check(o, [(2, 2), (2, 1), (1, 2)], L, 120)
    t = [tuple(int(want[f][i]) for f in A.FIELDS) for i in range(len(want["pair"]))]
    assert (0, 0, 4, 30, 30 + L, 0, 0, 0, 0) in t and (0, 0, 5, 40, 40 + L, 0, 0, 0, 0) in t      # pos_r == pf, f == r: + only
    assert not any(row[0] == 0 and row[5] == 1 for row in t)
    assert (1, 0, 5, 40, 120 + L, 0, 0, 0, 0) in t and (2, 0, 5, 40, 120 + L, 1, 0, 0, 0) in t


def test_record_and_assembly_boundaries(small):
    o, _ = small
    want, _ = _check(o, [(0, 1)], 1, 1000)
    t = {(int(want["record"][i]), int(want["start"][i]), int(want["end"][i])) for i in range(len(want["pair"]))}
    assert (7, 150, 280) in t                                      # the product inside record 7
    assert not any(rec == 6 for rec, _, _ in t) and not any(start == 300 for rec, start, _ in t if rec == 7)
    assert want["n_amplicons"][0, 1] == 0 and want["n_amplicons"][0, 2] == 0


def test_empty_and_repeated(small):
    o, (lo, hi) = small
    want, _ = _check(o, [(0, 1), (3, 1), (0, 3), (0, 1), (3, 3)], lo, hi, probes=[None, 0, 3, 3, None])
    assert np.array_equal(want["n_amplicons"][0], want["n_amplicons"][3]) and want["n_amplicons"][0].sum() == 3   # records 1, 2 and the one inside record 7
    assert not want["n_amplicons"][[1, 2, 4]].any() and not want["n_amplicons"][:, 2].any() and not want["n_detected"].any()


# ---- 5: repeats: the wave route, the merge of the orientations, the launch split -------------------------------------------------------

@pytest.fixture(scope="module")
def repeats(tmp_path_factory, primers):
    p = primers
    rng = random.Random(13)
    recs = []
    for n in (1, 63, 64, 65, 300):                                 # one first site, n partners 21 bases apart, a probe site among them
        places = [(10, p["f"]), (35, p["probe"])] + [(60 + 21 * i, p["rc_r"]) for i in range(n)]
        recs.append(_plant(rng, 60 + 21 * n + 40, places))
    # both orientations interleaved in one cell: + products start at 10 and 300, - products at 40 and 330
    inter = _plant(rng, 700, [(10, p["f"]), (40, p["r"]), (200, p["rc_f"]), (230, p["rc_r"]), (300, p["f"]), (330, p["r"]), (480, p["rc_f"]), (510, p["rc_r"])])
    b = _batch(tmp_path_factory.mktemp("amprep"), [recs[:2], recs[2:] + [inter]])
    o = b.oligo_hits([p["f"], p["r"], p["probe"]], 0, 0, sites=True)
    yield o
    o.close()
    b.close()


@pytest.mark.parametrize("hook", [None, ("SEQWIN_AMD_AMP_WAVE_RANGE", "4"), ("SEQWIN_AMD_AMP_MAX_BLOCKS", "1")])
def test_repeats_wave_route_and_order(repeats, monkeypatch, hook):
    if hook:
        monkeypatch.setenv(*hook)
    want, st = _check(repeats, [(0, 1), (1, 0)], 1, 7000, probes=[2, None], loop=False)
    per_record = np.bincount(want["record"][want["pair"] == 0], minlength=6)
    assert per_record[:5].tolist() == [1, 63, 64, 65, 300]
    cell = (want["pair"] == 0) & (want["record"] == 5)
    assert want["orientation"][cell].tolist()[:4] == [0, 0, 1, 1] and len(set(want["orientation"][cell].tolist())) == 2
    starts = want["start"][cell].tolist()
    assert starts == sorted(starts) and starts[0] == 10 and 40 in starts and 300 in starts and 330 in starts
    assert want["n_detected"][0].sum() >= 1 + 63 + 64 + 65 + 300 - 5 and not want["n_detected"][1].any()
    if hook:
        monkeypatch.delenv(hook[0])
    plain = repeats.amplicons([(0, 1), (1, 0)], 1, 7000, probes=[2, None]).stats()
    if hook is None:
        assert st["wave_items"] >= 2                               # the ranges of 65 and of 300, for either pair
    elif hook[0].endswith("WAVE_RANGE"):
        assert st["wave_items"] > plain["wave_items"]
    else:
        assert st["launches"] > plain["launches"] and st["wave_items"] == plain["wave_items"]
    assert st["partners"] >= st["products"]


def test_repeats_against_the_loop_form(repeats):
    """the triple loop on the cell with the interleaved orientations and the short repeats only (the loop is cubic)"""
    _check(repeats, [(0, 1), (1, 0), (0, 0)], 1, 250, probes=[2, 2, None])


# ---- 6: probes -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probed(tmp_path_factory, primers):
    p = primers
    rng = random.Random(17)
    flush = _plant(rng, 400, [(100, p["f"]), (100 + L, p["probe"]), (300 - L, p["rc_probe"]), (300, p["rc_r"])])        # both count
    into = _plant(rng, 400, [(119, p["probe"]), (100, p["f"]), (281, p["probe"]), (300, p["rc_r"])])                    # one base into either
    minus = _plant(rng, 400, [(60, p["r"]), (150, p["rc_probe"]), (260, p["rc_f"])])                                    # orientation -
    b = _batch(tmp_path_factory.mktemp("ampprobe"), [[flush, into], [minus]])
    o = b.oligo_hits([p["f"], p["r"], p["probe"]], 0, 0, sites=True)
    yield o
    o.close()
    b.close()


def test_probes(probed):
    want, _ = _check(probed, [(0, 1), (0, 1)], 50, 300, probes=[2, None])
    t = {(int(want["pair"][i]), int(want["record"][i])): int(want["n_probe"][i]) for i in range(len(want["pair"]))}
    assert t == {(0, 0): 2, (0, 1): 0, (0, 2): 1, (1, 0): 0, (1, 1): 0, (1, 2): 0}
    S = probed.sites()
    assert {(int(r), int(x)) for q, r, x in zip(S["oligo"], S["record"], S["pos"]) if q == 2} >= {(0, 120), (0, 280), (1, 119), (1, 281), (2, 150)}
    assert want["n_detected"].tolist() == [[1, 1], [0, 0]] and want["n_amplicons"].tolist() == [[2, 1], [2, 1]]
    _check(probed, [(1, 0)], 50, 300, probes=[A.NO_PROBE])


# ---- 7: a max_edits result: the sites' own ends ---------------------------------------------------------------------------------------

def test_edit_result_ends_decide(tmp_path_factory, primers):
    p = primers
    rng = random.Random(19)
    extra = next(c for c in b"ACGT" if c not in p["rc_r"][9:11])
    bulged = p["rc_r"][:10] + bytes([extra]) + p["rc_r"][10:]                                                        # one base more
    probe_bulged = p["probe"][:10] + p["probe"][11:]                                                                 # one base fewer
    rec = _plant(rng, 400, [(50, p["f"]), (90, probe_bulged), (140, p["probe"]), (200, bulged)])
    b = _batch(tmp_path_factory.mktemp("ampedit"), [[rec], [_plant(rng, 300, [(20, p["f"]), (120, p["rc_r"])])]])
    o = b.oligo_hits([p["f"], p["r"], p["probe"]], sites=True, max_edits=1)
    try:
        S = o.sites()
        last = (S["oligo"] == 1) & (S["record"] == 0) & (S["strand"] == 1)
        assert last.any() and (S["end"][last] - S["pos"][last] != L).any()                  # the last site is not L long
        assert ((S["oligo"] == 2) & (S["end"] - S["pos"] == L - 1)).any()                   # nor is one of the probe's
        ends = sorted(set(int(e) for e in S["end"][last]))
        top = ends[-1] - 50
        at, _ = _check(o, [(0, 1)], 1, top, probes=[2])
        below, _ = _check(o, [(0, 1)], 1, top - 1, probes=[2])
        assert at["n_amplicons"][0, 0] == below["n_amplicons"][0, 0] + int((S["end"][last] == ends[-1]).sum())
        assert at["n_probe"][at["record"] == 0].max() >= 2
        _check(o, [(0, 1), (1, 0)], 1, 400)
    finally:
        o.close()
        b.close()


# ---- 8: a thermo= result and max_dg; the refusals ------------------------------------------------------------------------------------

def test_dg_filter_and_refusals(tmp_path_factory, primers, small):
    p = primers
    rng = random.Random(23)
    weak = bytearray(p["f"])
    for i in (5, 12):
        weak[i] = ord("ACGT"["ACGT".index(chr(weak[i])) ^ 1])
    rec = _plant(rng, 500, [(40, p["f"]), (100, bytes(weak)), (200, p["probe"]), (300, p["rc_r"])])
    b = _batch(tmp_path_factory.mktemp("ampdg"), [[rec]])
    o = b.oligo_hits([p["f"], p["r"], p["probe"]], 2, 0, sites=True, thermo=O.santalucia98())
    try:
        S = o.sites()
        dg = {int(x): int(g) for q, x, g in zip(S["oligo"], S["pos"], S["dg"]) if q == 0}
        assert dg[40] < dg[100]
        between = (dg[40] + dg[100]) // 2
        every, _ = _check(o, [(0, 1)], 1, 400, probes=[2])
        kept, _ = _check(o, [(0, 1)], 1, 400, probes=[2], max_dg=between)
        assert every["start"].tolist() == [40, 100] and kept["start"].tolist() == [40] and kept["n_probe"].tolist() == [1]
        none, _ = _check(o, [(0, 1)], 1, 400, probes=[2], max_dg=dg[40] - 1)
        assert len(none["pair"]) == 0
        for bad in (dict(pairs=[]), dict(pairs=[(0, 3)]), dict(pairs=[(0, 1)], probes=[7]), dict(pairs=[(0, 1)], probes=[2, 2]), dict(pairs=[(0, 1)], lo=0),
                    dict(pairs=[(0, 1)], lo=9, hi=8), dict(pairs=[(0, 1)], max_dg=1.5), dict(pairs=np.zeros((65537, 2), np.uint32))):
            with pytest.raises(ValueError):
                o.amplicons(bad["pairs"], bad.get("lo", 1), bad.get("hi", 100), probes=bad.get("probes"), max_dg=bad.get("max_dg"))
    finally:
        o.close()
    plain, _ = small
    with pytest.raises(ValueError):
        plain.amplicons([(0, 1)], 1, 100, max_dg=-1000)            # max_dg on a result without a model
    counts_only = b.oligo_hits([p["f"], p["r"]], 0, 0)
    try:
        with pytest.raises(ValueError):
            counts_only.amplicons([(0, 1)], 1, 100)                # a result made without sites
        # the library's own checks, behind the wrapper's
        from seqwin_amd._core import _ptr
        from seqwin_amd._lib import c_u64, c_vp, check, lib
        pairs = np.array([[0, 1]], np.uint32)
        h = c_vp()
        for handle, n, lo, hi, no_th in ((counts_only._h, 1, 1, 100, 1), (plain._h, 0, 1, 100, 1), (plain._h, 1, 0, 100, 1), (plain._h, 1, 5, 4, 1),
                                         (plain._h, 1, 1, 100, 0)):
            with pytest.raises(ValueError):
                check(lib.sw_oligos_amplicons(handle, _ptr(pairs), None, c_u64(n), c_u64(lo), c_u64(hi), ctypes.c_int(1), ctypes.c_int64(0),
                                              ctypes.c_int(no_th), c_vp(0), ctypes.byref(h)))
        far = np.array([[0, 9]], np.uint32)
        with pytest.raises(ValueError):
            check(lib.sw_oligos_amplicons(plain._h, _ptr(far), None, c_u64(1), c_u64(1), c_u64(100), ctypes.c_int(1), ctypes.c_int64(0), ctypes.c_int(1),
                                          c_vp(0), ctypes.byref(h)))
    finally:
        counts_only.close()
        b.close()
