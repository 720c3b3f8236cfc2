"""CPU: the nearest-neighbour sums of the oligo search -- the two forms of the host restatement
(tests/tools/oligo_thermo_host.py) against each other, the model of seqwin_amd.oligos (constructor, from_dh_ds, santalucia98,
melting_temperature, thermo_summary), and csrc/oligo_thermo_core.hpp compiled for the host under sanitizers."""
import math
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oligo_host as H  # noqa: E402
import oligo_thermo_host as TH  # noqa: E402

from seqwin_amd import oligos as O  # noqa: E402

LETTERS = "ACGTRYSWKMBDHVN"
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
# SantaLucia 1998, Table 2 (the issue's table), typed here independently of the package: dH kcal/mol, dS cal/(K mol)
NN = {"AA/TT": (-7.9, -22.2), "AT/TA": (-7.2, -20.4), "TA/AT": (-7.2, -21.3), "CA/GT": (-8.5, -22.7), "GT/CA": (-8.4, -22.4),
      "CT/GA": (-7.8, -21.0), "GA/CT": (-8.2, -22.2), "CG/GC": (-10.6, -27.2), "GC/CG": (-9.8, -24.4), "GG/CC": (-8.0, -19.9)}


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _random_oligo(rng, L, degenerate):
    return "".join(rng.choice(LETTERS if rng.random() < degenerate else "ACGT") for _ in range(L))


def _random_cases(seed, n_asm=3):
    """random text with N runs, oligos cut from it (exact, mutated, degenerate, reverse-complemented) so that hits exist on both strands"""
    rng = random.Random(seed)
    asms = []
    for a in range(n_asm):
        recs = []
        for r in range(rng.randrange(1, 3)):
            t = list(_rand(rng, rng.randrange(60, 260)))
            for _ in range(rng.randrange(0, 3)):
                t[rng.randrange(len(t))] = "N"
            recs.append("".join(t).encode())
        asms.append(recs)
    oligos = []
    for _ in range(8):
        L = rng.choice((8, 9, 12, 20, 31, 32))
        rec = rng.choice(rng.choice(asms)).decode()
        at = rng.randrange(0, len(rec) - L)
        o = list(rec[at:at + L].replace("N", "A"))
        for _ in range(rng.randrange(0, 3)):
            j = rng.randrange(L)
            o[j] = rng.choice(LETTERS)
        o = "".join(o)
        oligos.append(H.revcomp(o.encode()).decode() if rng.random() < 0.5 and set(o) <= set("ACGT") else o)
    oligos.append(_random_oligo(rng, 8, 0.6))
    return oligos, asms


@pytest.mark.parametrize("seed", range(6))
def test_the_two_forms_agree_on_random_cases(seed):
    oligos, asms = _random_cases(seed)
    model = TH.random_model(np.random.default_rng(seed))
    plain = H.search(oligos, asms, 2, seed % 3)
    S = plain["sites"]
    assert len(S["oligo"]) > 10 and set(S["strand"].tolist()) == {0, 1}
    a, b = TH.sums_gather(oligos, asms, S, model), TH.sums_loop(oligos, asms, S, model)
    for x, y in zip(a, b):
        assert x.dtype == np.int32 and np.array_equal(x, y)
    # the cell summary: max_dg = one site's dg counts that site
    dg = a[2]
    w = TH.search(oligos, asms, 2, seed % 3, model, max_dg=int(dg[0]), plain=plain)
    assert w["n_stable"].sum() == int((dg <= dg[0]).sum()) >= 1
    w_all = TH.search(oligos, asms, 2, seed % 3, model, plain=plain)
    assert np.array_equal(w_all["n_stable"], plain["n_sites"])
    assert np.array_equal(w_all["stable_dg"] == TH.NO_SUM, plain["n_sites"] == 0)


def test_strand_1_is_strand_0_on_the_reverse_complement():
    rng = random.Random(11)
    model = TH.random_model(np.random.default_rng(11))
    for _ in range(200):
        L = rng.randrange(8, 33)
        o = _random_oligo(rng, L, 0.3)
        w = _rand(rng, L)
        assert TH.site_sums_loop(o, w, 1, model) == TH.site_sums_loop(o, H.revcomp(w.encode()).decode(), 0, model)


def test_santalucia98_strand_symmetry():
    """the 16 Watson-Crick stacks read from either strand: stack[x1][x2][c(x1)][c(x2)] == stack[c(x2)][c(x1)][x2][x1], on every plane; the
    ten of the table hold the table's values"""
    m = O.santalucia98()
    n = 0
    for x1 in range(4):
        for x2 in range(4):
            assert np.array_equal(m.stack[:, x1, x2, 3 - x1, 3 - x2], m.stack[:, 3 - x2, 3 - x1, x2, x1])
            assert m.stack[0, x1, x2, 3 - x1, 3 - x2] < 0
            n += 1
    assert n == 16
    for name, (dh, ds) in NN.items():
        x1, x2, y1, y2 = (CODE[c] for c in name.replace("/", ""))
        assert (y1, y2) == (3 - x1, 3 - x2)
        assert m.stack[0, x1, x2, y1, y2] == round(dh * 10) and m.stack[1, x1, x2, y1, y2] == round(ds * 10)
        assert m.stack[2, x1, x2, y1, y2] == round(1000 * dh - 310.15 * ds)      # (no entry is a tie of the rounding)
    wc = np.zeros((4, 4, 4, 4), bool)
    for x1 in range(4):
        for x2 in range(4):
            wc[x1, x2, 3 - x1, 3 - x2] = True
    assert (m.stack[:, ~wc] == 0).all() and (m.init == 0).all()                  # the defaults: not published values, zeros
    for x in range(4):
        for y in range(4):
            want = (0, 0, 0) if y != 3 - x else (23, 41, round(2300 - 310.15 * 4.1)) if x in (0, 3) else (1, -28, round(100 + 310.15 * 2.8))
            assert m.end[:, 0, x, y].tolist() == list(want) and m.end[:, 1, x, y].tolist() == list(want)
    mm = O.santalucia98(mismatch_stack=(5, -7), mismatch_end=(3, 9), temperature_K=300.0)
    assert (mm.stack[0][~wc] == 5).all() and (mm.stack[1][~wc] == -7).all() and (mm.stack[2][~wc] == 500 + 210).all()
    assert mm.end[:, 0, 0, 0].tolist() == [3, 9, 300 - 270] and np.array_equal(mm.stack[:2][:, wc], m.stack[:2][:, wc])


def _hand_sum(oligo):
    """a perfect site's sums written out from the table: every stack by its name or its other strand's, the two terminal pairs"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    dh = ds = dg = 0
    for a, b in zip(oligo, oligo[1:]):
        name = f"{a}{b}/{comp[a]}{comp[b]}"
        if name not in NN:
            name = f"{comp[b]}{comp[a]}/{b}{a}"
        h, s = NN[name]
        dh, ds, dg = dh + round(h * 10), ds + round(s * 10), dg + round(1000 * h - 310.15 * s)
    for c in (oligo[0], oligo[-1]):
        h, s = (2.3, 4.1) if c in "AT" else (0.1, -2.8)
        dh, ds, dg = dh + round(h * 10), ds + round(s * 10), dg + round(1000 * h - 310.15 * s)
    return dh, ds, dg


@pytest.mark.parametrize("oligo", ["ACGTTGCA", "GATTACAGGCTCAAGTCCTA"])
def test_a_perfect_site_equals_the_hand_sum(oligo):
    m = O.santalucia98()
    model = (m.stack, m.end, m.init)
    want = _hand_sum(oligo)
    assert TH.site_sums_loop(oligo, oligo, 0, model) == want
    assert TH.site_sums_loop(oligo, H.revcomp(oligo.encode()).decode(), 1, model) == want
    if oligo == "ACGTTGCA":
        # AC CG GT TT TG GC CA = GT/CA, CG/GC, GT/CA, AA/TT, CA/GT, GC/CG, CA/GT; two terminal A.T pairs
        assert want[0] == -84 - 106 - 84 - 79 - 85 - 98 - 85 + 23 + 23 and want[1] == -224 - 272 - 224 - 222 - 227 - 244 - 227 + 41 + 41
        assert -9300 < want[2] < -9050                                           # seven stacks of -1.0 .. -2.2 kcal/mol at 37 C, two ends of +1.03
    sites = dict(oligo=np.array([0, 0]), record=np.array([0, 1]), pos=np.array([3, 2]), strand=np.array([0, 1]))
    asms = [[b"TTT" + oligo.encode() + b"GG", b"CC" + H.revcomp(oligo.encode()) + b"A"]]
    for form in (TH.sums_gather, TH.sums_loop):
        dh, ds, dg = form([oligo], asms, sites, model)
        assert (dh.tolist(), ds.tolist(), dg.tolist()) == ([want[0]] * 2, [want[1]] * 2, [want[2]] * 2)


def test_the_degenerate_rule():
    """R = {A, G} facing a text T on strand 0 (y = A): the partner T is not in the set, x is its least member A; facing a text G
    (y = C): the set holds the partner G.  On strand 1 the text itself is y."""
    model = TH.random_model(np.random.default_rng(5))
    stack, end, init = (a.astype(np.int64) for a in model)
    o = "ACGTRCGT"

    def by_hand(xs, ys):
        return tuple(int(init[p] + end[p][0][xs[0]][ys[0]] + end[p][1][xs[-1]][ys[-1]] + sum(stack[p][xs[i]][xs[i + 1]][ys[i]][ys[i + 1]] for i in range(7)))
                     for p in range(3))

    # strand 0, window ACGTGCGT: the set holds G
    assert TH.site_sums_loop(o, "ACGTGCGT", 0, model) == by_hand([0, 1, 2, 3, 2, 1, 2, 3], [3, 2, 1, 0, 1, 2, 1, 0])
    # strand 0, window ACGTTCGT: y_5 = A, its partner T is not in {A, G}: x_5 = A
    assert TH.site_sums_loop(o, "ACGTTCGT", 0, model) == by_hand([0, 1, 2, 3, 0, 1, 2, 3], [3, 2, 1, 0, 0, 2, 1, 0])
    # strand 1, window ACGCACGT read backwards: y = T G C A C G C A; y_5 = C pairs with G, which the set holds
    assert TH.site_sums_loop(o, "ACGCACGT", 1, model) == by_hand([0, 1, 2, 3, 2, 1, 2, 3], [3, 2, 1, 0, 1, 2, 1, 0])
    # strand 1, window ACGAACGT: y_5 = A, partner T not in the set: x_5 = A
    assert TH.site_sums_loop(o, "ACGAACGT", 1, model) == by_hand([0, 1, 2, 3, 0, 1, 2, 3], [3, 2, 1, 0, 0, 2, 1, 0])
    # B = {C, G, T} without its partner: the least member is C
    assert TH.site_sums_loop("ACGTBCGT", "ACGTACGT", 0, model) == by_hand([0, 1, 2, 3, 1, 1, 2, 3], [3, 2, 1, 0, 3, 2, 1, 0])


def test_constructor_refusals():
    st, en, ini = np.zeros((3, 4, 4, 4, 4), np.int16), np.zeros((3, 2, 4, 4), np.int16), np.zeros(3, np.int32)
    m = O.ThermoModel(st, en, ini)
    assert m.stack.dtype == np.int16 and m.end.shape == (3, 2, 4, 4) and m.init.dtype == np.int32
    for bad in ((st.astype(np.int32), en, ini), (st, en.astype(np.int64), ini), (st, en, ini.astype(np.int64)), (st[:2], en, ini), (st, en[:, :1], ini),
                (st, en, ini[:2]), (st.tolist(), en, ini), (st, en, [0, 0, 0]), (st.reshape(3, 16, 16), en, ini)):
        with pytest.raises(ValueError, match="must be a NumPy array"):
            O.ThermoModel(*bad)
    for plane, ok in ((0, True), (1, True), (2, False)):            # only the dg plane is bounded
        for v in (15001, -15001):
            for which in range(3):
                arrs = [st.copy(), en.copy(), ini.copy()]
                if which == 2:
                    arrs[2][plane] = v
                else:
                    arrs[which][plane].flat[-1] = v
                if ok:
                    O.ThermoModel(*arrs)
                else:
                    with pytest.raises(ValueError, match="15000"):
                        O.ThermoModel(*arrs)
    edge = [st.copy(), en.copy(), ini.copy()]
    edge[0][2, 1, 2, 3, 0], edge[1][2, 1, 3, 3], edge[2][2] = 15000, -15000, -15000
    O.ThermoModel(*edge)
    z4, z2 = np.zeros((4, 4, 4, 4), np.int64), np.zeros((2, 4, 4), np.int64)
    with pytest.raises(ValueError, match="shape"):
        O.ThermoModel.from_dh_ds(z4[:3], z4, z2, z2, 0, 0)
    with pytest.raises(ValueError, match="shape"):
        O.ThermoModel.from_dh_ds(z4, z4, z2, z2[:1], 0, 0)
    with pytest.raises(ValueError, match="integers"):
        O.ThermoModel.from_dh_ds(z4 + 0.5, z4, z2, z2, 0, 0)
    with pytest.raises(ValueError):
        O.ThermoModel.from_dh_ds(z4 + 200, z4, z2, z2, 0, 0)             # dg = 20000 cal/mol
    with pytest.raises(ValueError):
        O.ThermoModel.from_dh_ds(z4, z4 + 40000, z2, z2, 0, 0)           # ds does not fit int16
    # round half to even: 100 * 0 - 300 * 15 / 10 = -450.0 exactly; 250 K x 0.1 x 1 = 25 -> no tie; T = 5, ds = 1: -0.5 -> -0; ds = 3: -1.5 -> -2
    m = O.ThermoModel.from_dh_ds(z4, z4 + 1, z2, z2 + 3, 0, -5, temperature_K=5.0)
    assert m.stack[2].max() == 0 and m.end[2].min() == -2 and m.end[2].max() == -2 and m.init.tolist() == [0, -5, 2]


def test_melting_temperature():
    rng = random.Random(3)
    for _ in range(200):
        dh, ds, L = rng.randrange(-3000, -300), rng.randrange(-8000, -800), rng.randrange(8, 33)
        c, na, div = 10 ** rng.uniform(-9, -5), 10 ** rng.uniform(-3, 0), rng.choice((1.0, 4.0))
        den = 1.987 * math.log(c / div) + (L - 1) * 0.368 * math.log(na) + ds * 0.1           # (the terms in another order)
        got = float(O.melting_temperature(dh, ds, L, c, na, div))
        if den < 0:
            want = dh * 100.0 / den - 273.15
            assert abs(got - want) <= 1e-9 * abs(want)
        else:
            assert math.isnan(got)
    # a 20-mer of the hand sum: a plausible two-state Tm at 0.25 uM, 50 mM Na+
    dh, ds, _ = _hand_sum("GATTACAGGCTCAAGTCCTA")
    assert 35.0 < float(O.melting_temperature(dh, ds, 20)) < 65.0
    out = O.melting_temperature(np.array([-1500, -1500, 100]), np.array([-4000, 4000, 0]), np.array([20, 20, 8]))
    assert out.dtype == np.float64 and not math.isnan(out[0]) and math.isnan(out[1]) and not math.isnan(out[2])
    assert math.isnan(float(O.melting_temperature(-100, 500, 8, oligo_molar=1.0, na_molar=1.0, divisor=1.0)))   # the denominator is 50 > 0
    assert math.isnan(float(O.melting_temperature(-100, 0, 8, oligo_molar=1.0, na_molar=1.0, divisor=1.0)))     # the denominator is 0


def test_thermo_summary():
    n = np.array([[1, 0, 2, 0], [0, 0, 0, 0], [3, 1, 0, 1]], np.uint32)
    dg = np.array([[-9000, -4000, -7000, TH.NO_SUM], [TH.NO_SUM] * 4, [-100, -300, TH.NO_SUM, 50]], np.int32)
    s = O.thermo_summary(dict(n_stable=n, stable_dg=dg), 2)
    assert s["f_tar_stable"].tolist() == [0.5, 0.0, 1.0] and s["f_neg_stable"].tolist() == [0.5, 0.0, 0.5]
    assert s["mean_stable_dg_tar"][0] == -6500.0 and math.isnan(s["mean_stable_dg_tar"][1]) and s["mean_stable_dg_tar"][2] == -200.0
    assert s["min_stable_dg_neg"][0] == -7000.0 and math.isnan(s["min_stable_dg_neg"][1]) and s["min_stable_dg_neg"][2] == 50.0
    assert set(s) == {"f_tar_stable", "f_neg_stable", "mean_stable_dg_tar", "min_stable_dg_neg"}
    s = O.thermo_summary(dict(n_stable=n, stable_dg=dg), 4)
    assert np.isnan(s["f_neg_stable"]).all() and np.isnan(s["min_stable_dg_neg"]).all()
    with pytest.raises(ValueError, match="n_tar"):
        O.thermo_summary(dict(n_stable=n, stable_dg=dg), 5)


def test_the_kernels_arithmetic_on_the_host(tmp_path):
    """seqwin_amd/csrc/oligo_thermo_core.hpp -- the window's planes from the packed words, the member test on the pattern row's mismatch
    planes, the least member, the three sums and the dg-only form of the scan kernel -- compiled for the host with
    tests/tools/oligo_thermo_core_driver.cpp (AddressSanitizer + UBSan where g++ links them) and run on random windows: every length
    8..32, both strands, degenerate oligos, any place of the window in its packed words, entries of +-15000 and int16's bounds."""
    src = [str(ROOT / "tests" / "tools" / "oligo_thermo_core_driver.cpp"), "-I", str(ROOT / "seqwin_amd" / "csrc"), "-o", str(tmp_path / "olt_core")]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    sanitized = subprocess.run(["g++", "-std=c++17"] + san + src, capture_output=True).returncode == 0
    if not sanitized:
        subprocess.run(["g++", "-std=c++17", "-O2"] + src, check=True, capture_output=True)
    print("oligo_thermo_core_driver: built", "with AddressSanitizer + UBSan" if sanitized else "WITHOUT sanitizers (g++ could not link them): a plain -O2 build")
    rng = random.Random(20)
    model = TH.random_model(np.random.default_rng(20))
    model[0][2].flat[::7] = 15000
    model[0][2].flat[3::7] = -15000
    model[0][0].flat[::5] = 32767
    model[0][1].flat[::5] = -32768
    cases, want = [], []
    for i in range(600):
        L = 8 + i % 25
        o = _random_oligo(rng, L, rng.choice((0.0, 0.2, 0.7)))
        w = "".join(rng.choice(sorted(H.IUPAC[c])) if rng.random() < 0.8 else rng.choice("ACGT") for c in o)
        strand = rng.randrange(2)
        if strand:
            w = H.revcomp(w.encode()).decode()
        cases.append(f"{w} {o} {strand} {rng.randrange(0, 100)}")
        P = H.strands(o)[strand]
        want.append(TH.site_sums_loop(o, w, strand, model) + (sum(c not in s for c, s in zip(w, P)),))
    head = " ".join(str(int(v)) for a in model for v in np.asarray(a).reshape(-1))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(tmp_path / "olt_core")], input=head + "\n" + "\n".join(cases) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.split("\n") if line]
    assert len(got) == len(want)
    for g, w, c in zip(got, want, cases):
        assert g[:3] == w[:3] and g[3] == w[2] and g[4] == w[3], c
