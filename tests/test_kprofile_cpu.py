"""CPU: the two host restatements of the k-mer profile (tests/tools/kprofile_host.py) against each other and
against hand-made tables written out here; seqwin_amd/kprofile.py (fraction, window_bounds, specific_positions, repeat_positions)
against its restatement and on small tables with nan and sentinel rows; and the ctypes table against the header's new entry points.
The device side (seqwin_amd/csrc/screen.hip) is compared with the same restatement in tests/test_gpu_kprofile.py."""
import random
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import kprofile_host as H  # noqa: E402

from seqwin_amd import kprofile as K  # noqa: E402

NW, NWC = H.NO_WINDOW, H.NO_WINDOW_COPIES
KS = [1, 2, 3, 15, 16, 21, 31, 32]


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _revcomp(s: bytes) -> bytes:
    return s.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def _both(queries, asms, k, labels, n_groups=None):
    a = H.profile_literal(queries, asms, k, labels, n_groups)
    b = H.profile_words(queries, asms, k, labels, n_groups)
    for x, y, dt in zip(a, b, (np.uint64, np.uint32, np.uint64, np.uint32)):
        assert x.dtype == dt and y.dtype == dt and x.shape == y.shape
        assert np.array_equal(x, y)
    return a


@pytest.mark.parametrize("k", KS)
def test_the_two_forms_agree_on_random_text(k):
    rng = random.Random(500 + k)
    anc = _rand(rng, 500)
    rec = bytearray(anc[:300])
    rec[40:41] = b"N"
    rec[90:130] = bytes(rec[90:130]).lower()
    asms = [[bytes(rec).replace(b"T", b"U", 3), anc[300:]], [_rand(rng, 300)], [anc[100:400], _rand(rng, max(k - 1, 0))],
            [_revcomp(anc[:250]), anc[:250]], []]
    queries = [anc[50:50 + 3 * k + 7], _revcomp(anc[200:260 + k]), b"", anc[10:10 + k - 1], anc[35:45 + k].lower().replace(b"t", b"u"),
               anc[100:100 + k] + b"N" + anc[100 + k:100 + 2 * k], anc[50:50 + 3 * k + 7], "".join(chr(c) for c in anc[150:150 + k + 9])]
    for labels, ng in (([0, 1, 255, 0, 1], None), ([0, 7, 7, 0, 255], 8), ([255] * 5, None), ([0] * 5, 1)):
        offs, present, copies, sizes = _both(queries, asms, k, labels, ng)
        assert offs[-1] == sum(len(q) for q in queries) and present.shape == (int(offs[-1]), len(sizes))
        assert sizes.tolist() == [sum(1 for x in labels if x == g) for g in range(len(sizes))]
        window = present[:, 0] != NW
        assert np.array_equal(window, copies[:, 0] != NWC)
        assert np.all(present[~window] == NW) and np.all(copies[~window] == NWC)
        assert np.all(copies[window] >= present[window]) and np.array_equal(copies[window] == 0, present[window] == 0)
        o = offs.astype(np.int64)
        assert np.array_equal(present[o[0]:o[1]], present[o[6]:o[7]])                      # a query given twice
        assert np.all(present[o[3]:o[4]] == NW)                                              # shorter than k
        for q in range(len(queries)):                                                         # the last k - 1 bytes of a query
            assert np.all(present[max(o[q], o[q + 1] - (k - 1)):o[q + 1]] == NW)
        assert np.all(present[window] <= sizes[None, :])


# name, k, queries, assemblies, labels, n_groups, present rows, copies rows (per query position; "-" = no window)
_ = "-"
HAND = [
    # AAC (= GTT): in target 0 (AAC) and target 1 (GTT), not in target 2; twice in non-target 3.  ACC (= GGT): in target 1 only
    ("present in two of three targets and twice in one non-target", 3, ["AACC"],
     [["TTAACT"], ["GGGTTG"], ["CCCC"], ["AACAAC"], ["TTTT"]], [0, 0, 0, 1, 1], None,
     [[2, 1], [1, 0], _, _], [[2, 2], [1, 0], _, _]),
    # ACGT is its own reverse complement: one window is one copy -- ACGTACGT holds it twice, TTACGTTT once.  TACG = CGTA: the first
    # assembly holds CGTA and TACG, the second TACG
    ("a palindromic k-mer", 4, ["ACGT", "TACGT"], [["ACGTACGT"], ["TTACGTTT"], ["ACGA"]], [0, 0, 1], None,
     [[2, 0], _, _, _, [2, 0], [2, 0], _, _, _], [[3, 0], _, _, _, [3, 0], [3, 0], _, _, _]),
    # the window that holds the N has no row; the windows on either side do
    ("a query window with an N", 2, ["ACNGT"], [["ACGT"], ["GGTT"]], [0, 1], None,
     # AC (= GT): asm 0 twice (AC, GT), asm 1 once (GT).  GT the same word
     [[1, 1], _, _, [1, 1], _], [[2, 1], _, _, [2, 1], _]),
    # ACGTACGTA holds ACGTA twice and its reverse complement TACGT once
    ("a query shorter than k", 5, ["ACGT", "", "ACGTA"], [["ACGTACGTA"], ["TTTTT"]], [0, 1], None,
     [_, _, _, _, [1, 0], _, _, _, _], [_, _, _, _, [3, 0], _, _, _, _]),
    # CCA = TGG in both queries; GGA = TCC in neither assembly
    ("two queries sharing a k-mer", 3, ["CCA", "TTGGA"], [["ACCAT"], ["TGGTGG"], ["AAAA"]], [0, 1, 1], None,
     # CCA: asm 0 once, asm 1 twice.  TTG = CAA: nowhere.  TGG = CCA.  GGA: nowhere
     [[1, 1], _, _, [0, 0], [1, 1], [0, 0], _, _], [[1, 2], _, _, [0, 0], [1, 2], [0, 0], _, _]),
    ("an assembly labelled 255", 2, ["AG"], [["AG"], ["AGAG"], ["CT"]], [0, 255, 1], None,
     [[1, 1], _], [[1, 1], _]),
    # labels 0 and 2 with three groups: group 1 is empty and reads 0 where a window starts
    ("an empty group", 2, ["AG"], [["AG"], ["CTCT"]], [0, 2], 3,
     [[1, 0, 1], _], [[1, 0, 2], _]),
]


def _rows(rows, ng, sentinel, dtype):
    return np.array([[sentinel] * ng if r == "-" else r for r in rows], dtype).reshape(len(rows), ng)


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_made_tables(case):
    _, k, queries, asms, labels, ng, present, copies = case
    for fn in (H.profile_literal, H.profile_words):
        offs, p, c, sizes = fn(queries, asms, k, labels, ng)
        assert offs.tolist() == np.concatenate(([0], np.cumsum([len(q) for q in queries]))).tolist(), fn.__name__
        assert p.tolist() == _rows(present, len(sizes), NW, np.uint32).tolist(), fn.__name__
        assert c.tolist() == _rows(copies, len(sizes), NWC, np.uint64).tolist(), fn.__name__
        assert sizes.tolist() == [sum(1 for x in labels if x == g) for g in range(len(sizes))]


def test_degenerate_shapes_and_refused_arguments():
    for fn in (H.profile_literal, H.profile_words):
        offs, p, c, sizes = fn([], [["ACGT"]], 3, [0])
        assert offs.tolist() == [0] and p.shape == (0, 1) and c.shape == (0, 1) and sizes.tolist() == [1]
        offs, p, c, sizes = fn(["ACGT"], [], 3, [])
        assert p.tolist() == [[0], [0], [NW], [NW]] and sizes.tolist() == [0]
        offs, p, c, sizes = fn(["ACGT"], [["ACGT"], ["ACGT"]], 3, [255, 255])
        assert p.tolist() == [[0], [0], [NW], [NW]] and c.tolist() == [[0], [0], [NWC], [NWC]] and sizes.tolist() == [0]
        for k in (0, 33):
            with pytest.raises(ValueError):
                fn(["ACGT"], [["ACGT"]], k, [0])
        for labels, ng in (([3], 3), ([254], None), ([0], 0), ([0], 9), ([0, 0], None)):
            with pytest.raises(ValueError):
                fn(["ACGT"], [["ACGT"]], 3, labels, ng)


# ---- seqwin_amd/kprofile.py ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """Three targets and three non-targets over one ancestor; two queries cut from it, one with an N."""
    rng = random.Random(77)
    anc = _rand(rng, 400)
    asms = []
    for g in range(6):
        seq = bytearray(anc)
        for _ in range(6 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([bytes(seq[:220]), bytes(seq[220:]) + (anc[30:60] if g % 2 else b"")])   # (a repeat in every other assembly)
    queries = [anc[20:120], anc[200:260][:30] + b"N" + anc[231:260], _revcomp(anc[300:380])]
    labels = [0, 0, 0, 1, 1, 1]
    return queries, asms, labels


@pytest.mark.parametrize("k", [8, 12])
def test_window_bounds(planted, k):
    queries, asms, labels = planted
    offs, present, copies, sizes = H.profile_words(queries, asms, k, labels)
    t = K.Table(offs, present, copies, sizes, k)
    assert np.array_equal(K.window_bounds(t, k), present)                           # length == k: the table itself
    text = b"".join(queries)
    o = offs.astype(np.int64)
    for length in (k, k + 1, k + 5, 20):
        got = K.window_bounds(t, length)
        assert got.dtype == np.uint32 and np.array_equal(got, H.window_bounds(offs, present, k, length))
        for q in range(len(queries)):
            assert np.all(got[max(o[q], o[q + 1] - length + 1):o[q + 1]] == NW)     # the window leaves the query
            for p in range(o[q], o[q + 1] - length + 1):
                w = text[p:p + length]
                if b"N" in w:
                    assert np.all(got[p] == NW)
                    continue
                exact = H.count_exact(w, asms, labels, 2)                           # by string search in the assemblies
                assert np.all(got[p] >= exact)
                if length == k:
                    assert got[p].tolist() == exact
    with pytest.raises(ValueError):
        K.window_bounds(t, k - 1)


def test_functions_on_small_tables():
    offs = np.array([0, 4, 4, 7], np.uint64)
    present = np.array([[4, 0, 0], [3, 1, 0], [NW] * 3, [0, 2, 0], [2, 0, 0], [NW] * 3, [4, 1, 0]], np.uint32)
    copies = np.array([[4, 0, 0], [7, 1, 0], [NWC] * 3, [0, 4, 0], [2, 0, 0], [NWC] * 3, [8, 1, 0]], np.uint64)
    sizes = np.array([4, 2, 0], np.uint32)
    t = K.Table(offs, present, copies, sizes, 3)
    f = K.fraction(t)
    assert f.dtype == np.float64 and np.array_equal(f, H.fraction(present, sizes), equal_nan=True)
    assert f[0].tolist()[:2] == [1.0, 0.0] and f[1, 0] == 0.75 and f[1, 1] == 0.5
    assert np.isnan(f[2]).all() and np.isnan(f[5]).all() and np.isnan(f[:, 2]).all()        # sentinel rows, the empty group
    # group 0 against group 1: rows 0 (1.0, 0) and 4 (0.5 fails 0.95); row 6 holds 1 of 2 non-targets
    assert K.specific_positions(t).tolist() == [0] == H.specific_positions(present, sizes).tolist()
    assert K.specific_positions(t, min_tar=0.5).tolist() == [0, 4]
    assert K.specific_positions(t, min_tar=0.5, max_neg=0.5).tolist() == [0, 1, 4, 6] == H.specific_positions(present, sizes, 0, 1, 0.5, 0.5).tolist()
    # the empty group as the non-target group reads f_neg = 0; as the target group it passes nothing
    assert K.specific_positions(t, tar=0, neg=2, min_tar=0.75).tolist() == [0, 1, 6] == H.specific_positions(present, sizes, 0, 2, 0.75).tolist()
    assert K.specific_positions(t, tar=2, neg=1).tolist() == [] == H.specific_positions(present, sizes, 2, 1).tolist()
    # copies / present: rows 1 (7 / 3), 6 (8 / 4) in group 0; row 3 (4 / 2) in group 1
    assert K.repeat_positions(t, 0).tolist() == [1, 6] == H.repeat_positions(present, copies, 0).tolist()
    assert K.repeat_positions(t, 0, min_mean_copies=2.1).tolist() == [1]
    assert K.repeat_positions(t, 1).tolist() == [3] and K.repeat_positions(t, 2).tolist() == []
    assert K.repeat_positions(t, 0, 1.0).tolist() == [0, 1, 4, 6] == H.repeat_positions(present, copies, 0, 1.0).tolist()
    with pytest.raises(ValueError, match="copies"):
        K.repeat_positions(K.Table(offs, present, None, sizes, 3), 0)
    for bad in (3, -1):
        with pytest.raises(ValueError):
            K.repeat_positions(t, bad)
        with pytest.raises(ValueError):
            K.specific_positions(t, tar=bad)
    # window_bounds over the sentinel rows: query 0 has windows at 0, 1, 3 -- a window of 4 covers rows 0 and 1; query 2 (rows 4..6)
    # has none of length 5 that avoids row 5
    wb = K.window_bounds(t, 4)
    assert wb[0].tolist() == [3, 0, 0] and np.all(wb[1:] == NW)
    assert np.array_equal(wb, H.window_bounds(offs, present, 3, 4))
    with pytest.raises(ValueError):
        K.Table(offs, present[:5], None, sizes, 3)


def test_functions_agree_with_their_restatement_on_a_planted_case(planted):
    queries, asms, labels = planted
    offs, present, copies, sizes = H.profile_literal(queries, asms, 10, labels)
    t = K.Table(offs, present, copies, sizes, 10)
    assert np.array_equal(K.fraction(t), H.fraction(present, sizes), equal_nan=True)
    for args in ((0, 1, 0.95, 0.05), (0, 1, 0.6, 0.4), (1, 0, 0.3, 1.0)):
        assert K.specific_positions(t, *args).tolist() == H.specific_positions(present, sizes, *args).tolist()
    assert len(K.specific_positions(t, 0, 1, 0.6, 0.7)) > 0
    for g in (0, 1):
        assert K.repeat_positions(t, g, 1.3).tolist() == H.repeat_positions(present, copies, g, 1.3).tolist()
    assert len(K.repeat_positions(t, 1, 1.3)) > 0                                     # the planted repeat anc[30:60] lies in query 0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_abi_declares_the_profile_entry_points():
    """seqwin_amd/_abi.py declares every entry point of the header (read as tests/test_abi_cpu.py reads it), the four new ones among
    them, each documented as having no counterpart in the reference; the library exports them."""
    from ctypes import c_char_p, c_int, c_uint64, c_void_p

    from seqwin_amd._abi import PROTOTYPES
    from seqwin_amd._lib import lib
    header = (ROOT / "include" / "seqwin_hip.h").read_text()
    declared = set(re.findall(r"\b(sw_[a-z_0-9]+)\s*\(", header))
    assert set(PROTOTYPES) == declared
    new = {
        "sw_batch_screen_profile": (c_int, [c_void_p, c_void_p, c_char_p, c_uint64, c_uint64, c_void_p, c_uint64, c_int, c_void_p, c_void_p]),
        "sw_screen_profile_sizes": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
        "sw_screen_profile_export": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
        "sw_screen_profile_stats": (c_int, [c_void_p, c_void_p, c_void_p]),
    }
    for name, (restype, argtypes) in new.items():
        assert name in declared and PROTOTYPES[name] == (restype, argtypes), name
        fn = getattr(lib, name)
        assert fn.restype == restype and list(fn.argtypes) == argtypes, name
        comment = header[:header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "(no counterpart in the reference)" in comment, name
        line = next(ln for ln in (ROOT / "seqwin_amd" / "_abi.py").read_text().splitlines() if f'"{name}"' in ln)
        assert line.endswith("# (no counterpart in the reference)"), name
    # the profile getters refuse a NULL handle without a device
    for name in ("sw_screen_profile_sizes", "sw_screen_profile_export", "sw_screen_profile_stats"):
        assert getattr(lib, name)(None, None, None, *([None] if len(new[name][1]) == 4 else [])) == 2, name
