"""CPU: the specification of the oligo search with indels as tests/tools/oligo_edit_host.py restates it
-- its two forms against each other, hand-made cases with every field written out, max_edits = 0 against the Hamming restatement --,
`amplicons` on a bulged site, and the refusals of `check_oligos`.  No device is touched."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import oligo_edit_host as E  # noqa: E402
import oligo_host as H  # noqa: E402

from seqwin_amd import oligos as O  # noqa: E402

IUPAC = "ACGTRYSWKMBDHVN"


def _both(oligos, asms, d, c=0):
    a, b = E.sites_matrix(oligos, asms, d, c), E.sites_literal(oligos, asms, d, c)
    assert a == b
    return a


# ---- the two forms against each other ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alphabet", ["AC", "ACGT"])
def test_the_two_forms_agree_on_random_text(alphabet):
    rng = random.Random(len(alphabet))
    total = 0
    for it in range(60):
        d, c = rng.randrange(0, 5), rng.randrange(0, 9)
        L = rng.randrange(max(8, d + c + 1), 21)
        recs = ["".join(rng.choice(alphabet + ("N" if rng.random() < 0.02 else "")) for _ in range(rng.randrange(1, 120))).encode() for _ in range(2)]
        oligos = []
        for _ in range(3):
            t = recs[0].decode().replace("N", "A")
            o = list(t[:L]) if len(t) >= L and rng.random() < 0.6 else [rng.choice(alphabet) for _ in range(L)]
            if len(o) < L:
                o += [rng.choice(alphabet) for _ in range(L - len(o))]
            for _ in range(rng.randrange(0, 3)):
                o[rng.randrange(L)] = rng.choice(IUPAC)
            oligos.append("".join(o))
        total += len(_both(oligos, [recs, [recs[1][::-1]]], d, c))
    assert total > 100


# ---- hand-made cases: (oligo, assembly, record, pos, end, strand, dist, mismatch, gaps) ---------------------------------------------------

P12 = "ACGGTCATTGCA"


def test_a_one_base_text_bulge():
    """The text holds the oligo with a G more after ACGGTC: ACGGTC G ATTGCA, at 3..16.  The walk from (12, 16): six `=`, a `D` (the text's
    extra base), six `=`: pos 3, end 16, no mismatch, one gap."""
    assert _both([P12], [[b"TTT" + b"ACGGTCGATTGCA" + b"TTT"]], 1) == [(0, 0, 0, 3, 16, 0, 1, 0, 1)]


def test_a_one_base_oligo_bulge():
    """The text lacks the oligo's A at 6 (ACGGTC A TTGCA -> ACGGTCTTGCA, 11 bases at 2..13).  The walk from (12, 13): five `=` (TTGCA);
    at (7, 8) the oligo's A faces C, `=` fails; `X` needs D[6][7] + 1 == D[7][8], but D[6][7] = 1 (ACGGTC against a text that ends in
    ...ACGGT) and D[7][8] = 1; `I` needs D[6][8] + 1 == 1 and D[6][8] = 0: an `I`; then six `=`: pos 2, end 13, one gap."""
    rows = _both([P12], [[b"GG" + b"ACGGTCTTGCA" + b"GG"]], 1)
    assert rows == [(0, 0, 0, 2, 13, 0, 1, 0, 1)]


def test_a_bulge_next_to_the_clamp():
    """c = 3: Q = ACGGTCATT, the clamp GCA must face the end's last three bases exactly.  The text has a base more just before them
    (ACGGTCATT C GCA): E(16) = D[9][13] = 1 -- the extra C is a `D` as the walk's first step.  With the extra base inside the clamp
    (ACGGTCATTG C CA) no end is a site."""
    assert _both([P12], [[b"TTT" + b"ACGGTCATTCGCA" + b"TTT"]], 1, 3) == [(0, 0, 0, 3, 16, 0, 1, 0, 1)]
    assert _both([P12], [[b"TTT" + b"ACGGTCATTGCCA" + b"TTT"]], 1, 3) == []
    assert len(_both([P12], [[b"TTT" + b"ACGGTCATTGCCA" + b"TTT"]], 1, 0)) == 1


def test_a_plateau_yields_its_first_end():
    """ACGTACGT in ...ACGTACGTT...: D(e) at the exact end 11 is 0; with d = 1 the ends 10 and 12 have D = 1 and are not sites (a better
    end lies within d).  In AAAAAAAAAA (ten As) the 8-mer AAAAAAAA has D = 0 at the ends 8, 9, 10: the first of the plateau is the site."""
    assert _both(["ACGTACGT"], [[b"GGG" + b"ACGTACGT" + b"TGG"]], 1)[0][3:] == (3, 11, 0, 0, 0, 0)
    rows = [r for r in _both(["AAAAAAAA"], [[b"CC" + b"A" * 10 + b"CC"]], 1) if r[5] == 0]
    assert rows == [(0, 0, 0, 2, 10, 0, 0, 0, 0)]


def test_tandem_copies_d_apart_yield_one_site_each():
    """Two copies of ACGGTCATTGCA with d = 2 and two bases between them: ends 12 and 26, each a strict minimum of its own
    neighbourhood of d ends."""
    rows = _both([P12], [[P12.encode() + b"TT" + P12.encode()]], 2)
    assert [r[3:] for r in rows if r[5] == 0] == [(0, 12, 0, 0, 0, 0), (14, 26, 0, 0, 0, 0)]


def test_sites_cut_by_the_runs_bounds():
    """A run that starts inside the oligo's copy (its first base missing): the site starts at the run's start with an `I`.  A run that
    ends one base early: the last base is an `I` too, and the site's end is the run's end.  An N bounds a run as a record's end does."""
    rows = _both([P12], [[b"CGGTCATTGCA" + b"TTTT"]], 1)
    assert rows == [(0, 0, 0, 0, 11, 0, 1, 0, 1)]
    rows = _both([P12], [[b"TTTT" + b"ACGGTCATTGC"]], 1)
    assert rows == [(0, 0, 0, 4, 15, 0, 1, 0, 1)]
    rows = _both([P12], [[b"TTTT" + b"ACGGTCATTGC" + b"N" + b"CGGTCATTGCA"]], 1)
    assert rows == [(0, 0, 0, 4, 15, 0, 1, 0, 1), (0, 0, 0, 16, 27, 0, 1, 0, 1)]


def test_a_strand_1_site_and_its_clamp():
    """The text holds the reverse complement of the oligo with a base more.  Strand 1 is strand 0 on the reverse complement of the
    run, mapped back: the 3' clamp faces the site's FIRST bases, and a plateau resolves toward them."""
    rc = H.revcomp(b"ACGGTCGATTGCA")                                # the bulged copy of test_a_one_base_text_bulge
    assert _both([P12], [[b"TTT" + rc + b"TTT"]], 1) == [(0, 0, 0, 3, 16, 1, 1, 0, 1)]
    assert _both([P12], [[b"TTT" + rc + b"TTT"]], 1, 4) == [(0, 0, 0, 3, 16, 1, 1, 0, 1)]
    broken = bytearray(rc)
    broken[1] = ord("A") if rc[1:2] != b"A" else ord("C")           # a mismatch inside the clamp: the 3' end is the site's start
    assert _both([P12], [[b"TTT" + bytes(broken) + b"TTT"]], 2, 4) == []


def test_a_palindrome_gives_two_sites_at_one_place():
    pal = "ACGTTGCATGCAACGT"
    assert H.revcomp(pal.encode()) == pal.encode()
    assert _both([pal], [[b"TT" + pal.encode() + b"TT"]], 1) == [(0, 0, 0, 2, 18, 0, 0, 0, 0), (0, 0, 0, 2, 18, 1, 0, 0, 0)]


def test_the_rule_order_decides_a_tie():
    """AAAAAAAC against the text AAAAAAC (one A less): a cheapest alignment may lose its `I` at any of the seven As.  The canonical walk
    takes `=` wherever the bases match and meets the gap last, at the oligo's FIRST base: pos is the run's start.  Against GAAAAAAC the
    first cell where `=` fails offers `X` (A against G) and `I` at the same cost; `X` comes first in the rule order: one mismatch, no
    gap, pos 0 -- with `I` before `X` the site would read pos 1, gaps 1."""
    assert _both(["AAAAAAAC"], [[b"AAAAAAC"]], 1) == [(0, 0, 0, 0, 7, 0, 1, 0, 1)]
    assert _both(["AAAAAAAC"], [[b"GAAAAAAC"]], 1) == [(0, 0, 0, 0, 8, 0, 1, 1, 0)]


# ---- max_edits = 0 is the Hamming search with no mismatch ----------------------------------------------------------------------------

@pytest.mark.parametrize("clamp", [0, 4])
def test_no_edits_is_the_hamming_form(clamp):
    rng = random.Random(3)
    recs = [bytes(rng.choice(b"ACGTN" if rng.random() < 0.03 else b"AC") for _ in range(400)) for _ in range(3)]
    oligos = ["ACACACAC", "AACCAACCA", "ACNNRYAC", "CCCCAAAACCCC", recs[0][50:70].decode().replace("N", "A")]
    asms = [[recs[0], recs[1]], [recs[2]]]
    ham = H.sites_loop(oligos, asms, 0, clamp)
    got = E.sites_matrix(oligos, asms, 0, clamp)
    assert len(ham) > 10
    assert [(q, a, r, p, s) for q, a, r, p, e, s, v, nx, ng in got] == [(q, a, r, p, s) for q, a, r, p, s, mm in ham]
    assert all(e == p + len(oligos[q]) and v == nx == ng == 0 for q, a, r, p, e, s, v, nx, ng in got)


# ---- amplicons with a bulged site ------------------------------------------------------------------------------------------------------

def test_amplicons_with_a_bulged_site():
    """f binds [10, 31) with a text bulge (21 bases for 20 letters), r binds on strand 1 with an oligo bulge ([100, 119)): the product is
    [10, 119) -- its end is the site's end, not pos + L --, and the bounds are applied to that length."""
    S = {f: np.array(v, np.uint32) for f, v in dict(oligo=[0, 1], assembly=[0, 0], record=[0, 0], pos=[10, 100], end=[31, 119], strand=[0, 1],
                                                  dist=[1, 1], mismatch=[0, 0], gaps=[1, 1]).items()}
    P, n = O.amplicons(S, [20, 20], [(0, 1)], 109, 109, n_assemblies=1)
    assert [int(P[f][0]) for f in O.AMPLICON_FIELDS] == [0, 0, 0, 10, 119, 0, 1, 1] and n.tolist() == [[1]]
    assert O.amplicons(S, [20, 20], [(0, 1)], 110, 200, n_assemblies=1)[1].tolist() == [[0]]      # (pos + L would have given 120)
    assert O.amplicons(S, [20, 20], [(0, 1)], 50, 108, n_assemblies=1)[1].tolist() == [[0]]
    old = {f: S[f] for f in ("oligo", "assembly", "record", "pos", "strand")}
    old["mm"] = S["dist"]
    P, n = O.amplicons(old, [20, 20], [(0, 1)], 110, 200, n_assemblies=1)                          # without `end`: as before
    assert int(P["end"][0]) == 120
    s = O.oligo_summary(dict(n_sites=np.array([[1, 0]]), best_dist=np.array([[1, 0xFFFFFFFF]])), 1)
    assert s["f_tar"].tolist() == [1.0] and s["mean_best_mm_tar"].tolist() == [1.0]


# ---- the refusals ---------------------------------------------------------------------------------------------------------------------

def test_check_oligos_refusals():
    ok = ["ACGTACGT", "ACGTACGTACGT"]
    assert O.check_oligos(ok, 0, 3, 4) == [b"ACGTACGT", b"ACGTACGTACGT"]
    assert O.check_oligos(ok, 2, 3) == O.check_oligos(ok, 2, 3, None)
    for kw, what in ((dict(max_edits=5), "max_edits"), (dict(max_edits=-1), "max_edits"), (dict(max_edits=1.5), "max_edits"),
                     (dict(max_edits=4, three_prime=4), "below the shortest"), (dict(max_edits=0, three_prime=8), "below the shortest"),
                     (dict(max_edits=1, max_mismatch=1), "exclude"), (dict(max_edits=0, max_mismatch=2), "exclude"),
                     (dict(max_edits=1, three_prime=9), "three_prime")):
        with pytest.raises(ValueError, match=what):
            O.check_oligos(ok, **kw)
    with pytest.raises(ValueError, match="letters"):
        O.check_oligos(["ACGTACG"], max_edits=1)


# ---- the kernels' arithmetic on the CPU ----------------------------------------------------------------------------------------------------

def test_the_kernels_arithmetic_on_the_host(tmp_path):
    """seqwin_amd/csrc/oligo_edit_core.hpp -- what a lane of k_ole_scan and a thread of k_ole_resolve compute -- compiled for the host
    with tests/tools/oligo_edit_core_driver.cpp (AddressSanitizer + UBSan where g++ links them) and run lane by lane over random runs:
    lengths around k, the lane's 16 and the tile's 1024, 2- and 4-letter text, IUPAC oligos of 8..32 with substitutions, insertions and
    deletions, d 0..4, c 0..8, k below L (another oligo of the call is shorter), any alignment of the run in its packed words.  Every
    site and every field against the NumPy form of the restatement."""
    import subprocess
    src = [str(ROOT / "tests" / "tools" / "oligo_edit_core_driver.cpp"), "-I", str(ROOT / "seqwin_amd" / "csrc"), "-o", str(tmp_path / "ole_core")]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    if subprocess.run(["g++", "-std=c++17"] + san + src, capture_output=True).returncode != 0:
        subprocess.run(["g++", "-std=c++17", "-O2"] + src, check=True, capture_output=True)
    rng = random.Random(77)
    cases, want = [], []
    while len(cases) < 400:
        alpha = rng.choice(["AC", "ACGT", "ACGT", "AT"])
        L, d, c = rng.choice([8, 9, 12, 17, 20, 31, 32]), rng.randrange(0, 5), rng.randrange(0, 9)
        lmins = [x for x in (8, L - 3, L) if 8 <= x <= L and d + c < x]
        if not lmins:
            continue
        k = rng.choice(lmins) - d
        n = rng.choice([max(k - 1, 1), k, k + 1, 15, 16, 17, 40, 100, 300, 1040, 1100])
        T = "".join(rng.choice(alpha) for _ in range(n))
        if rng.random() < 0.7 and n > L + 6:
            at = rng.randrange(0, n - L - 4)
            o = list(T[at:at + L] if rng.random() < 0.5 else E._rc(T[at:at + L]))
        else:
            o = [rng.choice(alpha) for _ in range(L)]
        for _ in range(rng.randrange(0, 4)):
            r, i = rng.random(), rng.randrange(len(o))
            if r < 0.3:
                o[i] = rng.choice(IUPAC)
            elif r < 0.6 and len(o) > 8:
                del o[i]
            elif len(o) < 32:
                o.insert(i, rng.choice(alpha))
        o = "".join(o)
        if d + c >= len(o) or len(o) < k + d:
            continue
        cases.append(f"{T} {o} {d} {c} {k} {rng.randrange(0, 40)}")
        rows = []
        for s, t in enumerate((T, E._rc(T))):
            for b, e, v, nx, ng in E.run_sites_matrix(E.sets_of(o), t, d, c):
                rows.append((s,) + ((b, e) if s == 0 else (n - e, n - b)) + (v, nx, ng))
        want.append(sorted(rows))
    env = dict(__import__("os").environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(tmp_path / "ole_core")], input="\n".join(cases) + "\n", capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    got = []
    for line in r.stdout.split("\n"):
        if line.startswith("case"):
            got.append([])
        elif line:
            got[-1].append(tuple(int(x) for x in line.split()))
    assert len(got) == len(want) and sum(len(w) for w in want) > 1000
    for i, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == w, cases[i]
