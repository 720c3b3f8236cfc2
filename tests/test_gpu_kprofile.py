"""GPU: the k-mer profile of csrc/screen.hip (Batch.screen(profile=...), Markers.screen(profile=...), Screen.profile()) against the
host restatement of its specification (tests/tools/kprofile_host.py) on the same text: every array compared
whole.  k_scr_profile gives a lane one bitmap word (32 k-mer numbers) of every row, a wave 64 consecutive words, a workgroup 256; a
lane's bit-sliced counters take PLANE_ROWS rows before they are emptied, a workgroup SLICE_ROWS rows of a chunk in group order; query
sizes, assembly counts and labels straddle all of these."""
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import kprofile_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
NW, NWC = H.NO_WINDOW, H.NO_WINDOW_COPIES
PLANE_ROWS = 255     # csrc/screen.hip PRF_FLUSH: 8 counter planes hold 255 rows, the 256th row finds them emptied
SLICE_ROWS = 1024    # csrc/screen.hip PRF_SLICE: the rows of one workgroup


@pytest.fixture(scope="module", autouse=True)
def _device():
    from seqwin_amd.device import set_device
    set_device(0)


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _revcomp(s: bytes) -> bytes:
    return s.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d some text\n" % (name.encode(), i))
            r = bytes(r)
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def _batch(d, assemblies, tag="a"):
    from seqwin_amd.device import Batch
    return Batch.from_fasta([_write(d, f"{tag}{i}.fa", recs) for i, recs in enumerate(assemblies)], n_cpu=2)


def _check(batch, queries, assemblies, k, labels, n_groups=None, copies=True, want=None, plain=True):
    """Screen with a profile and compare every array with the restatement (and the screen's own answers with a call without a
    profile); returns (present, copies or None, screen stats, profile stats)."""
    w_offs, w_present, w_copies, w_sizes = want if want is not None else H.profile_words(queries, assemblies, k, labels, n_groups)
    s = batch.screen(queries, k, profile=labels, n_groups=n_groups, copies=copies)
    try:
        p = s.profile()
        offs, present, cop = p.table()
        assert offs.dtype == np.uint64 and np.array_equal(offs, w_offs)
        assert present.dtype == np.uint32 and present.shape == w_present.shape and np.array_equal(present, w_present)
        assert np.array_equal(p.group_sizes(), w_sizes) and p.group_sizes().dtype == np.uint32
        assert p.sizes() == (int(w_offs[-1]), len(w_sizes), bool(copies)) and p.k == k
        if copies:
            assert cop.dtype == np.uint64 and np.array_equal(cop, w_copies)
        else:
            assert cop is None
            with pytest.raises(ValueError, match="copies"):
                p.copies(0)
        o = w_offs.astype(np.int64)
        for q in range(len(queries)):
            assert np.array_equal(p.present(q), w_present[o[q]:o[q + 1]])
            if copies:
                assert np.array_equal(p.copies(q), w_copies[o[q]:o[q + 1]])
        with pytest.raises(ValueError):
            p.present(len(queries))
        st, pst = s.stats(), p.stats()
        assert pst["table_bytes"] > 0 and pst["profile_ms"] >= 0 and pst["gather_ms"] >= 0
        if copies:   # one add per hit in an assembly that is not left out
            assert 0 <= pst["copy_adds"] <= st["hits"]
            if 255 not in [int(x) for x in labels]:
                assert pst["copy_adds"] == st["hits"]
        else:
            assert pst["copy_adds"] == 0
        if plain:   # a call without profile= answers the same counts, bit for bit
            s0 = batch.screen(queries, k)
            try:
                assert np.array_equal(s.counts(), s0.counts()) and np.array_equal(s.n_kmers(), s0.n_kmers()) and s.sizes() == s0.sizes()
                assert np.array_equal(s.containment(), s0.containment(), equal_nan=True)
                with pytest.raises(ValueError, match="profile"):
                    s0.profile()
            finally:
                s0.close()
        return present, cop, st, pst
    finally:
        s.close()


# ---- k sweep (tests/test_release_library_kprofile.py runs this and the invariants on the release library) ---------------------------

def _sweep_case(k):
    rng = random.Random(40 + k)
    anc = _rand(rng, 900)
    r0 = bytearray(anc[:400])
    r0[60:61] = b"N"
    r0[150:150 + k] = b"N" * k
    r0[200:260] = bytes(r0[200:260]).lower()
    asms = [[bytes(r0).replace(b"T", b"U", 4), anc[400:700], _rand(rng, max(k - 1, 1))],
            [_rand(rng, 300), anc[650:900]],
            [anc[100:500], _rand(rng, 200) + b"NNNN" + anc[300:330]],
            [_revcomp(anc[:350]), anc[:k - 1] if k > 1 else b"N", anc[500:800]],
            [anc[200:450] + b"N" * 7 + anc[200:450], _rand(rng, 250)]]
    twice = anc[40:40 + 3 * k + 30]
    queries = [twice, b"", anc[10:10 + k - 1], anc[300:300 + k] + b"R" + anc[300 + k:300 + 2 * k + 5], twice,
               anc[640:700 + k].lower().replace(b"t", b"u"), _revcomp(anc[380:430 + k]), _rand(rng, 60), anc[200:200 + k]]
    return queries, asms


@pytest.mark.parametrize("k", [1, 2, 15, 16, 21, 31, 32])
def test_k_sweep(tmp_path, k):
    queries, asms = _sweep_case(k)
    b = _batch(tmp_path, asms)
    try:
        for labels, ng in (([0, 1, 255, 0, 1], None), ([0, 7, 7, 0, 7], 8)):
            want = H.profile_words(queries, asms, k, labels, ng)
            lit = H.profile_literal(queries, asms, k, labels, ng)
            assert all(np.array_equal(x, y) for x, y in zip(want, lit))
            present, cop, st, _ = _check(b, queries, asms, k, labels, ng, want=want)
            o = want[0].astype(np.int64)
            assert present.shape[1] == (2 if ng is None else 8)
            assert np.all(present[o[2]:o[3]] == NW) and np.all(cop[o[2]:o[3]] == NWC)          # shorter than k
            assert np.array_equal(present[o[0]:o[1]], present[o[4]:o[5]])                        # given twice
            assert np.all(present[o[3] + 1:o[3] + k + 1] == NW) and present[o[3], 0] != NW       # windows over the invalid byte
            window = present[:, 0] != NW
            assert window.sum() == st["query_kmers"]
            assert np.all(cop[window] >= present[window]) and np.array_equal(cop[window] == 0, present[window] == 0)
            if ng == 8:
                assert not present[window][:, 1:7].any()
    finally:
        b.close()


# ---- bitmap word and counter bounds ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def word_batch(tmp_path_factory):
    rng = random.Random(21)
    text = _rand(rng, 64 * 32 + 1 + 20)                       # 2049 distinct 21-mers
    asms = [[text], [text[:1000], text[1010:]], [_revcomp(text[500:1500])], [_rand(rng, 500)], [text[-60:], text[:40]]]
    b = _batch(tmp_path_factory.mktemp("kpw"), asms, "w")
    yield b, text, asms
    b.close()


@pytest.mark.parametrize("n", [31, 32, 33, 64 * 32 - 1, 64 * 32 + 1])
def test_bitmap_word_bounds(word_batch, n):
    """n distinct k-mers: the last bitmap word, and the last 64 words a wave loads, are partial (or just full, or just begun)."""
    b, text, asms = word_batch
    k = 21
    for q in (text[:n + k - 1], text[-(n + k - 1):]):
        present, cop, st, _ = _check(b, [q], asms, k, [0, 1, 1, 0, 2])
        assert st["distinct_kmers"] == n and present.shape == (n + k - 1, 3)
        assert present[n - 1, 0] == 1 and np.all(present[n:] == NW)


# ---- counter plane flush and row slices ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """1026 one-record assemblies of 42 bases that all hold one 21-mer; most also hold one of three other 21-mers."""
    rng = random.Random(8)
    shared = _rand(rng, 21)
    variants = [_rand(rng, 21) for _ in range(3)]
    asms = []
    for i in range(SLICE_ROWS + 2):
        asms.append([shared + (variants[i % 3] if i % 5 else _rand(rng, 21))])
    queries = [shared + b"N" + b"N".join(variants), asms[700][0]]
    b = _batch(tmp_path_factory.mktemp("kpm"), asms, "m")
    yield b, queries, asms
    b.close()


@pytest.mark.parametrize("n", [PLANE_ROWS - 1, PLANE_ROWS, PLANE_ROWS + 1, 260, 513, SLICE_ROWS - 1, SLICE_ROWS, SLICE_ROWS + 1])
def test_counter_plane_flush(many, n):
    """n assemblies in ONE group (the others left out, then in a second group): a lane's 8 planes count PLANE_ROWS = 255 rows and are
    emptied before the 256th; a workgroup takes SLICE_ROWS = 1024 rows.  One below, at and one above both, and 260 and 513."""
    b, queries, asms = many
    for rest in (255, 1):
        labels = [0] * n + [rest] * (len(asms) - n)
        present, cop, st, _ = _check(b, queries, asms, 21, labels, 2, plain=False)
        assert present[0].tolist() == [n, 0 if rest == 255 else len(asms) - n]


# ---- chunks, launch splits, table pressure -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """9 assemblies of two records each over one ancestor (a stretch of it twice in each), and queries with more than 3 * 256 * 32
    distinct 21-mers: four word tiles of k_scr_profile."""
    rng = random.Random(9)
    anc = _rand(rng, 12_000)
    asms = []
    for g in range(9):
        seq = bytearray(anc)
        for _ in range(40 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        asms.append([bytes(seq[:7000]), bytes(seq[7000:]) + _rand(rng, 200) + bytes(seq[100:400])])
    queries = [anc[i * 1000:i * 1000 + 1100] for i in range(8)] + [_revcomp(anc[8500:9500]), _rand(rng, 16_500)]
    labels = [0, 1, 1, 0, 255, 2, 2, 0, 1]      # (they change inside chunks of 2 and 3 rows and at their borders)
    b = _batch(tmp_path_factory.mktemp("kp9"), asms, "n")
    want = H.profile_words(queries, asms, 21, labels)
    yield b, queries, asms, labels, want
    b.close()


def test_chunks(nine, monkeypatch):
    b, queries, asms, labels, want = nine
    _, _, st, _ = _check(b, queries, asms, 21, labels, want=want)
    assert st["chunks"] == 1
    words = (st["distinct_kmers"] + 31) // 32
    assert words > 3 * 256 and 4 * words > 1024
    for rows in (3, 2):
        kb = -(-rows * 4 * words // 1024)                    # the smallest budget that holds `rows` rows
        assert kb * 1024 // (4 * words) == rows
        monkeypatch.setenv("SEQWIN_AMD_SCR_BITMAP_KB", str(kb))
        _, _, st, _ = _check(b, queries, asms, 21, labels, want=want)
        assert st["chunks"] == -(-9 // rows)
    monkeypatch.setenv("SEQWIN_AMD_SCR_BITMAP_KB", "0")     # a row per chunk (one chunk holds only the assembly left out)
    _, _, st, _ = _check(b, queries, asms, 21, labels, want=want)
    assert st["chunks"] == 9
    _check(b, queries, asms, 21, labels, want=want, copies=False)


@pytest.mark.parametrize("blocks", [1, 3])
def test_launch_splits(nine, monkeypatch, blocks):
    """Launches of 1 and of 3 workgroups: k_scr_profile has four word tiles here -- four launches, or a full and a partial one."""
    b, queries, asms, labels, want = nine
    monkeypatch.setenv("SEQWIN_AMD_SCR_MAX_BLOCKS", str(blocks))
    _, _, st, _ = _check(b, queries, asms, 21, labels, want=want, plain=False)
    assert st["launches"] > 1 and (st["distinct_kmers"] + 31) // 32 > 3 * 256


def test_launch_split_over_row_slices(many, monkeypatch):
    b, queries, asms = many
    monkeypatch.setenv("SEQWIN_AMD_SCR_MAX_BLOCKS", "1")
    labels = [i % 2 for i in range(len(asms))]
    present, _, _, _ = _check(b, queries, asms, 21, labels, plain=False)
    assert present[0].tolist() == [len(asms) // 2, len(asms) // 2]


def test_table_pressure(nine, monkeypatch):
    b, queries, asms, labels, want = nine
    d = len(np.unique(np.concatenate([w[ok] for w, ok in (H._words(q, 21) for q in queries)])))
    monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(d.bit_length()))      # the smallest legal table: long chains, the wrap
    _, _, st, _ = _check(b, queries, asms, 21, labels, want=want)
    assert st["table_capacity"] == 1 << d.bit_length() and st["longest_chain"] > 1


def test_tiny_table_wraps(tmp_path, monkeypatch):
    asms = [[b"ACGTTGCAAGGCTA"], [b"TTTTTTTTTT"], [b"CCTTGCAACGT", b"ACGTT"]]
    b = _batch(tmp_path, asms)
    try:
        for queries, k, bits in (([b"ACGTTGC"], 5, 2), ([b"ACGTTGC", b"GGCTA"], 4, 3), ([b"ACGTTGCAAGG"], 4, 3)):
            monkeypatch.setenv("SEQWIN_AMD_SCR_TABLE_BITS", str(bits))
            want = H.profile_literal(queries, asms, k, [0, 1, 0])
            _, _, st, _ = _check(b, queries, asms, k, [0, 1, 0], want=want)
            assert st["table_capacity"] == 1 << bits
    finally:
        b.close()


# ---- copies --------------------------------------------------------------------------------------------------------------------------

def test_copies(tmp_path):
    rng = random.Random(31)
    w = b"GATTACAGGCTCA"                                         # 13 bases, not its own reverse complement
    rc = _revcomp(w)
    pad = [_rand(rng, 30) for _ in range(8)]
    asms = [
        [pad[0] + w + pad[1] + w + pad[2] + w + pad[3], pad[4]],                 # three times in one record
        [pad[5] + w + pad[6] + rc + pad[7]],                                       # once on each strand
        [pad[0] + w[:7], w[7:] + pad[1]],                                          # across a record border: not counted
    ]
    fixed = [
        [b"TTACGTTTTACGTCC"],                                                      # ACGT twice
        [b"A" * 100, b"C" * 3],                                                    # 96 windows of AAAAA
        [b"T" * 100],                                                              # the other strand of the run
        [b"GGGGGGG"],
    ]
    b = _batch(tmp_path, asms)
    try:
        labels = [0, 0, 1]
        present, cop, _, _ = _check(b, [w, rc], asms, 13, labels)
        assert present[0].tolist() == [2, 0] and cop[0].tolist() == [5, 0]
        assert present[13].tolist() == [2, 0] and cop[13].tolist() == [5, 0]      # the reverse complement reads the same figures
        for k in (4, 5, 13):
            queries = [asms[0][0][:80], asms[1][0], b"A" * 20]
            present, cop, _, _ = _check(b, queries, asms, k, labels)
            window = present[:, 0] != NW
            assert np.all(cop[window] >= present[window]) and np.array_equal(cop[window] == 0, present[window] == 0)
    finally:
        b.close()
    b = _batch(tmp_path, fixed, "x")
    try:
        labels = [1, 0, 1, 0]
        present, cop, _, _ = _check(b, [b"ACGT"], fixed, 4, labels)
        assert present[0].tolist() == [0, 1] and cop[0].tolist() == [0, 2]         # a palindrome's window is one window
        present, cop, _, _ = _check(b, [b"AAAAA", b"TTTTTT"], fixed, 5, labels)
        assert present[0].tolist() == [1, 1] and cop[0].tolist() == [96, 96]
        assert present[5].tolist() == [1, 1] and present[6].tolist() == [1, 1] and cop[6].tolist() == [96, 96]
        assert np.all(present[1:5] == NW) and np.all(cop[7:] == NWC)
    finally:
        b.close()


# ---- invariants against existing code on the same batch ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def family(tmp_path_factory):
    """8 assemblies over one ancestor with mutations, a duplicated stretch and a reverse-complemented record; a query cut from it."""
    rng = random.Random(61)
    anc = _rand(rng, 3000)
    asms = []
    for g in range(8):
        seq = bytearray(anc)
        for _ in range(25 * g):
            seq[rng.randrange(len(seq))] = rng.choice(b"ACGT")
        seq = bytes(seq)
        recs = [seq[:1400], _revcomp(seq[1400:2400]) if g % 2 else seq[1400:2400], seq[2400:] + seq[500:620]]
        asms.append(recs)
    queries = [anc[450:700], anc[1380:1420] + b"N" + anc[2000:2100], anc[450:700][::-1], _revcomp(anc[2390:2600])]
    b = _batch(tmp_path_factory.mktemp("kpf"), asms, "f")
    yield b, queries, asms
    b.close()


@pytest.mark.parametrize("k", [21, 8])
def test_invariant_counts(family, k):
    """With every assembly in a group: present summed over the groups and over the first-appearance positions of a query's distinct
    k-mers is the query's row sum of Screen.counts of the same object; counts, n_kmers and containment are those of a plain call."""
    b, queries, asms = family
    labels = [0, 1, 2, 0, 1, 2, 0, 1]
    s, s0 = b.screen(queries, k, profile=labels), b.screen(queries, k)
    try:
        counts, nk = s.counts(), s.n_kmers()
        assert np.array_equal(counts, s0.counts()) and np.array_equal(nk, s0.n_kmers())
        assert np.array_equal(s.containment(), s0.containment(), equal_nan=True) and s.sizes() == s0.sizes()
        assert s.stats()["launches"] == s0.stats()["launches"] and s.stats()["hits"] == s0.stats()["hits"]
        p = s.profile()
        assert p.group_sizes().tolist() == [3, 3, 2] and counts.sum() > 0
        for q, text in enumerate(queries):
            words, ok = H._words(text, k)
            present = p.present(q)
            assert np.array_equal(present[:len(ok), 0] != NW, ok) and np.all(present[len(ok):] == NW)
            _, first = np.unique(words[ok], return_index=True)
            rows = np.flatnonzero(ok)[first]
            assert len(rows) == nk[q]
            assert int(present[rows].astype(np.int64).sum()) == int(counts[q].astype(np.int64).sum())
    finally:
        s.close()
        s0.close()


def test_invariant_oligo_hits(family):
    """kmerlen = 20: present[p, g] is the number of assemblies of g in which the 20-base window at p has an exact site, copies[p, g]
    the sum of their sites (the oligos here are no palindromes: a palindrome's site counts twice there)."""
    b, queries, asms = family
    labels = np.array([0, 1, 255, 0, 1, 1, 0, 1], np.uint8)
    q = queries[0]
    starts = [0, 1, 7, 19, 20, 50, 51, 52, 53, 54, 120, len(q) - 20]
    oligos = [q[p:p + 20] for p in starts]
    assert len(set(oligos)) == 12 and all(o != _revcomp(o) for o in oligos)
    s = b.screen(queries, 20, profile=labels, copies=True)
    oh = b.oligo_hits(oligos, max_mismatch=0)
    try:
        p = s.profile()
        present, cop = p.present(0), p.copies(0)
        sites = oh.n_sites().astype(np.int64)
        assert sites.shape == (12, 8) and sites.max() >= 2          # (the duplicated stretch anc[500:620] holds windows of the query)
        for i, at in enumerate(starts):
            for g in (0, 1):
                assert present[at, g] == int((sites[i, labels == g] > 0).sum())
                assert cop[at, g] == int(sites[i, labels == g].sum())
    finally:
        s.close()
        oh.close()


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------------

def test_degenerate_shapes(tmp_path):
    rng = random.Random(3)
    asms = [[_rand(rng, 300)], [_rand(rng, 150), _rand(rng, 20)]]
    b = _batch(tmp_path, asms)
    try:
        s = b.screen([], 21, profile=[0, 1], copies=True)
        p = s.profile()
        offs, present, cop = p.table()
        assert offs.tolist() == [0] and present.shape == (0, 2) and cop.shape == (0, 2) and p.group_sizes().tolist() == [1, 1]
        assert p.sizes() == (0, 2, True) and p.stats()["copy_adds"] == 0
        s.close()
        q = [asms[0][0][10:60], b"ACGT"]
        present, cop, _, pst = _check(b, q, asms, 21, [255, 255])                 # every assembly left out
        assert present.shape == (54, 1) and not present[:30].any() and not cop[:30].any() and np.all(present[30:] == NW)
        assert pst["copy_adds"] == 0
        _check(b, [b"NNNN", b""], asms, 3, [0, 1])                                 # no window at all
    finally:
        b.close()
    short = [[b"ACGTACGTAC", b"GGGG"], [b"TTTTTTTT"]]                               # every record shorter than k
    b = _batch(tmp_path, short, "s")
    try:
        present, cop, st, _ = _check(b, [b"ACGTACGTACGTACG", b"TTTTTTTTTTTT"], short, 12, [0, 1])
        assert st["batch_kmers"] == 0 and not present[:4].any() and np.all(present[4:15] == NW) and present[15].tolist() == [0, 0]
    finally:
        b.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------

def test_errors(family):
    b, queries, _ = family
    ok = [0] * 8
    for labels, ng in (([0, 1, 2, 3, 0, 0, 0, 0], 3), ([0] * 7 + [254], None), ([0] * 7 + [8], None)):      # a label in n_groups..254
        with pytest.raises(ValueError):
            b.screen(queries, 21, profile=labels, n_groups=ng)
    for ng in (0, 9):
        with pytest.raises(ValueError, match="groups"):
            b.screen(queries, 21, profile=ok, n_groups=ng)
    for labels in ([0] * 7, [0] * 9, [[0] * 8]):
        with pytest.raises(ValueError, match="label"):
            b.screen(queries, 21, profile=labels)
    with pytest.raises(ValueError, match="profile"):
        b.screen(queries, 21, copies=True)
    for k in (0, 33):
        with pytest.raises(ValueError, match="1..32"):
            b.screen(queries, k, profile=ok)
    s = b.screen(queries, 21)
    with pytest.raises(ValueError, match="profile"):
        s.profile()
    s.close()
    s = b.screen(queries, 21, profile=ok)
    with pytest.raises(ValueError, match="copies"):
        s.profile().copies(0)
    assert s.profile().table()[2] is None
    s.close()


# ---- Markers.screen --------------------------------------------------------------------------------------------------------------

def test_markers_screen_profile():
    from seqwin_amd.device import Batch
    sub = {g["name"]: g for g in json.loads((GOLDEN / "subgraphs" / "manifest.json").read_text())["graphs"]}
    c = next(c for c in json.loads((GOLDEN / "markers" / "manifest.json").read_text())["cases"] if c["graph"] == "pan_b_k21_w10" and c["error"] is None)
    g = sub[c["graph"]]
    case = g["cases"][c["case"]]
    b = Batch.from_fasta([GOLDEN / p for p in g["paths"]])
    ix = b.build_index(g["k"], g["w"], g["is_targets"])
    f = ix.filter_graph(g["edge_weight_th"])
    sg = f.subgraphs(case["penalty_th"], case["min_nodes"], case["max_nodes"], random.Random(case["seed"]))
    kept = ix.filter_kmers(f, sg)
    m = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"])
    try:
        offs, blob, _ = m.sequences(b, "reps")
        o = offs.astype(np.int64)
        texts = [blob[o[i]:o[i + 1]] for i in range(len(o) - 1)]
        assert len(texts) > 0
        ro = b.record_offsets()
        asms = [[b.record(r) for r in range(int(ro[a]), int(ro[a + 1]))] for a in range(len(ro) - 1)]
        labels = [0 if t else 1 for t in g["is_targets"]]
        want = H.profile_words(texts, asms, 16, labels)
        s = m.screen(b, 16, profile=labels, copies=True)
        try:
            offs2, present, cop = s.profile().table()
            assert np.array_equal(offs2, want[0]) and np.array_equal(present, want[1]) and np.array_equal(cop, want[2])
            assert np.array_equal(s.profile().group_sizes(), want[3])
            own = m.reps()[0]["assembly_idx"].astype(np.int64)       # a representative is an interval of its own assembly
            for q in range(len(texts)):
                rows = s.profile().present(q)
                rows = rows[rows[:, 0] != NW]
                assert np.all(rows[:, labels[own[q]]] >= 1)
        finally:
            s.close()
        pick = [len(texts) - 1, 0]
        s = m.screen(b, 21, select=pick, profile=labels)
        want = H.profile_words([texts[i] for i in pick], asms, 21, labels)
        assert np.array_equal(s.profile().table()[1], want[1])
        s.close()
    finally:
        for x in (m, kept, sg, f, ix, b):
            x.close()
