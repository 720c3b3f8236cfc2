"""GPU: csrc/local.hip -- Batch.local_alignments, the optimal local alignment with affine gap scores -- on crafted pairs against the
host restatement (tests/tools/local_host.py): all nine arrays whole and element for element, and the identities of DESIGN.md section
3.2i on every output.  A lane owns R pattern rows, a group of at most 64 lanes makes one pass, longer queries take several passes
with a carry row in LDS or HBM; query lengths, text lengths, gaps and maxima straddle all of it, natively and with the pass
(SEQWIN_AMD_LOCAL_ROWS), the LDS bound (SEQWIN_AMD_LOCAL_LDS_KB) and the launch split (SEQWIN_AMD_SEQ_MAX_BLOCKS) lowered."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import hits_host as H  # noqa: E402
import local_host as L  # noqa: E402

pytestmark = pytest.mark.gpu
BLASTN = (2, -3, 5, 2)
TEXTS = [0, 1, 63, 64, 65]


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _other(rng, base):
    return bytes([rng.choice([c for c in b"ACGT" if c != base])])


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d\n" % (name.encode(), i))
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def make_case(R):
    """Records: 0 the ancestor with one N and a run of 12 N; 1 a piece of 65 bases; 2 the reverse complement of a stretch between
    random text; 3 two letters only (ties); 4 a second assembly's record.  Queries: the lengths 1, 2, R-1, R, R+1, 64R-1, 64R, 64R+1
    and 2*64R+1 cut from the ancestor; a stretch with runs of 3 or 4 inserted bases across rows 2R, 8R and 64R (a gap that opens in one
    lane's strip, or in one pass, and extends into the next) and two deletions; copies that end in row 2R and in row 64R before
    unrelated text (the maximum in the last row of a pass); an invalid byte; lower case with U; two letters; an empty query."""
    rng = random.Random(71)
    anc = _rand(rng, 1400)
    rec0 = bytearray(anc)
    rec0[900:901] = b"N"
    rec0[1000:1012] = b"N" * 12
    rec2 = _rand(rng, 90) + H.revcomp(anc[40:700]) + _rand(rng, 60)
    records = [bytes(rec0), anc[100:165], rec2, _rand(rng, 300, b"AC"), _rand(rng, 50) + anc[20:420] + _rand(rng, 33)]
    lens = [1, 2, R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 2 * 64 * R + 1]
    queries = [anc[40:40 + n] for n in lens]
    gap = bytearray(anc[40:40 + 64 * R + 90])
    for at, n in ((64 * R - 2, 4), (8 * R - 2, 4), (3 * R + 5, 0), (2 * R - 2, 3)):   # (from the back: earlier places stay put)
        if n:
            gap[at:at] = _rand(rng, n)
        else:
            del gap[at:at + 2]
    Q_GAP = len(queries)
    queries.append(bytes(gap))
    Q_END2R, Q_END64R = len(queries), len(queries) + 1
    queries.append(anc[40:40 + 2 * R] + _other(rng, anc[40 + 2 * R]) + _rand(rng, 12, b"N"))
    queries.append(anc[40:40 + 64 * R] + _other(rng, anc[40 + 64 * R]) + _rand(rng, 12, b"N"))
    bad = bytearray(anc[700:800])
    bad[50:51] = b"X"
    Q_SMALL = len(queries)
    queries += [bytes(bad), anc[800:900].lower().replace(b"t", b"u"), anc[960:1050], _rand(rng, 40, b"AC"), b"", anc[100:165]]
    Q_TIE, Q_65 = len(queries) - 3, len(queries) - 1
    pairs = []
    for q in range(len(queries)):
        pairs += [(q, 0, 0, 0, 330), (q, 1, 2, 60, 400)]
    for q in (Q_GAP, Q_END2R, Q_END64R):
        pairs += [(q, 0, 0, 20, 700), (q, 0, 4, 0, len(records[4])), (q, 1, 0, 0, 200)]
    for q in range(Q_SMALL, len(queries)):
        pairs += [(q, s, r, 0, len(records[r])) for s in (0, 1) for r in (1, 3)] + [(q, 0, 0, 850, 1100), (q, 1, 0, 700, 900)]
    for t in TEXTS:                                                       # texts of 0, 1, 63, 64 and 65 bases
        pairs += [(Q_65, 0, 0, 100, 100 + t), (Q_65, 1, 2, 600 - t, 600), (lens.index(R + 1), 0, 0, 40, 40 + t), (Q_TIE, 0, 3, 7, 7 + t)]
    for start in (31, 32, 33, 47):                                        # text starts at several places of a packed word
        pairs += [(Q_65, 0, 0, start, start + 200), (lens.index(64 * R - 1), 0, 0, start, start + 140)]
    pairs = np.array(pairs, np.int64)
    small = np.flatnonzero(np.array([len(queries[q]) for q in pairs[:, 0]]) <= 130)
    want = L.alignments(queries, records, pairs)
    info = dict(R=R, lens=lens, Q_GAP=Q_GAP, Q_END2R=Q_END2R, Q_END64R=Q_END64R, Q_TIE=Q_TIE, small=small)
    return queries, records, pairs, want, info


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The batch of make_case's records in two assemblies; R, the rows of a lane, is read from the counters of an empty call."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    probe = Batch.synthetic(1, 1, 64)
    try:
        R = probe.local_alignments([b"A"], np.zeros((0, 5), np.int64), stats=True)["stats"]["pass_rows"] // 64
    finally:
        probe.close()
    assert R >= 2
    queries, records, pairs, want, info = make_case(R)
    d = tmp_path_factory.mktemp("local")
    b = Batch.from_fasta([_write(d, "a0.fa", records[:3]), _write(d, "a1.fa", records[3:])], n_cpu=2)
    yield b, queries, records, pairs, want, info
    b.close()


def _check(case, order=None, scoring=BLASTN, want=None, subset=None):
    b, queries, records, pairs, base_want, _ = case
    want = base_want if want is None else want
    idx = np.arange(len(pairs)) if subset is None else np.asarray(subset)
    if order is not None:
        idx = idx[np.asarray(order)]
    got = b.local_alignments(queries, pairs[idx], scoring, stats=True)
    st = got.pop("stats")
    assert tuple(got) == L.FIELDS
    for name in L.FIELDS:
        arr = got[name]
        assert arr.dtype == np.uint32 and arr.shape == (len(idx),), name
        bad = np.flatnonzero(arr != want[name][idx])
        assert not len(bad), (name, pairs[idx][bad[:5]].tolist(), arr[bad[:5]], want[name][idx][bad[:5]])
    L.check(got, scoring, queries, records, pairs[idx])
    assert st["pairs"] == len(idx)
    assert st["cells"] == sum(len(queries[q]) * (e - s) for q, _, _, s, e in pairs[idx].tolist())
    return st


def test_the_crafted_pairs_cover_their_bounds(case):
    """On the host: what this file is about occurs among the pairs, and the second restatement agrees on the short ones."""
    _, queries, records, pairs, want, info = case
    R = info["R"]
    m = np.array([len(queries[q]) for q in pairs[:, 0]])
    assert set(info["lens"]) <= set(m.tolist()) and set(TEXTS) <= set((pairs[:, 4] - pairs[:, 3]).tolist())
    L.check(want, BLASTN, queries, records, pairs)
    g = np.flatnonzero((pairs[:, 0] == info["Q_GAP"]) & (pairs[:, 2] == 0) & (pairs[:, 3] == 20))[0]
    assert want["gapopen"][g] == 4 and want["gaps"][g] == 3 + 2 + 4 + 4 and want["qstart"][g] == 0 and want["qend"][g] == len(queries[info["Q_GAP"]])
    for q, row in ((info["Q_END2R"], 2 * R), (info["Q_END64R"], 64 * R)):
        x = np.flatnonzero((pairs[:, 0] == q) & (pairs[:, 2] == 0) & (pairs[:, 3] == 20))[0]
        assert want["qend"][x] == row and want["score"][x] == 2 * row           # the maximum lies in the last row of a pass
    assert (want["score"] == 0).sum() >= 8 and (want["mismatch"] > 0).any() and ((want["score"] > 0) & (pairs[:, 1] == 1)).sum() > 10
    pick = info["small"][::3]
    lit = L.alignments_literal(queries, records, pairs[pick])
    for f in L.FIELDS:
        assert np.array_equal(lit[f], want[f][pick]), f


def test_crafted_pairs(case):
    st = _check(case)
    R = case[5]["R"]
    assert st["pass_rows"] == 64 * R and st["hbm_carry_pairs"] == 0
    m = np.array([len(case[1][q]) for q in case[3][:, 0]])
    n = case[3][:, 4] - case[3][:, 3]
    assert st["striped_pairs"] == int(((m > 64 * R) & (n > 0)).sum()) > 0


@pytest.mark.parametrize("rows", [1, 2, 8])
def test_lowered_passes(case, monkeypatch, rows):
    """A pass of R, 2R and 8R rows: short queries take several passes, gaps and maxima meet the pass bounds."""
    R = case[5]["R"]
    monkeypatch.setenv("SEQWIN_AMD_LOCAL_ROWS", str(rows * R))
    st = _check(case)
    assert st["pass_rows"] == rows * R and st["hbm_carry_pairs"] == 0
    m = np.array([len(case[1][q]) for q in case[3][:, 0]])
    n = case[3][:, 4] - case[3][:, 3]
    assert st["striped_pairs"] == int(((m > rows * R) & (n > 0)).sum())


@pytest.mark.parametrize("rows", [None, 2])
def test_the_carry_row_in_hbm(case, monkeypatch, rows):
    R = case[5]["R"]
    monkeypatch.setenv("SEQWIN_AMD_LOCAL_LDS_KB", "2")                     # 64 columns: texts of 65 bases and more carry through HBM
    if rows:
        monkeypatch.setenv("SEQWIN_AMD_LOCAL_ROWS", str(rows * R))
    st = _check(case)
    m = np.array([len(case[1][q]) for q in case[3][:, 0]])
    n = case[3][:, 4] - case[3][:, 3]
    assert st["hbm_carry_pairs"] == int(((m > st["pass_rows"]) & (n > 64)).sum()) > 0
    assert st["striped_pairs"] >= st["hbm_carry_pairs"]
    if rows:
        assert st["striped_pairs"] > st["hbm_carry_pairs"]                 # (texts of 1, 63 and 64 bases stay in LDS)


def test_several_launches(case, monkeypatch):
    one = _check(case)
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    st = _check(case)
    assert st["launches"] > one["launches"]
    monkeypatch.setenv("SEQWIN_AMD_LOCAL_ROWS", str(2 * case[5]["R"]))
    monkeypatch.setenv("SEQWIN_AMD_LOCAL_LDS_KB", "2")
    _check(case)


def test_shuffled_order(case, monkeypatch):
    order = list(range(len(case[3])))
    random.Random(5).shuffle(order)
    _check(case, order)
    monkeypatch.setenv("SEQWIN_AMD_LOCAL_ROWS", str(case[5]["R"]))
    _check(case, order[::-1])


@pytest.mark.parametrize("scoring", L.SCORINGS[1:])
def test_the_other_scoring_systems(case, monkeypatch, scoring):
    """On the pairs with short queries (the two-letter ones make the ties), natively and with a pass of two lanes."""
    _, queries, records, pairs, _, info = case
    sub = info["small"]
    w = L.alignments(queries, records, pairs[sub], scoring)
    want = {f: np.zeros(len(pairs), np.uint32) for f in L.FIELDS}
    for f in L.FIELDS:
        want[f][sub] = w[f]
    _check(case, scoring=scoring, want=want, subset=sub)
    monkeypatch.setenv("SEQWIN_AMD_LOCAL_ROWS", str(2 * info["R"]))
    _check(case, scoring=scoring, want=want, subset=sub)


def test_outputs_may_be_absent(case):
    """The C ABI takes NULL for any of the nine arrays."""
    import ctypes

    from seqwin_amd._lib import check, lib
    from seqwin_amd.device import _infix_pairs, _ptr, _query_csr, _scoring
    b, queries, _, pairs, want, _ = case
    offs, blob, nq = _query_csr(queries)
    pr = _infix_pairs(pairs)
    score, gaps = np.empty(len(pr), np.uint32), np.empty(len(pr), np.uint32)
    check(lib.sw_batch_local_alignments(b._h, _ptr(offs), blob, ctypes.c_uint64(nq), _ptr(pr), ctypes.c_uint64(len(pr)), _scoring(BLASTN), _ptr(score), None,
                                        None, None, None, None, None, None, _ptr(gaps), None, None))
    assert np.array_equal(score, want["score"]) and np.array_equal(gaps, want["gaps"])


def test_malformed_calls_raise(case):
    b, queries, records, _, _, _ = case
    for p in ((len(queries), 0, 0, 0, 10), (0, 2, 0, 0, 10), (0, 0, len(records), 0, 10), (0, 0, 0, 11, 10), (0, 0, 1, 0, 66)):
        with pytest.raises(ValueError):
            b.local_alignments(queries, [p])
    for bad in ((0, -3, 5, 2), (256, -3, 5, 2), (2, 0, 5, 2), (2, -256, 5, 2), (2, -3, -1, 2), (2, -3, 256, 2), (2, -3, 5, 0), (2, -3, 5, 256), (2, -3, 5)):
        with pytest.raises(ValueError):
            b.local_alignments(queries, [(0, 0, 0, 0, 10)], bad)
    with pytest.raises(ValueError):
        b.local_alignments([b"A" * (1 << 16)], [(0, 0, 0, 0, 10)])
    assert b.local_alignments([b"A" * ((1 << 16) - 1)], [(0, 0, 0, 5, 5)])["score"].tolist() == [0]
    got = b.local_alignments(queries, np.zeros((0, 5), np.int64))
    assert all(got[f].shape == (0,) for f in L.FIELDS)
    assert b.local_alignments(queries, [(0, 0, 0, 40, 41)], (255, -255, 255, 255))["score"].tolist() == [255]


def test_the_tie_cases_with_their_figures_written_out(tmp_path, monkeypatch):
    """The hand-derived cases of tests/test_local_cpu.py under (1, -2, 0, 1): the diagonal wins a tie against E and F, E wins a tie
    against F, extension wins a tie against opening -- natively and with a pass of one lane, where rows 8 | 9 meet at a carry row."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    queries = [b"ACATTT", b"GCACTTT", b"ACGTGACGT", b"ACGTACGTGGCCAATT", b"ACGTACGTTTGGCCAATT"]
    records = [b"GCACTTT", b"ACATTT", b"ACGTCACGT", b"ACGTCCACGT", b"ACGTACGTTTGGCCAATT", b"ACGTACGTGGCCAATT"]
    pairs = [(0, 0, 0, 0, 7), (1, 0, 1, 0, 6), (2, 0, 2, 0, 9), (2, 0, 3, 0, 10), (3, 0, 4, 0, 18), (4, 0, 5, 0, 16)]
    figures = [(4, 1, 6, 1, 7, 5, 0, 1, 1), (4, 2, 7, 0, 6, 5, 0, 1, 1), (6, 0, 9, 0, 9, 8, 1, 0, 0), (5, 0, 9, 0, 10, 8, 1, 1, 1),
               (14, 0, 16, 0, 18, 16, 0, 1, 2), (14, 0, 18, 0, 16, 16, 0, 1, 2)]
    b = Batch.from_fasta([_write(tmp_path, "ties.fa", records)], n_cpu=1)
    try:
        for rows in (None, 8, 16):
            if rows:
                monkeypatch.setenv("SEQWIN_AMD_LOCAL_ROWS", str(rows))
            got = b.local_alignments(queries, pairs, (1, -2, 0, 1))
            assert [tuple(int(got[f][x]) for f in L.FIELDS) for x in range(len(pairs))] == figures, rows
    finally:
        b.close()
