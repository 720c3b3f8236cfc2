"""GPU: csrc/align.hip -- Batch.infix_alignments, the canonical alignment behind the infix edit distance -- on crafted pairs against
the host restatement (tests/tools/align_host.py): dist, end, start, nident, mismatch, gaps and the edit scripts, every array whole
and element for element.  The store pass works in blocks of 64 pattern rows and keeps the cells of a band of 2 dist + 1 diagonals;
query lengths, distances, window bounds, the lowered block bound (SEQWIN_AMD_DIST_LDS_CAP), the launch split
(SEQWIN_AMD_SEQ_MAX_BLOCKS) and the lowered scratch budget (SEQWIN_AMD_ALN_SCRATCH_KB) straddle all of it."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import hits_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 130]
DISTS = [1, 31, 32, 33, 64]
OTHER = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d\n" % (name.encode(), i))
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


def _substituted(seq, d):
    """seq with d substitutions at evenly spaced places."""
    out = bytearray(seq)
    for x in range(d):
        at = (2 * x + 1) * len(seq) // (2 * d)
        out[at:at + 1] = OTHER[out[at]]
    return bytes(out)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Records: 0 the ancestor with one N and a run of 12 N; 1 shorter than most queries; 2 the reverse complement of a stretch
    between random text; 3 without an A; 4 a second assembly's record.  Queries: the lengths of LENGTHS cut from the ancestor; a
    stretch of 300 with 1, 31, 32, 33 and 64 substitutions, and with insertions and deletions; 70 A (nothing of record 3 matches:
    dist = m at column 0); one with an invalid byte; one lower case with U; one that lies across the run of N."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    rng = random.Random(43)
    anc = _rand(rng, 2600)
    long_q = anc[700:1000]
    queries = [anc[200:200 + n] for n in LENGTHS]
    queries += [_substituted(long_q, d) for d in DISTS]
    indel = bytearray(long_q)
    for at in (250, 170, 90):
        del indel[at]
    for at in (40, 120, 200):
        indel[at:at] = b"GT"
    queries.append(bytes(indel))
    queries.append(b"A" * 70)
    bad = bytearray(anc[400:500])
    bad[50:51] = b"X"
    queries += [bytes(bad), anc[1300:1400].lower().replace(b"t", b"u"), anc[1450:1560], anc[0:100]]
    Q_LONG, Q_A, Q_ACROSS, Q_HEAD = len(LENGTHS), len(LENGTHS) + len(DISTS) + 1, len(queries) - 2, len(queries) - 1
    rec0 = bytearray(anc)
    rec0[1200:1201] = b"N"
    rec0[1500:1512] = b"N" * 12
    rec2 = _rand(rng, 120) + H.revcomp(anc[650:1050]) + _rand(rng, 90)
    records = [bytes(rec0), anc[300:340], rec2, _rand(rng, 260, b"CGT"), _rand(rng, 300) + anc[650:1700] + _rand(rng, 77)]
    d = tmp_path_factory.mktemp("aln")
    b = Batch.from_fasta([_write(d, "a0.fa", records[:4]), _write(d, "a1.fa", records[4:])], n_cpu=2)
    pairs = []
    for q in range(len(queries)):
        for s in (0, 1):
            pairs += [(q, s, 0, 150, 450), (q, s, 0, 10, 10), (q, s, 1, 0, 40), (q, s, 0, 0, 300), (q, s, 0, 2300, 2600)]
    for q in range(Q_LONG, Q_LONG + len(DISTS) + 1):                       # the edited stretches where they lie, on both strands
        pairs += [(q, 0, 0, 600, 1100), (q, 1, 2, 0, len(rec2)), (q, 0, 4, 200, 800), (q, 0, 0, 700, 1000), (q, 0, 0, 720, 990)]
    q129 = LENGTHS.index(129)
    pairs += [(q129, 0, 0, 100, 329),                                      # j* at n: the copy ends the window
              (q129, 0, 0, 210, 500),                                      # the window starts inside the copy: j == 0 with i > 0
              (q129, 0, 0, 200, 329),                                      # the copy is the window
              (Q_HEAD, 0, 0, 0, 300), (Q_HEAD, 0, 0, 0, 100),              # a copy at column 0 of a window at the record's start
              (Q_A, 0, 3, 0, 260), (Q_A, 1, 3, 0, 260),                    # dist = m, j* = 0 (strand 1: 70 T, which record 3 has)
              (Q_ACROSS, 0, 0, 1400, 1600), (Q_ACROSS, 0, 0, 1450, 1560),  # across the run of N
              (q129, 0, 0, 1100, 1300), (LENGTHS.index(65), 0, 4, 0, 1427)]
    for start in (160, 163, 175, 31, 32, 33):                              # text starts at several places of a packed word
        pairs += [(LENGTHS.index(65), 0, 0, start, start + 400), (q129, 1, 0, start, start + 131)]
    pairs = np.array(pairs, np.int64)
    want = A.alignments(queries, records, pairs)
    yield b, queries, records, pairs, want
    b.close()


def _check(case, order=None):
    b, queries, _, pairs, want = case
    idx = np.arange(len(pairs)) if order is None else np.asarray(order)
    got = b.infix_alignments(queries, pairs[idx], ops=True, stats=True)
    st = got[-1]
    w_off = want["offsets"].astype(np.int64)
    for name, arr in zip(A.FIELDS, got[:6]):
        assert arr.dtype == np.uint32 and arr.shape == (len(idx),), name
        bad = np.flatnonzero(arr != want[name][idx])
        assert not len(bad), (name, pairs[idx][bad[:5]].tolist(), arr[bad[:5]], want[name][idx][bad[:5]])
    offsets, ops = got[6], got[7]
    assert offsets.dtype == np.uint64 and ops.dtype == np.uint8
    lens = (w_off[1:] - w_off[:-1])[idx]
    assert np.array_equal(offsets.astype(np.int64), np.concatenate(([0], np.cumsum(lens))))
    want_ops = np.concatenate([want["ops"][w_off[i]:w_off[i + 1]] for i in idx]) if len(idx) else np.zeros(0, np.uint8)
    assert np.array_equal(ops, want_ops)
    assert st["pairs"] == len(idx) and st["ops"] == len(ops)
    return st


def test_the_crafted_pairs_cover_their_bounds(case):
    """On the host: the distances, band widths and walk ends this file is about occur among the pairs."""
    _, queries, _, pairs, want = case
    m = np.array([len(queries[q]) for q in pairs[:, 0]])
    dist, js, j0 = want["dist"], want["end"] - pairs[:, 3], want["start"] - pairs[:, 3]
    assert set(LENGTHS) <= set(m.tolist())
    assert {0, 1, 31, 32, 33, 64} <= set(dist.tolist()) and ((dist == m) & (m >= 70)).any()
    assert ((js == 0) & (m > 0)).any() and ((js == pairs[:, 4] - pairs[:, 3]) & (m > 64)).any()
    assert ((j0 == 0) & (js > 0) & (m > 64)).any()                          # the band is clipped at column 0
    o = want["offsets"].astype(np.int64)
    lead_i = [want["ops"][o[x]] == 2 for x in range(len(pairs)) if o[x + 1] > o[x] and js[x] > 0]
    assert any(lead_i)                                                      # the walk reaches j == 0 with i > 0
    assert (want["gaps"] > 0).sum() > 10 and (want["mismatch"] > 0).sum() > 10
    pick = np.flatnonzero(m <= 130)[::9]
    lit = A.alignments_literal(queries, case[2], pairs[pick])
    for f in A.FIELDS:
        assert np.array_equal(lit[f], want[f][pick]), f


def test_crafted_pairs(case):
    st = _check(case)
    assert st["striped_pairs"] == 0 and st["rounds"] == 1 and st["own_scratch_pairs"] == 0
    assert st["scratch_peak_bytes"] >= st["largest_pair_bytes"] > 0


def test_without_scripts(case):
    b, queries, _, pairs, want = case
    got = b.infix_alignments(queries, pairs)
    assert len(got) == 6
    for name, arr in zip(A.FIELDS, got):
        assert np.array_equal(arr, want[name]), name
    d, e = b.infix_distances(queries, pairs)
    assert np.array_equal(d, got[0]) and np.array_equal(e, got[1])


@pytest.mark.parametrize("cap", [1, 2])
def test_the_striped_route(case, monkeypatch, cap):
    monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", str(cap))
    st = _check(case)
    assert st["striped_pairs"] > 0


def test_several_launches(case, monkeypatch):
    one = _check(case)
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    st = _check(case)
    assert st["store_launches"] > one["store_launches"]
    monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", "2")
    _check(case)


@pytest.mark.parametrize("kb", [16, 1])
def test_several_rounds_and_a_pair_above_the_budget(case, monkeypatch, kb):
    one = _check(case)
    monkeypatch.setenv("SEQWIN_AMD_ALN_SCRATCH_KB", str(kb))
    st = _check(case)
    assert st["rounds"] > 2 and st["own_scratch_pairs"] >= 1 and st["largest_pair_bytes"] == one["largest_pair_bytes"] > kb * 1024
    if kb == 16:
        assert st["rounds"] < st["pairs"] // 2 and st["scratch_peak_bytes"] == st["largest_pair_bytes"]
    monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", "1")
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    _check(case)


def test_shuffled_order(case, monkeypatch):
    order = list(range(len(case[3])))
    random.Random(5).shuffle(order)
    _check(case, order)
    monkeypatch.setenv("SEQWIN_AMD_ALN_SCRATCH_KB", "16")
    _check(case, order[::-1])


def test_malformed_pairs_raise(case):
    b, queries, records, _, _ = case
    for p in ((len(queries), 0, 0, 0, 10), (0, 2, 0, 0, 10), (0, 0, len(records), 0, 10), (0, 0, 0, 11, 10), (0, 0, 1, 0, 41)):
        with pytest.raises(ValueError):
            b.infix_alignments(queries, [p])
    got = b.infix_alignments(queries, np.zeros((0, 5), np.int64), ops=True)
    assert all(a.shape == (0,) for a in got[:6]) and got[6].tolist() == [0] and got[7].shape == (0,)
