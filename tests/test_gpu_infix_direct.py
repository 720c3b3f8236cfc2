"""GPU: Layer A of csrc/hits.hip -- Batch.infix_distances, the infix edit distance of a query to an interval of the batch -- on
crafted pairs against the host restatement (tests/tools/hits_host.py): every dist and every end, exactly and whole.  The kernel
works in blocks of 64 pattern rows, reads the text 32 columns at a time from 16-base words, and takes queries above the block bound
through the striped route; query lengths, text starts and the lowered bound (SEQWIN_AMD_DIST_LDS_CAP) straddle all of them."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import hits_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129]


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _write(d, name, records):
    p = d / name
    with open(p, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">%s_r%d\n" % (name.encode(), i))
            f.write(b"\n".join(r[j:j + 70] for j in range(0, len(r), 70)) + b"\n")
    return p


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """Records: 0 the ancestor with one N; 1 shorter than most queries; 2 planted copies of the 129-base query (exact, one
    substitution, one insertion, one deletion, and a reverse complement); 3 two equally good copies of the 65-base query; 4 a second
    assembly's record.  Queries: the lengths of LENGTHS cut from the ancestor, two long ones (5 and 11 blocks), one with an invalid
    byte, one lower case with U."""
    from seqwin_amd.device import Batch, set_device
    set_device(0)
    rng = random.Random(41)
    anc = _rand(rng, 2600)
    queries = [anc[200:200 + n] for n in LENGTHS] + [anc[700:1000], anc[900:1600]]
    bad = bytearray(anc[400:500])
    bad[50:51] = b"X"
    queries += [bytes(bad), anc[1300:1400].lower().replace(b"t", b"u")]
    q129, q65 = queries[7], queries[4]
    sub = bytearray(q129)
    sub[60] = ord("ACGT"["ACGT".index(chr(sub[60])) ^ 1])
    ins, dele = q129[:70] + b"G" + q129[70:], q129[:90] + q129[91:]
    rec0 = anc[:1200] + b"N" + anc[1201:]
    rec2 = (_rand(rng, 100) + q129 + _rand(rng, 50) + bytes(sub) + _rand(rng, 50) + ins + _rand(rng, 50) + dele + _rand(rng, 50)
            + H.revcomp(q129) + _rand(rng, 100))
    rec3 = _rand(rng, 70) + q65 + _rand(rng, 30) + q65 + _rand(rng, 40)
    records = [rec0, anc[300:340], rec2, rec3, _rand(rng, 500) + anc[650:1700] + _rand(rng, 77)]
    d = tmp_path_factory.mktemp("infix")
    b = Batch.from_fasta([_write(d, "a0.fa", records[:4]), _write(d, "a1.fa", records[4:])], n_cpu=2)
    pairs = []
    for q in range(len(queries)):
        for s in (0, 1):
            pairs += [(q, s, 0, 150, 450), (q, s, 0, 1100, 1700), (q, s, 0, 10, 10), (q, s, 1, 0, 40),     # an N inside; empty; short
                      (q, s, 0, 0, 300), (q, s, 0, 2300, 2600), (q, s, 4, 400, 1627)]                      # clipped at either record end
    for start in list(range(160, 176)) + [31, 32, 33]:                                                      # every residue mod 16; the 32-column reads
        pairs += [(4, 0, 0, start, start + 400), (7, 1, 0, start, start + 131), (9, 0, 4, start, start + 1300)]
    o2 = [100, 100 + 129 + 50, 100 + 2 * 129 + 100, 100 + 3 * 129 + 151, 100 + 4 * 129 + 200]               # where rec2's copies start
    planted = len(pairs)
    pairs += [(7, 0, 2, 0, o2[1] - 10), (7, 0, 2, o2[1] - 20, o2[2] - 10), (7, 0, 2, o2[2] - 20, o2[3] - 10), (7, 0, 2, o2[3] - 20, o2[4] - 10),
              (7, 1, 2, o2[4] - 30, len(rec2)), (4, 0, 3, 0, len(rec3)), (7, 0, 2, 0, len(rec2))]
    pairs = np.array(pairs, np.int64)
    want = H.infix(queries, records, pairs)
    yield b, queries, records, pairs, want, planted, o2
    b.close()


def _check(case, **kw):
    b, queries, _, pairs, want, _, _ = case
    dist, end, st = b.infix_distances(queries, pairs, stats=True)
    assert dist.dtype == np.uint32 and end.dtype == np.uint32 and dist.shape == end.shape == (len(pairs),)
    bad = np.flatnonzero((dist != want[0]) | (end != want[1]))
    assert not len(bad), (pairs[bad[:5]].tolist(), dist[bad[:5]], want[0][bad[:5]], end[bad[:5]], want[1][bad[:5]])
    assert st["pairs"] == len(pairs)
    return st


def test_the_restatements_agree_on_the_crafted_pairs(case):
    _, queries, records, pairs, want, _, _ = case
    pick = pairs[::7]
    lit = H.infix_literal(queries, records, pick)
    assert np.array_equal(lit[0], want[0][::7]) and np.array_equal(lit[1], want[1][::7])


def test_crafted_pairs(case):
    st = _check(case)
    assert st["striped_pairs"] == 0 and st["block_cap"] == 64 and st["longest"] == 700


def test_planted_copies(case):
    b, queries, _, pairs, _, planted, o2 = case
    dist, end = b.infix_distances(queries, pairs[planted:])
    assert dist.tolist() == [0, 1, 1, 1, 0, 0, 0]
    assert end[0] == o2[0] + 129 and end[1] == o2[1] + 129 and end[2] == o2[2] + 130 and end[3] == o2[3] + 128 and end[4] == o2[4] + 129
    assert end[5] == 70 + 65                  # two equally good copies: the smallest end
    assert end[6] == o2[0] + 129              # the exact copy beats the edited ones
    pq = len(queries) * 2 * 7                 # empty queries and empty texts among the first pairs
    d0, e0 = b.infix_distances(queries, pairs[:pq])
    for (q, s, r, a, z), d, e in zip(pairs[:pq].tolist(), d0.tolist(), e0.tolist()):
        if len(queries[q]) == 0:
            assert (d, e) == (0, a)
        elif a == z:
            assert (d, e) == (len(queries[q]), a)


@pytest.mark.parametrize("cap", [1, 2])
def test_the_striped_route(case, monkeypatch, cap):
    monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", str(cap))
    st = _check(case)
    assert st["block_cap"] == cap and st["striped_pairs"] > 0


def test_several_launches(case, monkeypatch):
    one = _check(case)
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    st = _check(case)
    assert st["launches"] > one["launches"]
    monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", "2")
    _check(case)


def test_malformed_pairs_raise(case):
    b, queries, records, _, _, _, _ = case
    for p in ((len(queries), 0, 0, 0, 10), (0, 2, 0, 0, 10), (0, 0, len(records), 0, 10), (0, 0, 0, 11, 10), (0, 0, 1, 0, 41)):
        with pytest.raises(ValueError):
            b.infix_distances(queries, [p])
    d, e = b.infix_distances(queries, np.zeros((0, 5), np.int64))
    assert d.shape == e.shape == (0,)
