"""The core of csrc/seqs.hip on crafted intervals of a small batch (Batch.fetch, Batch.edit_distances) against the host
restatement (tests/tools/seqs_host.py): every alignment of an interval inside the 2-bit words, the ends of records and of the
batch, the run boundaries of a record with lower case, N runs and IUPAC letters, a .gz input, the launch split of the decode, and
for the distances the block bounds of the bit-vector recurrence on both routes (SEQWIN_AMD_DIST_LDS_CAP), with R and S in the same
record and in different ones, invalid bases on either side."""
import gzip
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import seqs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
RNG = random.Random(20)
MESSY = ("acgtACGTacgtACGGTCATTGACCATGatcgatcgaTCGATTAGCAGGCATCGA" + "NNNNN" + "GATTACAGATTACACCGGTTAACCGGTTAGCATCGACTAGCA" + "R" +
         "ccggatatatcgcgatatcgcgatatagcg" + "nn" + "ACGATCGATCGACTAGCTAGC" + "Y" + "A")


POOL, LONG, MESSY_REC, MESSY2, SINGLE, TAIL = range(6)   # the batch's records: a.fa | b.fa.gz (three records) | c.fa (two)


def _rnd(n):
    return "".join(RNG.choice("ACGT") for _ in range(n))


def _mutate(s, rate):
    if rate == 0:
        return s
    out = list(s)
    n_edits = 1 if rate == 1 else max(1, len(s) // 10)
    for _ in range(n_edits):
        at = RNG.randrange(len(out) + 1)
        kind = RNG.randrange(3)
        if kind == 0 and at < len(out):
            out[at] = RNG.choice([c for c in "ACGT" if c != out[at]])
        elif kind == 1 and len(out) > 1:
            del out[min(at, len(out) - 1)]
        else:
            out.insert(at, RNG.choice("ACGT"))
    return "".join(out)


class Pool:
    """Strings laid into one record behind fillers of 0-17 bases, so that their starts meet every place of a 2-bit word."""

    def __init__(self, record):
        self.record, self.text = record, []
        self.n = 0

    def add(self, s):
        fill = _rnd(RNG.randrange(18))
        self.text.append(fill + s)
        start = self.n + len(fill)
        self.n = start + len(s)
        return (self.record, start, self.n)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """Files, the batch made of them, the records' texts by global record, and the crafted distance pairs with their expected
    answers (computed once on the host)."""
    from seqwin_amd.device import Batch
    d = tmp_path_factory.mktemp("seqs")
    r1 = list(_rnd(9000))                 # record LONG: one valid run
    messy2 = r1[2000:2300]                # record MESSY2: a copy of LONG[2000:2300) with invalid bases, among them base 50 and block ends
    for at, ch in ((10, "N"), (50, "N"), (63, "R"), (64, "n"), (130, "N"), (131, "N"), (132, "N"), (133, "Y"), (255, "K"), (299, "N")):
        messy2[at] = ch
        r1[2000 + at] = "A"               # the packed code of an invalid base is A's: taken for valid it would match here
    r1, messy2 = "".join(r1), "".join(messy2)
    pool = Pool(POOL)
    pairs, sizes = [], (1, 63, 64, 65, 127, 128, 129)
    for np_ in sizes:
        for nt in sizes:
            for rate in (0, 1, 10):
                p = _rnd(np_)
                t = _mutate(p, rate) if np_ == nt else _mutate((p * (nt // np_ + 1))[:nt] if np_ < nt else p[:nt], rate)
                a, b = pool.add(p), pool.add(t)
                pairs += [(a, b), (a, pool.add(H.revcomp(t).decode()))]
    text = _rnd(4100)
    for blocks in (63, 64, 65):   # the lane bound of a one-wave wavefront
        p = _mutate((text + _rnd(100))[:blocks * 64], 10)
        p = (p + _rnd(64))[:blocks * 64]
        a, b = pool.add(p), pool.add(text)
        pairs += [(a, b), (b, a), (a, pool.add(H.revcomp(text).decode()))]
    one, long_ = pool.add("G"), pool.add(_rnd(4096))
    pairs += [(one, long_), (long_, one)]
    pal = pool.add("ACGCGT")
    pairs.append((pal, pal))                                                   # a reverse palindrome -> (0, 0)
    pairs.append((pool.add("AC"), pool.add("CA")))                              # d_fwd == d_rev == 2 -> strand 0
    m1, m2 = pool.add(MESSY), pool.add(_mutate(MESSY.upper().replace("N", "A").replace("R", "G").replace("Y", "C"), 10))
    m3 = pool.add(MESSY[5:] + "ACGT")
    pairs += [(m1, m2), (m2, m1), (m1, m3), (m1, m1), (m1, pool.add(H.revcomp(MESSY.upper()).decode()))]   # invalid bases in R, S, both
    big = pool.add(_rnd(700))
    pairs += [((0, big[1] + s0, big[1] + s0 + 150), (0, big[1] + 300 + s1, big[1] + 300 + s1 + 140)) for s0 in (1, 15, 16) for s1 in (3, 13)]
    pairs += [((0, 7, 7), long_), (one, (0, 9, 9)), ((0, 3, 3), (0, 5, 5))]    # an empty side
    # R and S in DIFFERENT records: what row_distances always does.  Clean grid pairs first ...
    for n, off in ((1, 77), (63, 501), (64, 1000), (65, 1601), (129, 3015), (300, 4000)):
        t = pool.add(_mutate(r1[off:off + n], 10))
        pairs += [((LONG, off, off + n), t), (t, (LONG, off, off + n))]
    # ... then invalid bases on one side at positions that the OTHER record's single long valid run covers (a run remembered from
    # one record must not answer for the other), on either side, on both, as pattern and as text, and on the reverse strand
    whole2, whole_m = (MESSY2, 0, 300), (MESSY_REC, 0, len(MESSY))
    cross = [((LONG, 2000, 2300), whole2), ((LONG, 2000, 2100), (MESSY2, 0, 100)), ((LONG, 2000, 2050), whole2), ((LONG, 2040, 2060), (MESSY2, 40, 60)),
             ((LONG, 0, len(MESSY)), whole_m), ((LONG, 100, 400), whole_m), (m1, whole_m), (whole2, whole_m), ((MESSY2, 120, 140), (MESSY_REC, 50, 64)),
             ((LONG, 2000, 2300), pool.add(H.revcomp(messy2.upper()).decode())), (pool.add(H.revcomp(r1[2000:2300]).decode()), whole2)]
    pairs += cross + [(b, a) for a, b in cross]
    recs0 = "".join(pool.text)
    f0 = d / "a.fa"
    f0.write_text(">pool\n" + "\n".join(recs0[i:i + 70] for i in range(0, len(recs0), 70)) + "\n")
    f1 = d / "b.fa.gz"
    f1.write_bytes(gzip.compress((">long x\n" + "\n".join(r1[i:i + 60] for i in range(0, len(r1), 60)) + "\n>messy\n" + MESSY + "\n>messy2\n" +
                                  messy2 + "\n").encode()))
    f2 = d / "c.fa"
    f2.write_text(">single\nG\n>tail\n" + _rnd(40) + "\n")
    files = [f0, f1, f2]
    batch = Batch.from_fasta(files, n_cpu=2)
    texts = [t for f in files for t in H.read_records(f)]
    assert batch.info()["n_records"] == len(texts) == 6 and [len(t) for t in texts] == [len(recs0), 9000, len(MESSY), 300, 1, 40]
    want = [H.distance(H.fetch(texts[a[0]], a[1], a[2])[0], H.fetch(texts[b[0]], b[1], b[2])[0]) for a, b in pairs]
    return dict(batch=batch, texts=texts, pairs=pairs, want=want)


def _check_fetch(world, ivs, **kw):
    offs, blob, inexact = world["batch"].fetch(np.array(ivs, np.int64).reshape(-1, 3), **kw)[:3]
    assert len(offs) == len(ivs) + 1 and offs[0] == 0 and int(offs[-1]) == len(blob)
    for i, (r, a, b) in enumerate(ivs):
        want, bad = H.fetch(world["texts"][r], a, b)
        assert blob[int(offs[i]):int(offs[i + 1])].decode() == want, (r, a, b)
        assert bool(inexact[i]) == bad, (r, a, b)


def test_fetch_at_every_alignment_and_length(world):
    ivs = []
    for rec in (0, 1):                       # a plain file and the .gz input
        for base in (0, 16, 4000):
            for sm in (0, 1, 15):
                for ln in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4097):
                    ivs.append((rec, base + sm, base + sm + ln))
    n1 = len(world["texts"][1])
    ivs += [(1, 0, n1), (1, n1 - 33, n1), (1, n1, n1), (1, 0, 0)]            # from base 0, up to rec_len, empty at either end
    ivs += [(SINGLE, 0, 1), (SINGLE, 0, 0), (SINGLE, 1, 1), (TAIL, 0, 40), (TAIL, 39, 40), (TAIL, 17, 40)]   # the one-base record; the last record of the last assembly
    ivs += [(MESSY2, 0, 300), (MESSY2, 40, 60), (MESSY2, 51, 63), (MESSY2, 65, 130)]
    _check_fetch(world, ivs)


def test_fetch_at_the_run_boundaries(world):
    messy = world["texts"][2]
    bad = [i for i, ch in enumerate(messy) if ch not in "ACGT"]
    gaps = []                                 # maximal stretches of invalid bases
    for i in bad:
        if gaps and gaps[-1][1] == i:
            gaps[-1][1] = i + 1
        else:
            gaps.append([i, i + 1])
    assert [b - a for a, b in gaps] == [5, 1, 2, 1]
    ivs = [(2, 0, len(messy))]
    for a, b in gaps:
        ivs += [(2, a - 10, a), (2, a - 10, a + 1), (2, b - 1, b + 1), (2, b, b + 1), (2, a, b), (2, a - 1, b + 1)]
        ivs += [(2, b - 1, min(b + 10, len(messy))), (2, b, min(b + 10, len(messy)))]
    offs, blob, inexact = world["batch"].fetch(np.array(ivs, np.int64))
    exact_want = [False] + [True, False, False, True, False, False, False, True] * len(gaps)
    assert (~inexact).tolist() == exact_want
    _check_fetch(world, ivs)
    # an interval that touches a run boundary by one base carries N exactly there
    a, b = gaps[0]
    o = offs.astype(np.int64)
    assert blob[o[2]:o[3]].decode().endswith("N") and "N" not in blob[o[2]:o[3] - 1].decode()
    assert blob[o[7]:o[8]].decode().startswith("N") and "N" not in blob[o[7] + 1:o[8]].decode()


def test_fetch_refuses_intervals_outside_their_record(world):
    b = world["batch"]
    n1 = len(world["texts"][1])
    for bad, name in (((1, 0, n1 + 1), "interval 1"), ((1, 5, 4), "interval 1"), ((6, 0, 0), "interval 1"), ((SINGLE, 0, 2), "interval 1")):
        with pytest.raises(ValueError, match=name):
            b.fetch(np.array([(0, 0, 4), bad, (9, 9, 1)], np.int64))
    with pytest.raises(ValueError):
        b.edit_distances(np.array([(0, 0, 4)]), np.array([(1, 5, n1 + 1)]))
    with pytest.raises(ValueError):
        b.edit_distances(np.array([(0, 8, 4)]), np.array([(1, 5, 9)]))
    assert b.fetch(np.zeros((0, 3), np.int64))[1] == b""


def test_fetch_in_several_launches(world, monkeypatch):
    """70 000 one-base intervals with the launch bound lowered to 64 workgroups: 4 096 intervals per launch (16 per wave by the
    grid stride), 18 launches."""
    rng = np.random.default_rng(4)
    n1 = len(world["texts"][1])
    pos = rng.integers(0, n1, 70_000)
    ivs = np.stack([np.ones_like(pos), pos, pos + 1], axis=1)
    monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "64")
    offs, blob, inexact, st = world["batch"].fetch(ivs, stats=True)
    assert st["launches"] == 18 and st["bytes"] == 70_000
    assert blob == np.frombuffer(world["texts"][1].encode(), np.uint8)[pos].tobytes() and not inexact.any()
    assert np.array_equal(offs, np.arange(70_001, dtype=np.uint64))
    monkeypatch.delenv("SEQWIN_AMD_SEQ_MAX_BLOCKS")
    assert world["batch"].fetch(ivs, stats=True)[3]["launches"] == 1


@pytest.mark.parametrize("cap", [None, 1, 2], ids=["default", "cap1", "cap2"])
def test_distances_on_both_routes(world, monkeypatch, cap):
    """Every crafted pair with the default bound (64 pattern blocks: only the 65-block pattern is striped) and with the bound at
    1 and 2 blocks, where patterns of 1 / 2 blocks sit exactly at it and those of 2 / 3 one above."""
    if cap is None:
        monkeypatch.delenv("SEQWIN_AMD_DIST_LDS_CAP", raising=False)
    else:
        monkeypatch.setenv("SEQWIN_AMD_DIST_LDS_CAP", str(cap))
    r = np.array([a for a, _ in world["pairs"]], np.int64)
    s = np.array([b for _, b in world["pairs"]], np.int64)
    dist, strand, st = world["batch"].edit_distances(r, s, stats=True)
    want = np.array(world["want"], np.int64)
    assert np.array_equal(dist, want[:, 0].astype(np.uint32)) and np.array_equal(strand, want[:, 1].astype(np.uint8))
    shorter = np.minimum(r[:, 2] - r[:, 1], s[:, 2] - s[:, 1])
    blocks = (shorter + 63) // 64
    assert st["block_cap"] == (cap or 64) and st["pairs"] == len(r)
    assert st["striped_pairs"] == int((blocks > (cap or 64)).sum()) > 0
    assert st["cells"] == int(((r[:, 2] - r[:, 1]) * (s[:, 2] - s[:, 1])).sum()) and st["longest"] == 4160
    if cap is not None:   # pairs exactly at the bound and one above it are in the set
        assert (blocks == cap).any() and (blocks == cap + 1).any()


def test_the_crafted_pairs_hold_the_named_cases(world):
    want = dict(zip(map(tuple, world["pairs"]), world["want"]))
    assert (0, 1) in want.values() and (2, 0) in want.values()          # a pure reverse complement; the tie that is no zero
    assert sum(1 for v in world["want"] if v == (0, 0)) >= 9             # the unedited equal-length grid pairs, the palindrome, two empty sides
    empties = [(a, b) for a, b in world["pairs"] if a[1] == a[2] or b[1] == b[2]]
    assert [want[e] for e in empties] == [(4096, 0), (1, 0), (0, 0)]
    # a clean interval against its copy with invalid bases in another record: every invalid base costs one edit
    assert want[((LONG, 2000, 2100), (MESSY2, 0, 100))] == (4, 0) == want[((MESSY2, 0, 100), (LONG, 2000, 2100))]
    assert want[((LONG, 2000, 2300), (MESSY2, 0, 300))] == (10, 0) and want[((LONG, 2040, 2060), (MESSY2, 40, 60))] == (1, 0)
    assert sum(1 for a, b in world["pairs"] if a[0] != b[0]) >= 30
