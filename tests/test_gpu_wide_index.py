"""GPU: the query layer on a batch whose batch-wide base index passes 2^32.  Every feature behind the index build addresses the
resident batch by a 64-bit base index (rec_base[r] + pos, run_base[r] + first, the oligo site keys, the rollers' pos, load_codes,
the run and tile searches); their own tests run on kilobases.  Here: 10 synthetic genomes of one record of 480 000 011 bases, so that
records 0-7 lie below 2^32, record 8 straddles it at its position 454 967 040 and record 9 lies above it, and two shards of the same
job -- genomes [0, 2) and [8, 10) -- in which every index is below 2^30.

Two references, neither the code under test at a wide index (tests/tools/wide_host.py):
* pair lists (fetch, row edit distances, infix distances, infix alignments with ops, local alignments, infix pileup, infix windows):
  the host restatements on a model whose records are the pairs' text windows, fetched from the shards;
* whole-batch walks (oligo hits with sites on the Hamming and on the edit route, screen with and without the k-mer profile, MinHash,
  best hits plain / align / loci / seed_copies / local / pileup / windows): the columns of genomes 0-1 and 8-9 equal the shards'
  results in every field, and every planted item is found where it was cut from.  The edit route's sites are also those of
  tests/tools/oligo_edit_host.py on excerpts of 100 bases to either side of every planted place.
Items are cut so that they end at the last base below 2^32, start at 2^32, span it, and lie in the first and the last window of
record 9 (its last packed word is partial); one control lies in record 0.  Everything runs without a hook, with the hit buffer and
the oligo site / candidate buffer lowered (several chunks on the wide batch), and with one workgroup per launch of the list kernels;
the screen with a profile also with a bitmap row per chunk, the edit scan also in several launches."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import hits_host as H  # noqa: E402
import kprofile_host as KP  # noqa: E402
import local_host as LH  # noqa: E402
import oligo_edit_host as OE  # noqa: E402
import pileup_host as PH  # noqa: E402
import seqs_host as SH  # noqa: E402
import wide_host as W  # noqa: E402
import windows_host as WH  # noqa: E402

pytestmark = pytest.mark.gpu

G, L, SEED, K = 10, 480_000_011, 1, 21
BOUND = 1 << 32                       # the first batch-wide base index that needs 33 bits
PAD = (L + 31) // 32 * 32             # every record starts on a 32-base boundary
X = BOUND - 8 * PAD                   # the position of record 8 whose batch-wide index is BOUND
CTRL = 1_000_003                      # the control place in record 0
NO_HIT = W.NO_HIT
BLASTN = (2, -3, 5, 2)
HIT_BUFFER_BYTES = 1 << 30            # the library's default budget of the hit buffer
HOOKS = ("none", "buffers", "list_launches")
EDIT_ARGS = ((0, 0), (1, 3), (2, 0))  # (max_edits, three_prime) of the oligo search with indels
WINDOW_LENGTHS = (8, 20, 32)          # of the oligo windows on the pair list: the shortest, a usual and the longest
WINDOW_ARGS = ((2, 3), (0, 8), (2, 0))   # their (max_mismatch, three_prime)


# ---- the batches ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batches():
    import torch

    from seqwin_amd.device import Batch, pool_trim, set_device
    set_device(0)
    pool_trim()                        # blocks the pool keeps from earlier tests are not free to the driver
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(0)
    need = (G + 4) * (PAD // 4) + HIT_BUFFER_BYTES + (1 << 30)
    assert free >= need, (f"the wide-index tests need {need >> 20} MiB of free device memory (three synthetic batches of {G}, 2 and 2 genomes of "
                          f"{L} bases, the default hit buffer, 1 GiB of work space); the device has {free >> 20} MiB free")
    wide = Batch.synthetic(G, 1, L, seed=SEED)
    lo = Batch.synthetic(2, 1, L, seed=SEED, first_genome=0)
    hi = Batch.synthetic(2, 1, L, seed=SEED, first_genome=8)
    ro = wide.record_offsets().astype(np.int64)
    assert ro.tolist() == list(range(G + 1)) and wide.info()["total_bp"] == G * L      # one record per genome: assembly a is record a
    assert L % 32 != 0 and L % 16 != 0 and PAD == 480_000_032
    rec_base = np.arange(int(ro[-1]), dtype=np.int64) * PAD                              # records lie one behind the other, padded
    assert (rec_base[:8] + L <= BOUND).all()                                             # records 0-7 lie below 2^32
    assert rec_base[8] < BOUND < rec_base[8] + L and BOUND - rec_base[8] == X == 454_967_040   # record 8 straddles it
    assert rec_base[9] >= BOUND                                                          # record 9 lies wholly above it
    assert X % 16 == 0 and 0 < X - 1000 and X + 1000 < L
    for shard in (lo, hi):
        assert shard.record_offsets().tolist() == [0, 1, 2] and 2 * PAD < 1 << 30
    yield SimpleNamespace(wide=wide, lo=lo, hi=hi)
    for b in (wide, lo, hi):
        b.close()


def _shard_of(batches, rec):
    """(shard, its record index, the shard's first record) of a record that a shard holds"""
    if rec < 2:
        return batches.lo, rec, 0
    assert rec >= 8
    return batches.hi, rec - 8, 8


def _texts(batches, intervals):
    """the text of (record, start, stop) intervals of the wide batch, fetched from the shards"""
    out = [None] * len(intervals)
    assert all(r in (0, 1, 8, 9) for r, _, _ in intervals)
    for shard, r0 in ((batches.lo, 0), (batches.hi, 8)):
        mine = [i for i, (r, _, _) in enumerate(intervals) if (r < 2) == (r0 == 0)]
        if not mine:
            continue
        offs, blob, inexact = shard.fetch([(intervals[i][0] - r0, intervals[i][1], intervals[i][2]) for i in mine])
        assert not inexact.any()
        for j, i in enumerate(mine):
            out[i] = blob[int(offs[j]):int(offs[j + 1])]
    return out


def _edited(seq, sub_at, ins_at, del_at):
    """seq with one substitution, one inserted base and one deleted base (given from the back to the front)"""
    s = bytearray(seq)
    assert sub_at < del_at < ins_at < len(s)
    s[ins_at:ins_at] = b"ACGT"["ACGT".index(chr(s[ins_at])) ^ 2:][:1]
    del s[del_at]
    s[sub_at] = ord("ACGT"["ACGT".index(chr(s[sub_at])) ^ 1])
    return bytes(s)


@pytest.fixture(params=HOOKS)
def hook(request, monkeypatch, sizes):
    if request.param == "buffers":
        monkeypatch.setenv("SEQWIN_AMD_HIT_BUFFER_KB", str(sizes.hit_kb))
        monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", str(sizes.oligo_kb))
    elif request.param == "list_launches":
        monkeypatch.setenv("SEQWIN_AMD_SEQ_MAX_BLOCKS", "1")
    return request.param


# ---- planted queries and oligos ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted(batches):
    """Queries (k = 21) and oligos cut from fetched text: (record, start, length, strand) each; strand 1 is given reverse-complemented.
    The spanning query overlaps the two at the crossing, so the unique-seed rule drops the shared windows and seed_copies=2 keeps them."""
    q_places = [(8, X - 260, 260, 0),            # ends with the last base below 2^32
                (8, X, 260, 1),                  # starts with base 2^32
                (8, X - 133, 300, 0),            # spans it; the crossing lies at offset 5 of a packed word of the query
                (9, 0, 200, 0),                  # the first window of record 9
                (9, L - 250, 250, 1),            # the last window of record 9, flush with its end
                (0, CTRL, 220, 0)]               # the control
    o_places = [(8, X - 32, 32, 0), (8, X, 20, 1), (8, X - 13, 27, 0), (8, X - 5, 21, 1), (9, 0, 25, 0), (9, L - 32, 32, 1), (9, L - 20, 20, 0),
                (0, CTRL, 24, 0), (8, X - 20, 20, 0)]

    def cut(places):
        texts = _texts(batches, [(r, s, s + n) for r, s, n, _ in places])
        return [H.revcomp(t) if strand else t for t, (_, _, _, strand) in zip(texts, places)]
    return SimpleNamespace(q_places=q_places, queries=cut(q_places), o_places=o_places, oligos=cut(o_places))


@pytest.fixture(scope="module")
def sizes(batches, planted, edit_case):
    """The buffer hooks, from the hits of the plain calls on the wide batch: a hit buffer that holds one assembly's keys and not
    two's (16 bytes a key with the sort's second buffer), a site buffer below one assembly's sites, and for the edit route a
    candidate buffer below one assembly's candidates (8 bytes each; every candidate becomes a site, so `hits` counts them) in the
    call that has the fewest."""
    h = batches.wide.best_hits(planted.queries, K)
    st = h.stats()
    h.close()
    assert st["chunks"] == 1 and st["hits"] >= G * len(planted.queries)
    o = batches.wide.oligo_hits(planted.oligos, 1, sites=True)
    so = o.stats()
    o.close()
    assert so["chunks"] == 1 and so["hits"] >= len(planted.oligos)
    edit_hits = []
    for d, c in EDIT_ARGS:
        o = batches.wide.oligo_hits(edit_case.oligos, three_prime=c, max_edits=d)
        se = o.stats()
        o.close()
        assert se["chunks"] == 1 and se["candidates"] == se["hits"] >= len(planted.oligos), se
        edit_hits.append(se["hits"])
    return SimpleNamespace(hit_kb=max(1, (st["hits"] // G * 16 * 5 // 4) // 1024), oligo_kb=(so["hits"] // G * 8 // 2) // 1024,
                           oligo_edit_kb=(min(edit_hits) // G * 8 // 2) // 1024)


# ---- pair lists: the host restatements on excerpts ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pair_case(batches):
    """Queries cut around the crossing, at both ends of record 9 and at the control place -- one of 700 bases (more than the 64 x 8 rows
    of one pass of the local kernel), two with an edit of every kind -- and pairs whose text windows start 1, 15, 16 and 17 bases
    before the crossing, end at it, start at it, span it, lie in record 9 and in record 0, on both strands; the restatements' results
    on the excerpt model."""
    cuts = [(8, X - 40, 129), (8, X - 40, 129), (8, X - 350, 700), (9, 0, 65), (9, L - 100, 100), (0, CTRL, 80), (8, X + 3, 90), (8, X - 95, 90),
            (8, X - 33, 70), (8, X - 60, 120)]
    queries = _texts(batches, [(r, s, s + n) for r, s, n in cuts])
    queries[1] = _edited(queries[1], 30, 90, 60)
    queries[2] = _edited(queries[2], 100, 600, 340)
    queries[8] = H.revcomp(queries[8])
    queries[9] = H.revcomp(_edited(queries[9], 25, 95, 60))                        # an edit of every kind, piled on strand 1
    pairs = []
    for d in (1, 15, 16, 17):
        pairs += [(6, 0, 8, X - d, X + 150), (1, 0, 8, X - d, X + 120)]
    pairs += [(7, 0, 8, X - 200, X), (0, 0, 8, X - 200, X),                        # the window's last base is the last below 2^32
              (6, 0, 8, X, X + 200), (0, 0, 8, X, X + 200),                        # its first base is base 2^32
              (0, 0, 8, X - 100, X + 150), (1, 0, 8, X - 101, X + 153), (1, 1, 8, X - 101, X + 153),
              (8, 1, 8, X - 133, X + 99), (8, 0, 8, X - 133, X + 99),              # strand 1: the reverse-complemented query's copy
              (2, 0, 8, X - 450, X + 450), (2, 0, 8, X - 550, X + 550), (2, 1, 8, X - 450, X + 450),   # 700 rows: carry rows in LDS and in HBM
              (3, 0, 9, 0, 200), (3, 0, 9, 0, 65), (3, 1, 9, 0, 100),
              (4, 0, 9, L - 300, L), (4, 0, 9, L - 100, L), (4, 0, 9, L - 37, L), (4, 1, 9, L - 300, L),
              (5, 0, 0, CTRL - 50, CTRL + 150),
              (0, 0, 9, X - 100, X + 150), (0, 0, 0, X - 100, X + 150), (1, 0, 9, X - 60, X + 130),      # the near-copies of other genomes
              (0, 0, 9, 5, 5), (0, 0, 8, X, X),                                    # empty texts
              (9, 1, 8, X - 80, X + 80)]                                           # strand 1 with a mismatch, an insertion and a deletion
    texts = _texts(batches, [(r, a, z) for _, _, r, a, z in pairs])
    records, model, starts = W.excerpt_model(pairs, texts)
    infix = W.shift_back(dict(zip(("dist", "end"), H.infix(queries, records, model))), starts)
    al_model = A.alignments(queries, records, model)
    local = W.shift_back(LH.alignments(queries, records, model, BLASTN), starts)
    groups = np.array([(0, 1, 2, 255)[i % 4] for i in range(len(pairs))], np.uint8)
    pile = PH.pile_ops(queries, records, model, groups, 3, 300, al=al_model)
    assert pile["piled"].any() and not pile["piled"].all() and pile["table"][:, :, PH.DEL].any() and pile["table"][:, :, PH.INS].any()
    windows = {(mm, c3): WH.windows_ops(queries, records, model, groups, 3, WINDOW_LENGTHS, mm, c3, 300, al=al_model) for mm, c3 in WINDOW_ARGS}
    o = al_model["offsets"].astype(np.int64)

    def imperfect(i):
        """whether the piled pair i has a window with a mismatch and a window with an indel"""
        rows = np.zeros((len(queries[pairs[i][0]]), len(WINDOW_LENGTHS), 3, 8), np.uint32)
        WH.add_script_prefix(rows, int(groups[i]), pairs[i][1], al_model["ops"][o[i]:o[i + 1]], list(WINDOW_LENGTHS), 2, 3)
        return bool(rows[..., WH.MM1:WH.MM4P + 1].any() and rows[..., WH.GAPPED].any())
    for strand in (0, 1):                                                          # the walk is exercised beyond MM0 on either strand
        assert any(imperfect(i) for i in np.flatnonzero(pile["piled"] & (np.array(pairs)[:, 1] == strand))), strand
    return SimpleNamespace(queries=queries, pairs=np.array(pairs, np.int64), texts=texts, infix=infix, al=W.shift_back(al_model, starts), local=local,
                           groups=groups, pile=pile, windows=windows)


def test_fetch_and_row_edit_distances(batches, pair_case, hook):
    """Batch.fetch of windows at, around and above 2^32 gives the shards' text; Batch.edit_distances of such windows gives the host's
    Levenshtein distance of the shards' text."""
    iv = [(int(r), int(a), int(z)) for _, _, r, a, z in pair_case.pairs] + [(8, X - 1, X + 1), (8, X - 16, X), (8, X, X + 16), (9, L - 11, L), (9, L - 27, L - 11)]
    want = pair_case.texts + _texts(batches, iv[len(pair_case.texts):])
    offs, blob, inexact = batches.wide.fetch(iv)
    assert not inexact.any() and offs.tolist() == np.concatenate(([0], np.cumsum([len(t) for t in want]))).tolist()
    assert blob == b"".join(want)
    r = [(8, X - d, X - d + 100) for d in (1, 15, 16, 17, 50)] + [(9, L - 80, L), (9, 0, 70), (0, CTRL, CTRL + 90), (8, X - 300, X + 300)]
    s = [(9, X - d + 2, X - d + 98) for d in (1, 15, 16, 17, 50)] + [(8, L - 77, L), (0, 0, 64), (9, CTRL + 3, CTRL + 90), (9, X - 290, X + 310)]
    tr, ts = _texts(batches, r), _texts(batches, s)
    ref = [SH.distance(a, b) for a, b in zip(tr, ts)]
    dist, strand = batches.wide.edit_distances(r, s)
    assert dist.tolist() == [d for d, _ in ref] and strand.tolist() == [o for _, o in ref]
    assert max(dist[:5]) < 20                                                       # near-copies of one ancestor, 1 % apart, 2 bases longer at either end


def test_infix_distances(batches, pair_case, hook):
    c = pair_case
    dist, end, st = batches.wide.infix_distances(c.queries, c.pairs, stats=True)
    assert np.array_equal(dist, c.infix["dist"]) and np.array_equal(end, c.infix["end"]), (dist.tolist(), c.infix["dist"].tolist(), end.tolist(),
                                                                                            c.infix["end"].tolist())
    assert st["pairs"] == len(c.pairs) and st["longest"] == 700
    by = {tuple(p): i for i, p in enumerate(c.pairs.tolist())}
    for pair, e in (((6, 0, 8, X - 1, X + 150), X + 93), ((7, 0, 8, X - 200, X), X - 5), ((6, 0, 8, X, X + 200), X + 93), ((0, 0, 8, X - 100, X + 150), X + 89),
                    ((8, 1, 8, X - 133, X + 99), X + 37), ((3, 0, 9, 0, 65), 65), ((4, 0, 9, L - 300, L), L), ((5, 0, 0, CTRL - 50, CTRL + 150), CTRL + 80)):
        assert (dist[by[pair]], end[by[pair]]) == (0, e), pair                    # the exact copies, where they were cut


def test_infix_alignments_with_ops(batches, pair_case, hook):
    c = pair_case
    got = batches.wide.infix_alignments(c.queries, c.pairs, ops=True)
    for f, a in zip(A.FIELDS + ("offsets", "ops"), got):
        assert a.dtype == c.al[f].dtype and np.array_equal(a, c.al[f]), (f, a.tolist()[:40], c.al[f].tolist()[:40])
    i = c.pairs.tolist().index([1, 0, 8, X - 101, X + 153])                         # the edited query: one X, one I, one D
    assert (got[0][i], got[4][i], got[5][i]) == (3, 1, 2)


def test_local_alignments(batches, pair_case, hook):
    c = pair_case
    got = batches.wide.local_alignments(c.queries, c.pairs, BLASTN, stats=True)
    for f in LH.FIELDS:
        assert np.array_equal(got[f], c.local[f]), (f, got[f].tolist(), c.local[f].tolist())
    assert got["stats"]["striped_pairs"] == 3 and got["stats"]["hbm_carry_pairs"] >= 1 and got["stats"]["pass_rows"] == 512
    LH.check({f: got[f] for f in LH.FIELDS}, BLASTN)
    i = c.pairs.tolist().index([8, 1, 8, X - 133, X + 99])
    assert [int(got[f][i]) for f in ("score", "qstart", "qend", "sstart", "send")] == [140, 0, 70, X - 33, X + 37]


def test_infix_pileup(batches, pair_case, hook):
    c = pair_case
    pile, al = batches.wide.infix_pileup(c.queries, c.pairs, c.groups, n_groups=3, max_dist_permille=300)
    try:
        for f, a in zip(A.FIELDS, al):
            assert np.array_equal(a, c.al[f]), f
        offs, table = pile.table()
        assert np.array_equal(offs.astype(np.int64), c.pile["q_offsets"]) and np.array_equal(table, c.pile["table"])
        assert np.array_equal(pile.depth(), c.pile["depth"]) and pile.stats()["piled"] == int(c.pile["piled"].sum())
    finally:
        pile.close()


@pytest.mark.parametrize("max_mismatch,three_prime", WINDOW_ARGS)
def test_infix_windows(batches, pair_case, hook, max_mismatch, three_prime):
    """The window walk reads the text a third time: its table, the pileup it fills beside it and the alignment arrays are the host's
    on the excerpts (tests/tools/windows_host.py)."""
    c = pair_case
    want = c.windows[max_mismatch, three_prime]
    win, pile, al = batches.wide.infix_windows(c.queries, c.pairs, c.groups, lengths=WINDOW_LENGTHS, n_groups=3, max_dist_permille=300,
                                               max_mismatch=max_mismatch, three_prime=three_prime)
    try:
        for f, a in zip(A.FIELDS, al):
            assert np.array_equal(a, c.al[f]), f
        offs, wtable = win.table()
        assert win.lengths == WINDOW_LENGTHS and win.sizes()[4:] == (max_mismatch, three_prime)
        assert np.array_equal(offs.astype(np.int64), want["q_offsets"]) and wtable.dtype == want["wtable"].dtype
        assert np.array_equal(wtable, want["wtable"]), np.argwhere(wtable != want["wtable"])[:10].tolist()
        p_offs, table = pile.table()
        assert np.array_equal(p_offs.astype(np.int64), c.pile["q_offsets"]) and np.array_equal(table, c.pile["table"])
        assert np.array_equal(pile.depth(), c.pile["depth"]) and np.array_equal(pile.depth(), want["depth"])
        assert pile.stats()["piled"] == int(want["piled"].sum()) == int(c.pile["piled"].sum())
        WH.invariants(wtable, pile.depth(), offs, WINDOW_LENGTHS)
        assert wtable[..., WH.MM1:WH.MM4P + 1].any() and wtable[..., WH.GAPPED].any()
    finally:
        win.close()
        pile.close()


# ---- whole-batch walks: the shards' results, and the planted items --------------------------------------------------------------------

OLIGO_MATRICES = ("n_sites", "best_mm", "best_record", "best_pos", "best_strand")
SITE_FIELDS = ("oligo", "assembly", "record", "pos", "strand", "mm")


def _oligo_fields(batch, oligos):
    o = batch.oligo_hits(oligos, 1, sites=True)
    try:
        out = {f: getattr(o, f)() for f in OLIGO_MATRICES}
        out["sites"], out["stats"] = o.sites(), o.stats()
        return out
    finally:
        o.close()


@pytest.fixture(scope="module")
def oligo_shards(batches, planted):
    return _oligo_fields(batches.lo, planted.oligos), _oligo_fields(batches.hi, planted.oligos)


def test_oligo_hits_with_sites(batches, planted, oligo_shards, hook):
    nq = len(planted.oligos)
    assert sorted({len(o) for o in planted.oligos}) == [20, 21, 24, 25, 27, 32]
    w = _oligo_fields(batches.wide, planted.oligos)
    for shard, c0 in zip(oligo_shards, (0, 8)):
        W.assert_columns(w, shard, OLIGO_MATRICES, c0, c0, ("oligo hits", c0))
        W.assert_list(w["sites"], shard["sites"], SITE_FIELDS, nq, G, c0, c0, ("oligo sites", c0))
    S = w["sites"]
    assert int(w["n_sites"].sum()) == len(S["oligo"]) == w["stats"]["hits"]
    for i, (rec, start, _, strand) in enumerate(planted.o_places):
        assert w["best_mm"][i, rec] == 0 and w["n_sites"][i, rec] >= 1, i
        assert W.has_entry(S, oligo=i, assembly=rec, record=rec, pos=start, strand=strand, mm=0), (i, rec, start, strand)
    if hook == "buffers":
        assert w["stats"]["chunks"] > 1 and w["stats"]["chunk_splits"] >= 1, w["stats"]
    else:
        assert w["stats"]["chunks"] == 1


# ---- the oligo search with indels: its own candidate, site and best keys, anchors, decoders and text readers -----------------------------

EDIT_MATRICES = ("n_sites", "best_dist", "best_record", "best_pos", "best_strand", "best_end", "best_mismatch", "best_gaps")
EDIT_EXCERPT = 100                    # bases of an excerpt to either side of a planted place
# Workgroups per launch of the edit scan in the launch-split case: 2^18, i.e. 2^20 tiles of 1024 ends, 5 launches on the 4 687 500 tiles
# of this batch; the crossing lies in tile 2^22 - 1 (record 8 starts at tile 3 750 000, X // 1024 = 444 303), so the launch that starts
# at tile 2^22 starts 256 bases behind it.  One workgroup per launch (the value the small tests use) is 1.17 M launches here: measured
# at 57 us a launch on one shard (234 375 launches, 13.5 s), about 67 s on the wide batch -- no test for a suite.
EDIT_SCAN_BLOCKS = str(1 << 18)


@pytest.fixture(scope="module")
def edit_case(batches, planted):
    """The planted oligos and, cut from the same places, oligos with a bulge: one base deleted from the oligo (the text has a base
    more: the site is the whole place) and one base inserted into it (a place of 32 bases gives its last 31 and the base, so that
    the oligo keeps to 32 letters and the site stays flush with the place's end), each edit 5 letters or more from either end.
    `sites`: (oligo, record, pos, end, strand, dist) of every planted site; `excerpts`: (record, lo, hi, text, the oligos cut there).
    The bulged sites [X - 24, X) on strand 0 and [X, X + 23) on strand 1 have the candidate anchors 2^32 - 1 and 2^32."""
    bulged = [(8, X - 13, 27, 0), (8, X - 5, 21, 1), (8, X, 20, 1), (9, L - 32, 32, 1), (0, CTRL, 24, 0),
              (8, X - 24, 24, 0),      # strand 0, ends with the last base below 2^32: the anchor e - 1 is index 2^32 - 1
              (8, X, 23, 1)]           # strand 1, starts with base 2^32: the anchor n - e is index 2^32
    assert all(p in planted.o_places for p in bulged[:5])
    oligos = list(planted.oligos)
    sites = [(i, r, s, s + n, strand, 0) for i, (r, s, n, strand) in enumerate(planted.o_places)]
    cut_at = {(r, s, n): [i] for i, (r, s, n, _) in enumerate(planted.o_places)}
    for (r, s, n, strand), text in zip(bulged, _texts(batches, [(r, s, s + n) for r, s, n, _ in bulged])):
        skip = 1 if n == 32 else 0
        for variant, pos in ((W.deleted(text), s), (W.inserted(text[skip:]), s + skip)):
            assert 19 <= len(variant) <= 32
            cut_at.setdefault((r, s, n), []).append(len(oligos))
            sites.append((len(oligos), r, pos, s + n, strand, 1))
            oligos.append(H.revcomp(variant) if strand else variant)
    assert len(set(oligos)) == len(oligos) == len(planted.oligos) + 2 * len(bulged)
    iv = [(r, max(0, s - EDIT_EXCERPT), min(L, s + n + EDIT_EXCERPT)) for r, s, n in cut_at]
    excerpts = [(r, lo, hi, text, ids) for (r, lo, hi), text, ids in zip(iv, _texts(batches, iv), cut_at.values())]
    assert any(lo == 0 for _, lo, _, _, _ in excerpts) and any(hi == L for _, _, hi, _, _ in excerpts)       # both ends of record 9
    return SimpleNamespace(oligos=oligos, sites=sites, excerpts=excerpts)


def _oligo_edit_fields(batch, oligos, d, c):
    o = batch.oligo_hits(oligos, three_prime=c, sites=True, max_edits=d)
    try:
        out = {f: getattr(o, f)() for f in EDIT_MATRICES}
        out["sites"], out["stats"] = o.sites(), o.stats()
        return out
    finally:
        o.close()


@pytest.fixture(scope="module")
def edit_refs(batches, edit_case):
    """Per (max_edits, three_prime): the shards' results, and per excerpt the restatement's sites (the matrix form) of the oligos
    cut there that the excerpt alone decides (wide_host.EDIT_MARGIN), as rows over OE.SITE_FIELDS at their place in the wide batch."""
    out = {}
    for d, c in EDIT_ARGS:
        want = []
        for rec, lo, hi, text, ids in edit_case.excerpts:
            a, z = W.interior(lo, hi, L)
            rows = [(ids[q], rec, rec, lo + pos, lo + end, s, v, nx, ng)
                    for q, _, _, pos, end, s, v, nx, ng in OE.sites_matrix([edit_case.oligos[i] for i in ids], [[text]], d, c) if a <= lo + pos and lo + end <= z]
            want.append((rec, a, z, ids, sorted(rows)))
        out[d, c] = SimpleNamespace(shards=(_oligo_edit_fields(batches.lo, edit_case.oligos, d, c), _oligo_edit_fields(batches.hi, edit_case.oligos, d, c)),
                                    excerpts=want)
    return out


def _check_edit_result(w, edit_case, ref, d):
    """What every run of the edit route on the wide batch must give, whatever the hook."""
    nq, S = len(edit_case.oligos), w["sites"]
    for shard, c0 in zip(ref.shards, (0, 8)):
        W.assert_columns(w, shard, EDIT_MATRICES, c0, c0, ("oligo edit hits", d, c0))
        W.assert_list(S, shard["sites"], OE.SITE_FIELDS, nq, G, c0, c0, ("oligo edit sites", d, c0))
    assert int(w["n_sites"].sum()) == len(S["oligo"]) == w["stats"]["hits"]
    rec, pos, end, oligo = (S[f].astype(np.int64) for f in ("record", "pos", "end", "oligo"))
    for r, a, z, ids, want in ref.excerpts:
        got = W.rows_of(S, OE.SITE_FIELDS, (rec == r) & (pos >= a) & (end <= z) & np.isin(oligo, ids))
        assert sorted(got) == want, (d, r, a, z, got, want)
    for i, r, p, e, strand, dist in edit_case.sites:
        there = W.has_entry(S, oligo=i, assembly=r, record=r, pos=p, end=e, strand=strand, dist=dist, mismatch=0, gaps=dist)
        if dist <= d:
            assert there and w["best_dist"][i, r] == dist and w["n_sites"][i, r] >= 1, (d, i, r, p, e, strand, dist)
        else:                                                                        # a bulged oligo at max_edits 0: nothing at its place
            assert not ((oligo == i) & (rec == r) & (end > p - 8) & (pos < e + 8)).any(), (d, i, r, p, e)


@pytest.mark.parametrize("max_edits,three_prime", EDIT_ARGS)
def test_oligo_hits_edit_with_sites(batches, edit_case, edit_refs, sizes, hook, monkeypatch, max_edits, three_prime):
    """The edit route packs the batch-wide index into three keys of its own (candidate, site, best), forms its anchors per strand and
    reads the text through its own readers: every matrix and the site list against the shards and against the restatement on excerpts,
    exact and bulged oligos where they were cut -- among them sites whose candidate anchors are the indices 2^32 - 1 and 2^32."""
    if hook == "buffers":                                                            # below one assembly's candidates
        monkeypatch.setenv("SEQWIN_AMD_OLIGO_BUFFER_KB", str(sizes.oligo_edit_kb))
    w = _oligo_edit_fields(batches.wide, edit_case.oligos, max_edits, three_prime)
    _check_edit_result(w, edit_case, edit_refs[max_edits, three_prime], max_edits)
    if (max_edits, three_prime) == (0, 0):                                           # "max_edits=0 gives the sites of max_mismatch=0"
        o = batches.wide.oligo_hits(edit_case.oligos, 0, sites=True)
        try:
            hamming = o.sites()
        finally:
            o.close()
        for f in ("oligo", "assembly", "record", "pos", "strand", "cell_offsets"):
            assert np.array_equal(w["sites"][f], hamming[f]), f
    if hook == "buffers":
        assert w["stats"]["chunks"] > 1 and w["stats"]["chunk_splits"] >= 1, w["stats"]
    else:
        assert w["stats"]["chunks"] == 1 and w["stats"]["launches"] == 1, w["stats"]


def test_oligo_hits_edit_scan_launches(batches, edit_case, edit_refs, monkeypatch):
    """The launch split of the edit scan (the 15 000-genome set needs it by its size)."""
    monkeypatch.setenv("SEQWIN_AMD_OLIGO_MAX_BLOCKS", EDIT_SCAN_BLOCKS)
    w = _oligo_edit_fields(batches.wide, edit_case.oligos, 1, 3)
    _check_edit_result(w, edit_case, edit_refs[1, 3], 1)
    k = min(len(o) for o in edit_case.oligos) - 1                                    # a site spans L - max_edits bases or more
    tiles = G * -(-(L - k + 1) // 1024)                                              # four tiles to a workgroup
    assert w["stats"]["chunks"] == 1 and w["stats"]["launches"] == -(-tiles // (4 * int(EDIT_SCAN_BLOCKS))) == 5, w["stats"]


@pytest.fixture(scope="module")
def screen_shards(batches, planted):
    out = []
    for b in (batches.lo, batches.hi):
        s = b.screen(planted.queries, K)
        out.append(dict(n_kmers=s.n_kmers(), counts=s.counts()))
        s.close()
    return out


def test_screen(batches, planted, screen_shards, hook):
    s = batches.wide.screen(planted.queries, K)
    try:
        w = dict(n_kmers=s.n_kmers(), counts=s.counts())
    finally:
        s.close()
    for shard, c0 in zip(screen_shards, (0, 8)):
        assert np.array_equal(w["n_kmers"], shard["n_kmers"])
        W.assert_columns(w, shard, ("counts",), c0, c0, ("screen", c0))
    for i, (rec, _, n, _) in enumerate(planted.q_places):
        assert w["n_kmers"][i] == n - K + 1 and w["counts"][i, rec] == n - K + 1, i     # every k-mer of a query lies where it was cut


def _profile_fields(batch, queries, groups, copies):
    s = batch.screen(queries, K, profile=groups, copies=copies)
    try:
        p = s.profile()
        offs, present, cop = p.table()
        return dict(n_kmers=s.n_kmers(), counts=s.counts(), offs=offs.astype(np.int64), present=present, copies=cop, group_sizes=p.group_sizes(),
                    stats=s.stats())
    finally:
        s.close()


@pytest.fixture(scope="module")
def profile_shards(batches, planted):
    return {copies: [_profile_fields(b, planted.queries, [0, 0], copies) for b in (batches.lo, batches.hi)] for copies in (False, True)}


@pytest.mark.parametrize("bitmap_kb", (None, "0"))
@pytest.mark.parametrize("copies", (False, True))
def test_screen_profile(batches, planted, screen_shards, profile_shards, hook, monkeypatch, copies, bitmap_kb):
    """The flagged probe k_scr_probe<true> and the profile's kernels on the wide batch: `present` (and `copies`) of the group of
    genomes 0-1 / 8-9 are the shards' at every position; what the call answers without a profile is test_screen's.

    The identity with Screen.counts() (tests/tools/kprofile_host.py: present[p, g] = the assemblies labelled g
    that hold the canonical k-mer of the window at p; counts[i, a] = the distinct canonical k-mers of query i that assembly a holds)
    is asserted in the form that holds whether or not a k-mer repeats inside a query: `present` summed over the FIRST window of every
    distinct canonical k-mer of query i equals counts[i] summed over the assemblies of the group.  Summed over all windows it would
    count a repeated k-mer once per window."""
    if bitmap_kb is not None:
        monkeypatch.setenv("SEQWIN_AMD_SCR_BITMAP_KB", bitmap_kb)                    # a bitmap row per chunk: groups change between chunks
    w = _profile_fields(batches.wide, planted.queries, WIDE_GROUPS, copies)
    assert w["group_sizes"].tolist() == [2, 2] and w["present"].shape == (sum(len(q) for q in planted.queries), 2)
    assert (w["copies"] is not None) == copies
    for g, (shard, plain, c0) in enumerate(zip(profile_shards[copies], screen_shards, (0, 8))):
        assert np.array_equal(w["offs"], shard["offs"])
        assert np.array_equal(w["present"][:, g], shard["present"][:, 0]), (g, np.flatnonzero(w["present"][:, g] != shard["present"][:, 0])[:10].tolist())
        if copies:
            assert np.array_equal(w["copies"][:, g], shard["copies"][:, 0]), (g, np.flatnonzero(w["copies"][:, g] != shard["copies"][:, 0])[:10].tolist())
        assert np.array_equal(w["n_kmers"], plain["n_kmers"])                        # the profile changes nothing the call answers without it
        W.assert_columns(w, plain, ("counts",), c0, c0, ("screen with a profile", c0))
    group_cols = {0: (0, 1), 1: (8, 9)}
    for i, ((rec, _, n, _), q) in enumerate(zip(planted.q_places, planted.queries)):
        assert w["n_kmers"][i] == n - K + 1 and w["counts"][i, rec] == n - K + 1, i
        rows = w["present"][w["offs"][i]:w["offs"][i + 1]]
        assert len(rows) == n and (rows[n - K + 1:] == KP.NO_WINDOW).all() and (rows[:n - K + 1] != KP.NO_WINDOW).all()
        words, valid = KP._words(q, K)
        assert valid.all() and len(words) == n - K + 1
        first = np.unique(words, return_index=True)[1]                               # the first window of every distinct canonical k-mer
        assert len(first) == w["n_kmers"][i]
        for g, cols in group_cols.items():
            assert int(rows[first, g].astype(np.int64).sum()) == int(w["counts"][i, list(cols)].astype(np.int64).sum()), (i, g)
        g = WIDE_GROUPS[rec]                                                         # every k-mer of a query lies where it was cut
        assert (rows[:n - K + 1, g] >= 1).all(), i
        if copies:
            cop = w["copies"][w["offs"][i]:w["offs"][i + 1]]
            assert (cop[n - K + 1:] == KP.NO_WINDOW_COPIES).all() and (cop[:n - K + 1, g] >= 1).all() and (cop[:n - K + 1, g] != KP.NO_WINDOW_COPIES).all(), i
            assert (cop[:n - K + 1] >= rows[:n - K + 1]).all()                       # an assembly that holds a k-mer holds a window of it
    # the spanning query shares windows with queries 0 and 1: the profile has no unique-seed rule, the shared k-mers' rows are theirs
    o = w["offs"]
    (_, s0, n0, _), (_, s1, n1, _), (_, s2, _, _) = planted.q_places[:3]
    shared0 = np.arange(0, s0 + n0 - K + 1 - s2)                                    # windows of query 2 inside query 0 (strand 0)
    shared1 = np.arange(s1 - s2, len(planted.queries[2]) - K + 1)                   # ... inside query 1, which is given reverse-complemented
    assert len(shared0) == 133 - K + 1 and len(shared1) == 300 - 133 - K + 1
    for tab in (w["present"],) + ((w["copies"],) if copies else ()):
        assert np.array_equal(tab[o[2] + shared0], tab[o[0] + shared0 + (s2 - s0)])
        assert np.array_equal(tab[o[2] + shared1], tab[o[1] + (n1 - K) - (shared1 + s2 - s1)])
        assert (tab[o[2] + shared0, 1] >= 1).all() and (tab[o[2] + shared1, 1] >= 1).all()
    if bitmap_kb == "0":
        assert w["stats"]["chunks"] > 1, w["stats"]
    else:
        assert w["stats"]["chunks"] == 1, w["stats"]


def _minhash_fields(batch):
    m = batch.minhash(K, 1000)
    try:
        offs, hashes = m.sketches()
        shared, total = m.counts()
        return dict(offs=offs.astype(np.int64), hashes=hashes, shared=shared, total=total)
    finally:
        m.close()


@pytest.fixture(scope="module")
def minhash_shards(batches):
    return _minhash_fields(batches.lo), _minhash_fields(batches.hi)


def test_minhash(batches, minhash_shards, hook):
    w = _minhash_fields(batches.wide)
    assert np.diff(w["offs"]).tolist() == [1000] * G
    for shard, c0 in zip(minhash_shards, (0, 8)):
        for a in range(2):
            got = w["hashes"][w["offs"][c0 + a]:w["offs"][c0 + a + 1]]
            want = shard["hashes"][shard["offs"][a]:shard["offs"][a + 1]]
            assert np.array_equal(got, want) and (got[1:] > got[:-1]).all(), (c0, a)
        for f in ("shared", "total"):
            assert np.array_equal(w[f][c0:c0 + 2, c0:c0 + 2], shard[f]), (f, c0)
    assert (np.diag(w["shared"]) == 1000).all()


# ---- best hits, every mode -------------------------------------------------------------------------------------------------------------

MATRIX = ("seeds", "record", "strand", "end", "dist")
ALIGNED = ("start", "nident", "mismatch", "gaps")
LOCAL = ("score", "qstart", "qend", "sstart", "send", "local_nident", "local_mismatch", "local_gapopen", "local_gaps")
LOCI = ("n_loci", "sum_nident")
LOCI_LIST = ("query", "assembly", "record", "strand", "band", "seeds", "dist", "end", "start", "nident", "mismatch", "gaps", "dup")
WIDE_GROUPS = [0, 0] + [255] * (G - 4) + [1, 1]      # the pileup's groups on the wide batch: the two shards' assemblies
MODES = {"plain": {}, "align": dict(align=True), "loci": dict(loci=True), "seed_copies": dict(seed_copies=2, align=True), "local": dict(local=True),
         "pileup": dict(pileup=True), "windows": dict(pileup=True, window_lengths=(18, 20, 25))}


def _hit_fields(batch, queries, mode, groups):
    kw = dict(MODES[mode])
    if kw.pop("pileup", False):
        kw.update(pileup=groups)
    h = batch.best_hits(queries, K, **kw)
    try:
        fields = MATRIX + (ALIGNED if mode in ("align", "loci", "seed_copies", "pileup", "windows") else ()) + (LOCAL if mode == "local" else ()) + (LOCI if mode == "loci" else ())
        out = {f: getattr(h, f)() for f in fields}
        out["n_seeds"], out["stats"], out["fields"] = h.n_seeds(), h.stats(), fields
        if mode == "loci":
            out["loci"] = h.loci()
        if mode in ("pileup", "windows"):
            out["table"], out["depth"] = h.pileup().table()[1], h.pileup().depth()
        if mode == "windows":
            out["q_offsets"], out["wtable"] = h.windows().table()
            assert h.windows().lengths == kw["window_lengths"]
        return out
    finally:
        h.close()


@pytest.fixture(scope="module")
def hit_shards(batches, planted):
    return {mode: (_hit_fields(batches.lo, planted.queries, mode, [0, 0]), _hit_fields(batches.hi, planted.queries, mode, [0, 0])) for mode in MODES}


@pytest.mark.parametrize("mode", list(MODES))
def test_best_hits(batches, planted, hit_shards, hook, mode):
    nq = len(planted.queries)
    w = _hit_fields(batches.wide, planted.queries, mode, WIDE_GROUPS)
    for g, (shard, c0) in enumerate(zip(hit_shards[mode], (0, 8))):
        assert np.array_equal(w["n_seeds"], shard["n_seeds"])
        W.assert_columns(w, shard, w["fields"], c0, c0, (mode, c0))
        if mode == "loci":
            W.assert_list(w["loci"], shard["loci"], LOCI_LIST, nq, G, c0, c0, (mode, "loci", c0))
        if mode in ("pileup", "windows"):
            assert np.array_equal(w["table"][:, g, :], shard["table"][:, 0, :]) and np.array_equal(w["depth"][:, g], shard["depth"][:, 0]), (mode, c0)
        if mode == "windows":                                                       # the window table of group g is the shard's group 0
            assert np.array_equal(w["wtable"][:, :, g, :], shard["wtable"][:, :, 0, :]) and np.array_equal(w["q_offsets"], shard["q_offsets"]), (mode, c0)
    # near-copies of one ancestor: a hit in every column (the spanning query: where it keeps more seeds than the K - 1 windows across the crossing)
    assert (w["seeds"][[i for i in range(nq) if i != 2 or mode == "seed_copies"]] > 0).all()
    for i, (rec, start, n, strand) in enumerate(planted.q_places):
        got = {f: int(w[f][i, rec]) for f in w["fields"]}
        assert (got["record"], got["strand"], got["end"], got["dist"]) == (rec, strand, start + n, 0), (mode, i, got)
        if "start" in got:
            assert (got["start"], got["nident"], got["mismatch"], got["gaps"]) == (start, n, 0, 0), (mode, i, got)
        if mode == "local":
            assert [got[f] for f in LOCAL] == [2 * n, 0, n, start, start + n, n, 0, 0, 0], (mode, i, got)
        if mode == "loci":
            assert got["n_loci"] >= 1 and W.has_entry(w["loci"], query=i, assembly=rec, record=rec, strand=strand, dist=0, start=start, end=start + n), (i, got)
        if mode in ("pileup", "windows") and rec in (0, 1, 8, 9):
            assert w["depth"][i, WIDE_GROUPS[rec]] >= 1
        if mode == "windows":                                                       # the exact copy faces every window of every length perfectly
            rows = w["wtable"][int(w["q_offsets"][i]):int(w["q_offsets"][i + 1])]
            for l, length in enumerate(MODES[mode]["window_lengths"]):
                assert (rows[:n - length + 1, l, WIDE_GROUPS[rec], WH.MM0] >= 1).all(), (i, length)
    if mode == "windows":
        WH.invariants(w["wtable"], w["depth"], w["q_offsets"], MODES[mode]["window_lengths"])
    if mode == "seed_copies":
        assert w["n_seeds"][2] == 300 - K + 1                                       # the spanning query keeps the windows it shares
    elif mode == "plain":
        assert w["n_seeds"][2] == K - 1                                             # ... and has only the windows across the crossing without
    if hook == "buffers":
        assert w["stats"]["chunks"] > 1, w["stats"]
    else:
        assert w["stats"]["chunks"] == 1
