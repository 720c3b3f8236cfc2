"""Sequences and row edit distances through Markers (Markers.sequences, Markers.row_distances, markers.row_summary) and the
drop-in's last step (markers.get_cks with a batch, markers.save_markers), on the resident route over the marker goldens: the
representatives against the strings recorded from the reference's Assemblies.fetch_seq (tests/golden/markers/*_seqs.npz), every
row and every distance against the host restatement (tests/tools/seqs_host.py)."""
import functools
import json
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import seqs_host as H  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
GRAPHS = ("pan_a_k15_w20", "pan_b_k21_w10", "smoke_k17_w10")
CASES = [c for c in json.loads((GOLDEN / "markers" / "manifest.json").read_text())["cases"] if c["graph"] in GRAPHS and c["error"] is None]
SUB = {g["name"]: g for g in json.loads((GOLDEN / "subgraphs" / "manifest.json").read_text())["graphs"]}
IDS = [f"{c['graph']}_c{c['case']}" for c in CASES]
distance = functools.lru_cache(maxsize=None)(H.distance)


def _resident(c, paths=None):
    from seqwin_amd.device import Batch
    g = SUB[c["graph"]]
    case = g["cases"][c["case"]]
    b = Batch.from_fasta(paths or [GOLDEN / p for p in g["paths"]])
    ix = b.build_index(g["k"], g["w"], g["is_targets"])
    f = ix.filter_graph(g["edge_weight_th"])
    sg = f.subgraphs(case["penalty_th"], case["min_nodes"], case["max_nodes"], random.Random(case["seed"]))
    return g, b, sg, ix.filter_kmers(f, sg)


def _strings(offs, blob):
    o = offs.astype(np.int64)
    return [blob[o[i]:o[i + 1]].decode("ascii") for i in range(len(o) - 1)]


def _golden_rep_strings(c):
    z = np.load(GOLDEN / "markers" / f"{c['graph']}_c{c['case']}_seqs.npz")
    return _strings(z["rep_seq_offsets"], z["rep_seq_blob"].tobytes())


def _texts(g):
    """The records' texts by assembly, the restatement's way."""
    return [H.read_records(GOLDEN / p) for p in g["paths"]]


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_sequences_distances_and_summary(ci):
    from seqwin_amd import markers
    c = CASES[ci]
    g, b, sg, kept = _resident(c)
    m = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"], keep_rows=True)
    texts = _texts(g)
    # the representatives: the reference's strings
    offs, blob, inexact = m.sequences(b, "reps")
    rep_seqs = _strings(offs, blob)
    assert rep_seqs == _golden_rep_strings(c) and not inexact.any()
    reps = m.reps()[0]
    # every row: the restatement
    per = m.rows()
    rows = np.concatenate([r for r, _, _ in per])
    offs, blob, inexact = m.sequences(b, "rows")
    row_seqs = _strings(offs, blob)
    want = [H.fetch(texts[r["assembly_idx"]][r["record_idx"]], int(r["start"]), int(r["stop"])) for r in rows]
    assert row_seqs == [w for w, _ in want] and inexact.tolist() == [bad for _, bad in want]
    # a selection, in the order asked for
    pick = [len(per) - 1, 0]
    so, sb, _ = m.sequences(b, "reps", select=pick)
    assert _strings(so, sb) == [rep_seqs[i] for i in pick]
    ro, rb, _ = m.sequences(b, "rows", select=pick)
    bounds = np.concatenate([[0], np.cumsum([len(r) for r, _, _ in per])])
    assert _strings(ro, rb) == [s for i in pick for s in row_seqs[bounds[i]:bounds[i + 1]]]
    # distances: the host programme on the fetched strings
    dist, strand, st = m.row_distances(b, stats=True)
    sg_of_row = np.repeat(np.arange(len(per)), [len(r) for r, _, _ in per])
    host = [distance(rep_seqs[s], row_seqs[j]) for j, s in enumerate(sg_of_row)]
    assert np.array_equal(dist, np.array([d for d, _ in host], np.uint32)) and np.array_equal(strand, np.array([t for _, t in host], np.uint8))
    assert st["pairs"] == len(rows) == c["n_rows"] and st["striped_pairs"] == 0
    for i, (r, _, _) in enumerate(per):        # each representative's own row is (0, 0)
        own = np.flatnonzero((r["assembly_idx"] == reps["assembly_idx"][i]) & (r["start"] == reps["start"][i]) & (r["record_idx"] == reps["record_idx"][i]))
        assert len(own) == 1
        j = bounds[i] + own[0]
        assert (dist[j], strand[j]) == (0, 0)
    d2, s2 = m.row_distances(b, select=pick)
    assert d2.tolist() == [x for i in pick for x in dist[bounds[i]:bounds[i + 1]].tolist()]
    # the summary: a straightforward loop
    n_tar, n_neg = c["n_tar"], len(g["paths"]) - c["n_tar"]
    got = markers.row_summary(m, dist, n_tar, n_neg)
    for i, (r, _, _) in enumerate(per):
        length = int(reps["stop"][i]) - int(reps["start"][i])
        idt = dng = 0.0
        nt = nn = 0
        for j, row in enumerate(r):
            d = int(dist[bounds[i] + j])
            if row["assembly_idx"] < n_tar:
                idt += max(0.0, 1.0 - d / length)
                nt += 1
            else:
                dng += min(1.0, d / length)
                nn += 1
        assert got["identity_tar"][i] == pytest.approx(idt / n_tar, rel=1e-12, abs=1e-15) and got["f_tar_rows"][i] == nt / n_tar
        if n_neg:
            assert got["distance_neg"][i] == pytest.approx(dng / n_neg, rel=1e-12, abs=1e-15) and got["f_neg_rows"][i] == nn / n_neg
    m.close()


def test_rows_need_keep_rows_and_the_batch_must_cover_the_records(tmp_path):
    from seqwin_amd.device import Batch
    c = CASES[0]
    g, b, sg, kept = _resident(c)
    m = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"])
    assert len(m.sequences(b, "reps")[0]) == c["n_subgraphs"] + 1
    with pytest.raises(ValueError, match="keep_rows"):
        m.sequences(b, "rows")
    with pytest.raises(ValueError, match="keep_rows"):
        m.row_distances(b)
    with pytest.raises(ValueError, match="which"):
        m.sequences(b, "loc")
    m2 = kept.marker_locs(sg, b.record_offsets(), c["n_tar"], g["k"], g["w"], keep_rows=True)
    fewer = Batch.from_fasta([GOLDEN / p for p in g["paths"][:-1]])
    for call in (lambda: m2.sequences(fewer, "reps"), lambda: m2.sequences(fewer, "rows"), lambda: m2.row_distances(fewer)):
        with pytest.raises(ValueError, match="does not cover"):
            call()
    # as many assemblies, but the first holds one record more than the markers' table says
    first = H.read_records(GOLDEN / g["paths"][0])
    longer = tmp_path / "one_more.fa"
    longer.write_text("".join(f">r{j}\n{t}\n" for j, t in enumerate(first + ["ACGTACGT"])))
    other = Batch.from_fasta([longer] + [GOLDEN / p for p in g["paths"][1:]])
    assert len(other.record_offsets()) == len(b.record_offsets()) and other.record_offsets()[1] == b.record_offsets()[1] + 1
    for call in (lambda: m2.sequences(other, "reps"), lambda: m2.row_distances(other)):
        with pytest.raises(ValueError, match="does not cover"):
            call()


def _golden_candidates(c, z, min_len):
    reps = z["reps"]
    length = (reps["stop"] - reps["start"]).astype(np.uint32)
    return reps, length, np.flatnonzero((length >= min_len) & ((reps["flags"] & 3) == 0))


def test_get_cks_with_a_batch_and_save_markers(tmp_path):
    from seqwin_amd import markers
    c = next(x for x in CASES if x["graph"] == "pan_a_k15_w20")
    g, b, sg, kept = _resident(c)
    z = np.load(GOLDEN / "markers" / f"{c['graph']}_c{c['case']}.npz")
    reps, length, keep = _golden_candidates(c, z, 0)
    min_len = int(np.median(length))
    reps, length, keep = _golden_candidates(c, z, min_len)
    cks = markers.get_cks(kept, sg, b.record_offsets(), c["n_tar"], g["k"], g["w"], min_len, batch=b)
    ref_seqs = _golden_rep_strings(c)
    assert 0 < len(cks) == len(keep)
    assert [ck.rep["seq"] for ck in cks] == [ref_seqs[i] for i in keep] and all(type(ck.rep["seq"]) is str for ck in cks)
    record_ids = b.records()[1]
    fasta_path, csv_path = markers.save_markers(cks, record_ids, tmp_path, overwrite=False)
    assert (fasta_path.name, csv_path.name) == ("signatures.fasta", "signatures.csv")
    want_fasta, want_csv = H.save_block([(int(reps["assembly_idx"][i]), int(reps["record_idx"][i]), int(reps["start"][i]), int(reps["stop"][i]), ref_seqs[i],
                                          int(length[i]), int(reps["n_rep"][i]) / c["n_tar"], int(reps["n_kmers"][i])) for i in keep], record_ids)
    assert fasta_path.read_bytes() == want_fasta.encode() and csv_path.read_bytes() == want_csv.encode()
    with pytest.raises(FileExistsError):
        markers.save_markers(cks, record_ids, tmp_path, overwrite=False)
    markers.save_markers(cks, record_ids, tmp_path, overwrite=True)
    assert fasta_path.read_bytes() == want_fasta.encode()


def test_get_cks_reads_a_flagged_representative_from_its_file(tmp_path):
    """Input files that carry the IUPAC letter R in the middle of every representative of the golden run: a candidate whose
    interval holds one is flagged by the fetch, read from its file with `paths` -- the original letter is there -- and refused
    without."""
    import gzip
    from seqwin_amd import markers
    c = next(x for x in CASES if x["graph"] == "pan_a_k15_w20")
    g = SUB[c["graph"]]
    reps = np.load(GOLDEN / "markers" / f"{c['graph']}_c{c['case']}.npz")["reps"]
    texts = _texts(g)
    for r in reps:
        if int(r["stop"]) - int(r["start"]) >= 100:
            t = texts[r["assembly_idx"]][r["record_idx"]]
            mid = (int(r["start"]) + int(r["stop"])) // 2
            texts[r["assembly_idx"]][r["record_idx"]] = t[:mid] + "R" + t[mid + 1:]
    paths = []
    for a, recs in enumerate(texts):
        p = tmp_path / (f"g{a}.fa.gz" if a % 2 else f"g{a}.fa")
        body = "".join(f">r{a}_{j} x\n" + "\n".join(t[i:i + 80] for i in range(0, len(t), 80)) + "\n" for j, t in enumerate(recs)).encode()
        p.write_bytes(gzip.compress(body) if a % 2 else body)
        paths.append(p)
    _, b, sg, kept = _resident(c, paths)
    args = (kept, sg, b.record_offsets(), c["n_tar"], g["k"], g["w"], 30)
    cks = markers.get_cks(*args, batch=b, paths=paths)
    flagged = [ck for ck in cks if "R" in ck.rep["seq"]]
    assert flagged, "no candidate spans an inserted letter: the premise of this test is gone"
    for ck in cks:
        rep = ck.rep
        assert rep["seq"] == texts[rep["assembly_idx"]][rep["record_idx"]][int(rep["start"]):int(rep["stop"])]
    with pytest.raises(ValueError, match="candidate " + str(flagged[0].rep["assembly_idx"]) + "-"):
        markers.get_cks(*args, batch=b)
    assert all(ck.rep["seq"] is None for ck in markers.get_cks(*args))
