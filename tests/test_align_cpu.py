"""CPU: the host restatement of the canonical alignment behind the infix edit distance (tests/tools/align_host.py, DESIGN.md section
3.2f) -- its two forms against each other and against answers written out by hand, the three identities, the replay of every
script, dist and end against tests/tools/hits_host.py, and the ties that the order of the four rules decides."""
import random
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "tools"))
import align_host as A  # noqa: E402
import hits_host as H  # noqa: E402


def _ops(res, x):
    o = res["offsets"].astype(np.int64)
    return "".join(A.OPS[c] for c in res["ops"][o[x]:o[x + 1]])


def _both(queries, records, pairs):
    a, b = A.alignments(queries, records, pairs), A.alignments_literal(queries, records, pairs)
    for f in A.FIELDS + ("offsets", "ops"):
        assert a[f].dtype == b[f].dtype and np.array_equal(a[f], b[f]), (f, a[f].tolist(), b[f].tolist())
    return a


def _properties(res, queries, records, pairs):
    """The three identities, the script's length, the replay, and Layer A's dist and end."""
    d, e = H.infix(queries, records, pairs)
    assert np.array_equal(res["dist"], d) and np.array_equal(res["end"], e)
    o = res["offsets"].astype(np.int64)
    for x, (q, strand, rec, start, stop) in enumerate(np.asarray(pairs).tolist()):
        ops = res["ops"][o[x]:o[x + 1]]
        n_i, n_d = int((ops == 2).sum()), int((ops == 3).sum())
        m = len(H._bytes(queries[q]))
        ni, nx, ng = int(res["nident"][x]), int(res["mismatch"][x]), int(res["gaps"][x])
        assert ni == (ops == 0).sum() and nx == (ops == 1).sum() and ng == n_i + n_d
        assert ni + nx + n_i == m
        assert ni + nx + n_d == int(res["end"][x]) - int(res["start"][x])
        assert nx + ng == int(res["dist"][x])
        assert len(ops) == m + n_d
        assert start <= res["start"][x] <= res["end"][x] <= stop
        pat = H._text(queries[q])
        pat = H._rc(pat) if strand else pat
        seg = H._text(records[rec])[int(res["start"][x]):int(res["end"][x])]
        assert A.replay_matches(pat, ops, seg), (x, _ops(res, x), pat, seg)
        assert len(A.replay(pat, ops)) == len(seg)


# (pattern, text, dist, start, end, ops) -- every answer worked out by hand from the rules
HAND = [
    ("ACGT", "TTACGTTT", 0, 2, 6, "===="),
    ("CAAAAG", "TCAAAGT", 1, 1, 6, "=I===="),        # a run shorter in the text: rule 3 fires at the run's first base, not before
    ("GCAAAGC", "GCAAAAGC", 1, 0, 8, "==D====="),    # a run longer in the text: the text's first A faces the gap (rules 2 and 3 fail there)
    ("CAAAG", "TCAAAAGT", 1, 1, 5, "====I"),         # ... but the smallest column of the minimum is 5 (CAAA, G unplaced), not 7 (X====)
    ("TTACGT", "ACGTCC", 2, 0, 4, "II===="),         # the prefix is missing at the window start: j == 0 with i > 0
    ("ACGTACGT", "GTAC", 4, 0, 4, "II====II"),       # a pattern longer than the text
    ("ACGTA", "GGACNTAGG", 1, 2, 7, "==X=="),        # an N in the text opposite a valid base
    ("ACNTA", "GGACGTAGG", 1, 2, 7, "==X=="),        # an N in the query
    ("ACNTA", "GGACNTAGG", 1, 2, 7, "==X=="),        # an N in both: it equals nothing
    ("", "ACGT", 0, 0, 0, ""),                       # an empty query
    ("ACG", "", 3, 0, 0, "III"),                     # an empty text
    ("AAAA", "CCCC", 4, 0, 0, "IIII"),               # nothing matches: column 0 already attains the minimum
]


@pytest.mark.parametrize("case", HAND, ids=[f"{p or 'empty'}-{t or 'empty'}" for p, t, *_ in HAND])
def test_hand_made_cases(case):
    pat, text, dist, start, end, ops = case
    res = _both([pat], [text], [(0, 0, 0, 0, len(text))])
    got = (int(res["dist"][0]), int(res["start"][0]), int(res["end"][0]), _ops(res, 0))
    assert got == (dist, start, end, ops)
    assert (int(res["nident"][0]), int(res["mismatch"][0]), int(res["gaps"][0])) == (ops.count("="), ops.count("X"), ops.count("I") + ops.count("D"))
    _properties(res, [pat], [text], [(0, 0, 0, 0, len(text))])
    # the same alignment inside a longer record, and on the other strand of the reverse-complemented query
    rec = "GATTACA" + text + "TGCA"
    res = _both([pat, H.revcomp(pat).decode()], [rec], [(0, 0, 0, 7, 7 + len(text)), (1, 1, 0, 7, 7 + len(text))])
    for x in (0, 1):
        assert (int(res["dist"][x]), int(res["start"][x]), int(res["end"][x]), _ops(res, x)) == (dist, 7 + start, 7 + end, ops)


def test_the_two_forms_agree_on_random_pairs():
    rng = random.Random(20)
    queries, records, pairs = [], [], []
    for case in range(300):
        anc = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 60)))
        q = list(anc[rng.randint(0, len(anc) // 2):])
        for _ in range(rng.randint(0, 4)):                  # a few edits of every kind, an invalid byte, lower case and U
            if not q:
                break
            at = rng.randrange(len(q))
            kind = rng.randrange(5)
            if kind == 0:
                q[at] = rng.choice("ACGT")
            elif kind == 1:
                q.insert(at, rng.choice("ACGT"))
            elif kind == 2:
                del q[at]
            elif kind == 3:
                q[at] = rng.choice("NnRX")
            else:
                q[at] = q[at].lower().replace("t", "u")
        rec = list("".join(rng.choice("ACGT") for _ in range(rng.randint(0, 8))) + anc + "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 8))))
        if rec and rng.random() < 0.3:
            rec[rng.randrange(len(rec))] = "N"
        strand = rng.randrange(2)
        q = "".join(q)
        queries.append(H.revcomp(q).decode() if strand else q)
        records.append("".join(rec))
        start = rng.randint(0, len(rec) // 4)
        pairs.append((case, strand, case, start, rng.randint(start, len(rec))))
    res = _both(queries, records, pairs)
    _properties(res, queries, records, pairs)
    assert (res["gaps"] > 0).sum() > 30 and (res["mismatch"] > 0).sum() > 30 and (res["start"] > 0).sum() > 30


def test_homopolymers_and_low_complexity_text():
    """Many optimal paths: runs of one base and short periods, where only the rule order fixes the script."""
    rng = random.Random(4)
    queries, records, pairs = [], [], []
    for case in range(80):
        unit = rng.choice(["A", "AC", "AAC", "ACG"])
        q = unit * rng.randint(1, 12) + rng.choice(["", "G", "TT"])
        r = rng.choice(["", "T", "GG"]) + unit * rng.randint(0, 14) + rng.choice(["", "C", "TG"])
        queries.append(q)
        records.append(r)
        pairs.append((case, rng.randrange(2), case, 0, len(r)))
    res = _both(queries, records, pairs)
    _properties(res, queries, records, pairs)


def test_replay():
    assert A.replay("ACGT", "==X=") == "AC?T" and A.replay("ACGT", "=I=D=") == "AG*T" and A.replay("", "") == ""
    assert A.replay_matches("ACGT", "==X=", "ACTT") and not A.replay_matches("ACGT", "==X=", "ACGT") and not A.replay_matches("ACGT", "====", "ACG")
    assert not A.replay_matches("AC#T", "====", "AC#T") and A.replay_matches("AC#T", "==X=", "AC#T")
    for bad in ("===", "=====", "==I"):
        with pytest.raises(ValueError):
            A.replay("ACGT", bad)


def test_cigar():
    from seqwin_amd.markers import cigar
    res = A.alignments(["CAAAAG", "", "ACGT"], ["TCAAAGT"], [(0, 0, 0, 0, 7), (1, 0, 0, 0, 7), (2, 0, 0, 0, 0)])
    assert cigar(res["offsets"], res["ops"]) == ["1=1I4=", "", "4I"]
    assert cigar([0], []) == []
    with pytest.raises(ValueError):
        cigar([0, 3], [0, 1])
