"""CPU: the oracle against the compiled reference (oracle/_ref) on seeded fuzz.

Where oracle/_ref is built, the reference runs on the same inputs and the arrays are compared element for element; everywhere,
the oracle's outputs must carry the digests of the reference's outputs recorded in tests/golden/oracle_vs_ref.json
(SEQWIN_RECORD_REF_DIGESTS=1 rewrites that file from the reference, where it is built)."""
import gzip
import hashlib
import json
import os
import random

import numpy as np
import pytest

import oracle
from conftest import GOLDEN

ref = oracle.load_ref()
FIXTURE = GOLDEN / "oracle_vs_ref.json"
RECORD = os.environ.get("SEQWIN_RECORD_REF_DIGESTS") == "1"
DIGESTS = {} if RECORD else json.loads(FIXTURE.read_text())


def _digest(x):
    if isinstance(x, np.ndarray):
        return hashlib.sha256(str(x.dtype.descr).encode() + np.ascontiguousarray(x).tobytes()).hexdigest()
    return hashlib.sha256(repr(x).encode()).hexdigest()


def _ids(ids):
    return [[str(i) for i in t] for t in ids]


def _against_reference(key, got, exp):
    """`got` (the oracle's outputs) against the reference's: element for element where the reference is built (`exp`), and
    against the digests of the reference's outputs in the fixture always."""
    assert not RECORD or exp is not None, "SEQWIN_RECORD_REF_DIGESTS=1 needs oracle/_ref"
    if exp is not None:
        for x, y in zip(got, exp):
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and np.array_equal(x, y), key
            else:
                assert x == y, key
        if RECORD:
            DIGESTS[key] = [_digest(y) for y in exp]
    assert [_digest(x) for x in got] == DIGESTS[key], key


def _save_digests():
    if RECORD:
        cur = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else {}
        cur.update(DIGESTS)
        FIXTURE.write_text(json.dumps(cur, indent=0, sort_keys=True) + "\n")


def _randseq(rng, n):
    mode = rng.random()
    s = []
    for _ in range(n):
        r = rng.random()
        if r < 0.01:
            s.append(rng.choice("NnRYKMxX-*"))
        elif r < 0.03:
            s.append(rng.choice("acgtuU"))
        else:
            s.append(rng.choice("ACGT" if mode < 0.8 else "AC"))
    s = "".join(s)
    if rng.random() < 0.3:
        p = rng.randrange(0, max(1, n))
        s = s[:p] + "N" * rng.randrange(1, 60) + s[p:]
    return s


def test_fuzz_build_matches_reference(tmp_path):
    rng = random.Random(1)
    for it in range(60):
        ps = []
        for a in range(rng.randrange(1, 5)):
            txt = ""
            for r in range(rng.randrange(0, 4)):
                s = _randseq(rng, rng.choice([0, 5, 30, 100, 400, 1500]))
                txt += f">r{r} desc\n"
                width = rng.choice([60, 80, 7])
                for i in range(0, len(s), width):
                    txt += s[i:i + width] + rng.choice(["\n", "\r\n", " \n"])
                if rng.random() < 0.2:
                    txt += "\n  \n"
            gz = rng.random() < 0.3
            p = tmp_path / (f"{it}_{a}.fa" + (".gz" if gz else ""))
            if gz:
                with gzip.open(p, "wt") as f:
                    f.write(txt)
            else:
                p.write_text(txt)
            ps.append(str(p))
        k = rng.choice([3, 4, 5, 7, 15, 16, 17, 18, 19, 21, 31, 32, 33, 40])
        w = rng.choice([1, 2, 3, 5, 10, 25, 50, 200])
        n_cpu, low_memory = rng.choice([1, 2, 3]), rng.random() < 0.5
        a = oracle.build(ps, k, w)
        b = ref._build_native(ps, k, w, n_cpu, low_memory) if ref is not None else None
        _against_reference(f"fuzz/{it}/build", list(a[:4]) + [_ids(a[4])], b and list(b[:4]) + [_ids(b[4])])
        if len(a[1]) and len(ps) >= 2:
            tar = [i % 2 == 0 for i in range(len(ps))]
            n1 = a[1].copy()
            oracle.get_penalty(a[0], n1, a[3], tar)
            n2 = None
            if ref is not None:
                n2 = b[1].copy()
                ref._get_penalty_native(b[0], n2, b[3], np.asarray(tar, np.bool_), 2)
            _against_reference(f"fuzz/{it}/penalty", [n1], n2 is not None and [n2] or None)
            used = set(int(h) for h in n1["hash"][::3])
            f1 = oracle.filter_kmers(a[0], n1, used)
            f2 = ref._filter_kmers_native(b[0], n2, list(used)) if ref is not None else None
            _against_reference(f"fuzz/{it}/filter", list(f1[:2]), f2 and list(f2[:2]))
    _save_digests()


# The GPU parity tests lean on the oracle for k up to 300 and windows up to 10^6 (tests/test_gpu_parity.py); the fuzz
# above stops at k = 40, w = 200.  The same comparison on the wide range: every k the GPU tests use against the oracle
# (64, 100, 255, 256, 257, 300) plus 41 .. 1000, windows 1000, 4097, 20 000, 100 000, records with N runs, three assemblies.
WIDE_K = [41, 47, 63, 64, 65, 100, 128, 200, 255, 256, 257, 300, 511, 512, 1000]
WIDE_W = [1, 2, 31, 200, 1000, 4097, 20_000, 100_000]


@pytest.mark.parametrize("k", WIDE_K)
def test_wide_k_and_w_match_reference(tmp_path, k):
    rng = random.Random(1000 + k)
    ps = []
    for a in range(3):
        txt = ""
        for r in range(rng.randrange(1, 4)):
            n = rng.choice([k - 1, k, k + 1, 3000, 12_000, 45_000, 130_000])
            seq = "".join(rng.choice("ACGT") for _ in range(max(0, n)))
            if n > 2000 and rng.random() < 0.7:       # N runs, some of them closer than k to each other
                for _ in range(rng.randrange(1, 5)):
                    p = rng.randrange(0, n)
                    seq = seq[:p] + "N" * rng.choice([1, 2, k // 2 + 1, 500]) + seq[p:]
            if rng.random() < 0.3:
                seq = seq.lower().replace("t", "u")
            txt += f">a{a}r{r}\n{seq}\n"
        if a == 2:                                    # a contig shared with assembly 0: nodes and edges with weight 2
            txt += ps_first_contig
        p = tmp_path / f"w{k}_{a}.fa"
        p.write_text(txt)
        if a == 0:
            ps_first_contig = txt[:txt.index("\n", txt.index("\n") + 1) + 1]
        ps.append(str(p))
    tar = [True, False, True]
    for w in WIDE_W:
        a = oracle.build(ps, k, w)
        b = ref._build_native(ps, k, w, 2, False) if ref is not None else None
        _against_reference(f"wide/k{k}/w{w}/build", list(a[:4]), b and list(b[:4]))
        if len(a[1]):
            n1 = a[1].copy()
            oracle.get_penalty(a[0], n1, a[3], tar)
            n2 = None
            if ref is not None:
                n2 = b[1].copy()
                ref._get_penalty_native(b[0], n2, b[3], np.asarray(tar, np.bool_), 2)
            _against_reference(f"wide/k{k}/w{w}/penalty", [n1], n2 is not None and [n2] or None)
    _save_digests()
