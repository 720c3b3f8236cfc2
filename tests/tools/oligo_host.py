"""Host restatement of the oligo search (csrc/oligo.hip, seqwin_amd/oligos.py), twice, and of `amplicons`.

An assembly is a list of records (bytes).  A base is valid iff it is one of ACGTU in either case (U = T); a site is a window
[p, p + L) of valid bases only; P0 is the oligo as a list of sets, P1 its reverse complement (sets complemented, order reversed);
mm = #{i : text[p + i] not in Ps[i]}; a hit has mm <= max_mismatch and no mismatch among the `three_prime` positions at the oligo's
3' end (strand 0: L - c .. L - 1, strand 1: 0 .. c - 1).

    sites_loop    a per-position Python loop over sets
    sites_planes  NumPy over one-hot planes of the text
    search        either of them as the arrays Batch.oligo_hits returns
    amplicons     all pairs of sites, by two nested loops
"""
import numpy as np

NO_HIT = 0xFFFFFFFF
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT",
         "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


def _text(x):
    return x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x


def strands(oligo):
    """[P0, P1]: lists of sets of 'ACGT'"""
    p0 = [set(IUPAC[c]) for c in _text(oligo).upper()]
    p1 = [{COMP[b] for b in s} for s in reversed(p0)]
    return [p0, p1]


def revcomp(seq: bytes) -> bytes:
    return bytes(seq).translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]


def _clamped(L, strand, c):
    return range(L - c, L) if strand == 0 else range(0, c)


def sites_loop(oligos, assemblies, max_mm, three_prime=0):
    """sorted list of (oligo, assembly, record, pos, strand, mm); record is global"""
    out = []
    rec0 = 0
    for a, recs in enumerate(assemblies):
        for ri, rec in enumerate(recs):
            t = _text(rec).upper().replace("U", "T")
            for q, o in enumerate(oligos):
                L = len(o)
                for s, P in enumerate(strands(o)):
                    for p in range(len(t) - L + 1):
                        w = t[p:p + L]
                        if any(ch not in "ACGT" for ch in w):
                            continue
                        miss = [i for i in range(L) if w[i] not in P[i]]
                        if len(miss) <= max_mm and not any(i in _clamped(L, s, three_prime) for i in miss):
                            out.append((q, a, rec0 + ri, p, s, len(miss)))
        rec0 += len(recs)
    return sorted(out)


def _planes(rec):
    """(onehot[4, n] bool, valid[n] bool)"""
    b = np.frombuffer(bytes(rec).upper().replace(b"U", b"T"), np.uint8)
    onehot = np.stack([b == ord(c) for c in "ACGT"])
    return onehot, onehot.any(0)


def sites_planes(oligos, assemblies, max_mm, three_prime=0):
    out = []
    rec0 = 0
    pats = []
    for o in oligos:
        pats.append([np.array([[b not in s for s in P] for b in "ACGT"], bool) for P in strands(o)])   # miss[b, i]
    for a, recs in enumerate(assemblies):
        for ri, rec in enumerate(recs):
            onehot, valid = _planes(rec)
            n = len(valid)
            bad = np.concatenate([[0], np.cumsum(~valid)])
            for q, o in enumerate(oligos):
                L = len(o)
                nw = n - L + 1
                if nw <= 0:
                    continue
                ok = bad[L:] - bad[:nw] == 0
                for s in (0, 1):
                    miss = pats[q][s]
                    per_pos = np.zeros((L, nw), bool)
                    for i in range(L):
                        for b in range(4):
                            if miss[b, i]:
                                per_pos[i] |= onehot[b, i:i + nw]
                    mm = per_pos.sum(0)
                    cl = list(_clamped(L, s, three_prime))
                    hit = ok & (mm <= max_mm) & (per_pos[cl].sum(0) == 0 if cl else True)
                    for p in np.nonzero(hit)[0]:
                        out.append((q, a, rec0 + ri, int(p), s, int(mm[p])))
        rec0 += len(recs)
    return sorted(out)


def search(oligos, assemblies, max_mm, three_prime=0, form=sites_planes):
    """dict: n_sites, best_mm, best_record, best_pos, best_strand [nq, na] uint32 and sites (the six columns + cell_offsets)"""
    S = form(oligos, assemblies, max_mm, three_prime)
    nq, na = len(oligos), len(assemblies)
    n_sites = np.zeros((nq, na), np.uint32)
    best = {f: np.full((nq, na), NO_HIT, np.uint32) for f in ("best_mm", "best_record", "best_pos", "best_strand")}
    best_key = {}
    for q, a, r, p, s, mm in S:
        n_sites[q, a] += 1
        if (q, a) not in best_key or (mm, r, p, s) < best_key[q, a]:
            best_key[q, a] = (mm, r, p, s)
    for (q, a), (mm, r, p, s) in best_key.items():
        best["best_mm"][q, a], best["best_record"][q, a], best["best_pos"][q, a], best["best_strand"][q, a] = mm, r, p, s
    cols = np.array(S, np.uint32).reshape(-1, 6)
    sites = {f: cols[:, i].copy() for i, f in enumerate(("oligo", "assembly", "record", "pos", "strand", "mm"))}
    sites["cell_offsets"] = np.concatenate([[0], np.cumsum(n_sites.reshape(-1), dtype=np.uint64)]).astype(np.uint64)
    return dict(n_sites=n_sites, sites=sites, **best)


def amplicons(sites, lengths, pairs, min_len, max_len, n_assemblies):
    """(sorted list of (pair, assembly, record, start, end, orientation, mm_f, mm_r), n_amplicons[n_pairs, n_assemblies])"""
    S = list(zip(*(np.asarray(sites[f]).tolist() for f in ("oligo", "assembly", "record", "pos", "strand", "mm"))))
    out = []
    for pi, (f, r) in enumerate(pairs):
        for (q1, a1, r1, p1, s1, m1) in S:
            for (q2, a2, r2, p2, s2, m2) in S:
                if r1 != r2 or s1 != 0 or s2 != 1 or p1 > p2:
                    continue
                if q1 == f and q2 == r:      # orientation +: f on strand 0, r on strand 1
                    start, end, row = p1, p2 + lengths[r], (0, m1, m2)
                    if min_len <= end - start <= max_len:
                        out.append((pi, a1, r1, start, end) + row)
                if q1 == r and q2 == f and f != r:   # orientation -: r on strand 0, f on strand 1
                    start, end, row = p1, p2 + lengths[f], (1, m2, m1)
                    if min_len <= end - start <= max_len:
                        out.append((pi, a1, r1, start, end) + row)
    out.sort()
    n = np.zeros((len(pairs), n_assemblies), np.uint32)
    for row in out:
        n[row[0], row[1]] += 1
    return out, n
