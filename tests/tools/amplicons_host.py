"""Host restatement of the amplicon stage (csrc/amplicons.hip, seqwin_amd/device.py: OligoHits.amplicons), twice.

A site is (oligo, assembly, record, pos, end, strand, d[, dg]) -- the columns of ``OligoHits.sites()``: ``end`` and ``dist`` are there
for either kind of result.  For pair i = (f, r): orientation + (0) joins a site of f on strand 0 at pf with a site of r on strand 1 of
the same record with pos_r >= pf, product [pf, end_r); orientation - (1) the same with f and r exchanged; with f == r only +.  Kept iff
min_len <= end - start <= max_len.  With max_dg a PRIMER site takes part only if dg <= max_dg.  n_probe of a product: the sites of
the pair's probe in that record, either strand, with end_first <= pos_p and end_p <= pos_last.  The list is ascending by its first
eight columns; rows equal in all eight keep the order (first site, last site) of the site list.

    amplicons_loop    all pairs of sites by nested loops, as oligo_host.amplicons does it, and a loop over all sites for the probe
    amplicons_merge   per record the two sides sorted by pos, a moving lower pointer, bisection for the probe
"""
import bisect

import numpy as np

NO_PROBE = 0xFFFFFFFF
FIELDS = ("pair", "assembly", "record", "start", "end", "orientation", "mm_f", "mm_r", "n_probe")


def _rows(sites):
    cols = [np.asarray(sites[f]).tolist() for f in ("oligo", "assembly", "record", "pos", "end", "strand", "dist")]
    dg = np.asarray(sites["dg"]).tolist() if "dg" in sites else [None] * len(cols[0])
    return list(zip(*cols, dg))


def _probe_of(probes, pi):
    if probes is None or probes[pi] is None or int(probes[pi]) == NO_PROBE:
        return None
    return int(probes[pi])


def _finish(out, n_pairs, n_assemblies):
    out = sorted(out, key=lambda row: row[:8])   # (stable: equal rows keep the order they were formed in)
    n_amp = np.zeros((n_pairs, n_assemblies), np.uint32)
    n_det = np.zeros((n_pairs, n_assemblies), np.uint32)
    for row in out:
        n_amp[row[0], row[1]] += 1
        n_det[row[0], row[1]] += row[8] >= 1
    cols = np.array(out, np.int64).reshape(-1, len(FIELDS))
    res = {f: cols[:, i].astype(np.uint32) for i, f in enumerate(FIELDS)}
    res["cell_offsets"] = np.concatenate([[0], np.cumsum(n_amp.reshape(-1), dtype=np.uint64)]).astype(np.uint64)
    res["n_amplicons"], res["n_detected"] = n_amp, n_det
    return res


def amplicons_loop(sites, pairs, min_len, max_len, n_assemblies, probes=None, max_dg=None):
    S = _rows(sites)
    out = []
    for pi, (f, r) in enumerate(pairs):
        p = _probe_of(probes, pi)
        for orientation, (first, last) in enumerate(((f, r), (r, f))):
            if orientation == 1 and f == r:
                continue
            for (q1, a1, r1, p1, e1, s1, d1, g1) in S:
                if q1 != first or s1 != 0 or (max_dg is not None and g1 > max_dg):
                    continue
                for (q2, a2, r2, p2, e2, s2, d2, g2) in S:
                    if q2 != last or s2 != 1 or r2 != r1 or p2 < p1 or (max_dg is not None and g2 > max_dg):
                        continue
                    if not min_len <= e2 - p1 <= max_len:
                        continue
                    n_probe = 0
                    if p is not None:
                        n_probe = sum(1 for (q3, a3, r3, p3, e3, s3, d3, g3) in S if q3 == p and r3 == r1 and e1 <= p3 and e3 <= p2)
                    mf, mr = (d1, d2) if orientation == 0 else (d2, d1)
                    out.append((pi, a1, r1, p1, e2, orientation, mf, mr, n_probe))
    return _finish(out, len(pairs), n_assemblies)


def amplicons_merge(sites, pairs, min_len, max_len, n_assemblies, probes=None, max_dg=None):
    S = _rows(sites)
    by = {}    # (oligo, record) -> list indices, ascending (the list's order within an oligo and record: pos, then end, then strand)
    for i, row in enumerate(S):
        by.setdefault((row[0], row[2]), []).append(i)
    records = sorted({row[2] for row in S})
    ok = [max_dg is None or row[7] <= max_dg for row in S]
    out = []
    for pi, (f, r) in enumerate(pairs):
        p = _probe_of(probes, pi)
        for orientation, (first, last) in enumerate(((f, r), (r, f))):
            if orientation == 1 and f == r:
                continue
            for rec in records:
                F = [i for i in by.get((first, rec), []) if S[i][5] == 0 and ok[i]]
                R = [i for i in by.get((last, rec), []) if S[i][5] == 1 and ok[i]]
                if not F or not R:
                    continue
                P = by.get((p, rec), []) if p is not None else []
                probe_pos = [S[i][3] for i in P]             # (ascending)
                lo = 0
                for i in F:                                  # (pos ascending)
                    pf, ef = S[i][3], S[i][4]
                    while lo < len(R) and S[R[lo]][3] < pf:
                        lo += 1
                    k = lo
                    while k < len(R) and S[R[k]][3] < pf + max_len:   # (a site is a base or more: end > pos)
                        j = R[k]
                        k += 1
                        if not min_len <= S[j][4] - pf <= max_len:
                            continue
                        x0, x1 = bisect.bisect_left(probe_pos, ef), bisect.bisect_right(probe_pos, S[j][3])
                        n_probe = sum(1 for x in P[x0:x1] if S[x][4] <= S[j][3])
                        mf, mr = (S[i][6], S[j][6]) if orientation == 0 else (S[j][6], S[i][6])
                        out.append((pi, S[i][1], rec, pf, S[j][4], orientation, mf, mr, n_probe))
    return _finish(out, len(pairs), n_assemblies)
