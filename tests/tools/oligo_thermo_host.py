"""Host restatement of the nearest-neighbour sums of the oligo search (csrc/oligo_thermo_core.hpp,
seqwin_amd/oligos.py), twice, on top of the Hamming sites of tests/tools/oligo_host.py.

A model is (stack int16[3, 4, 4, 4, 4], end int16[3, 2, 4, 4], init int32[3]); planes dh, ds, dg; base codes A=0 C=1 G=2 T=3.
For a hit with oligo letters O_1..O_L (sets) and window text t_0..t_{L-1}:
    strand 0   y_i = 3 - t_{i-1}       (the oligo has the text's sense and binds its complement)
    strand 1   y_i = t_{L-i}           (the oligo binds the text strand itself, read backwards)
    x_i = 3 - y_i where O_i holds it, else the least member of O_i (A < C < G < T)
    sums = init + end[0][x_1][y_1] + end[1][x_L][y_L] + sum over i = 1..L-1 of stack[x_i][x_i+1][y_i][y_i+1]

    site_sums_loop   one site, a per-position Python loop over sets
    sums_gather      the whole site list, NumPy gathers
    search           the arrays Batch.oligo_hits(..., thermo=, max_dg=) returns, on top of oligo_host.search
"""
import numpy as np

import oligo_host as H

NO_HIT = 0xFFFFFFFF
NO_SUM = -2 ** 31
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}
STABLE_FIELDS = ("stable_dg", "stable_dh", "stable_ds", "stable_record", "stable_pos", "stable_strand", "stable_mm")


def _text(x):
    return x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else x


def random_model(rng, dg_max=15000):
    """asymmetric random tables: every index order and strand mistake changes a sum"""
    stack = rng.integers(-30000, 30001, (3, 4, 4, 4, 4)).astype(np.int16)
    end = rng.integers(-30000, 30001, (3, 2, 4, 4)).astype(np.int16)
    init = rng.integers(-10 ** 6, 10 ** 6, 3).astype(np.int32)
    stack[2] = rng.integers(-dg_max, dg_max + 1, (4, 4, 4, 4))
    end[2] = rng.integers(-dg_max, dg_max + 1, (2, 4, 4))
    init[2] = rng.integers(-dg_max, dg_max + 1)
    return stack, end, init


def site_sums_loop(oligo, window, strand, model):
    """(dh, ds, dg) of one site: `window` is the L bases of the text at the site (ACGTU in either case)"""
    stack, end, init = model
    sets = [{CODE[b] for b in H.IUPAC[c]} for c in _text(oligo).upper()]
    t = [CODE[c] for c in _text(window).upper()]
    L = len(sets)
    assert len(t) == L
    xs, ys = [], []
    for i in range(1, L + 1):
        y = 3 - t[i - 1] if strand == 0 else t[L - i]
        ys.append(y)
        xs.append(3 - y if (3 - y) in sets[i - 1] else min(sets[i - 1]))
    out = []
    for p in range(3):
        v = int(init[p]) + int(end[p][0][xs[0]][ys[0]]) + int(end[p][1][xs[-1]][ys[-1]])
        for i in range(L - 1):
            v += int(stack[p][xs[i]][xs[i + 1]][ys[i]][ys[i + 1]])
        out.append(v)
    return tuple(out)


def _codes(rec):
    """int8[n]: the base codes of a record, -1 for an invalid base"""
    lut = np.full(256, -1, np.int8)
    for c, v in CODE.items():
        lut[ord(c)] = lut[ord(c.lower())] = v
    return lut[np.frombuffer(bytes(rec), np.uint8)]


def sums_gather(oligos, assemblies, sites, model):
    """int32 dh, ds, dg of every entry of a site list (the columns oligo, record, pos, strand), by gathers: per oligo length one
    [n, L] matrix of text codes, y and x from it, the tables indexed by whole columns"""
    stack, end, init = (np.asarray(a).astype(np.int64) for a in model)
    recs = [_codes(r) for recs in assemblies for r in recs]
    oligo, record, pos, strand = (np.asarray(sites[f]).astype(np.int64) for f in ("oligo", "record", "pos", "strand"))
    n = len(oligo)
    out = np.zeros((3, n), np.int64)
    member = []                                  # member[q][i, b]: base b lies in the set of position i
    for o in oligos:
        member.append(np.array([[b in H.IUPAC[c] for b in "ACGT"] for c in _text(o).upper()], bool))
    for L in sorted({len(o) for o in oligos}):
        idx = np.nonzero(np.array([len(oligos[q]) for q in oligo], np.int64) == L)[0] if n else np.zeros(0, np.int64)
        if not len(idx):
            continue
        T = np.stack([recs[record[j]][pos[j]:pos[j] + L] for j in idx]).astype(np.int64)          # [m, L]
        assert T.shape == (len(idx), L) and (T >= 0).all()
        s = strand[idx][:, None]
        Y = np.where(s == 0, 3 - T, T[:, ::-1])                                                    # y_i, i = 1..L along axis 1
        M = np.stack([member[q] for q in oligo[idx]])                                              # [m, L, 4]
        holds = np.take_along_axis(M, (3 - Y)[:, :, None], 2)[:, :, 0]
        least = M.argmax(2)                                                                        # the first True: the least member
        X = np.where(holds, 3 - Y, least)
        for p in range(3):
            v = init[p] + end[p][0][X[:, 0], Y[:, 0]] + end[p][1][X[:, -1], Y[:, -1]]
            v = v + stack[p][X[:, :-1], X[:, 1:], Y[:, :-1], Y[:, 1:]].sum(1)
            out[p, idx] = v
    assert (np.abs(out) < 2 ** 31).all()
    return out[0].astype(np.int32), out[1].astype(np.int32), out[2].astype(np.int32)


def sums_loop(oligos, assemblies, sites, model):
    """the same by site_sums_loop, site by site"""
    recs = [bytes(r) for recs in assemblies for r in recs]
    rows = []
    for q, r, p, s in zip(*(np.asarray(sites[f]).tolist() for f in ("oligo", "record", "pos", "strand"))):
        rows.append(site_sums_loop(oligos[q], recs[r][p:p + len(oligos[q])], s, model))
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32)


def search(oligos, assemblies, max_mm, three_prime, model, max_dg=None, plain=None, form=sums_gather):
    """oligo_host.search's dict (or `plain`, one made before) with dh, ds, dg in its sites, n_stable [nq, na] uint32 and the seven
    stable fields: the hit least in (dg, record, pos, strand) among ALL hits of the cell"""
    want = dict(plain if plain is not None else H.search(oligos, assemblies, max_mm, three_prime))
    S = dict(want["sites"])
    S["dh"], S["ds"], S["dg"] = form(oligos, assemblies, S, model)
    want["sites"] = S
    nq, na = len(oligos), len(assemblies)
    n_stable = np.zeros((nq, na), np.uint32)
    out = {f: np.full((nq, na), NO_SUM if f in STABLE_FIELDS[:3] else NO_HIT, np.int32 if f in STABLE_FIELDS[:3] else np.uint32) for f in STABLE_FIELDS}
    best = {}
    cols = [np.asarray(S[f]).tolist() for f in ("oligo", "assembly", "record", "pos", "strand", "mm", "dh", "ds", "dg")]
    for q, a, r, p, s, mm, dh, ds, dg in zip(*cols):
        if max_dg is None or dg <= max_dg:
            n_stable[q, a] += 1
        if (q, a) not in best or (dg, r, p, s) < best[q, a][:4]:
            best[q, a] = (dg, r, p, s, dh, ds, mm)
    for (q, a), (dg, r, p, s, dh, ds, mm) in best.items():
        for f, v in zip(STABLE_FIELDS, (dg, dh, ds, r, p, s, mm)):
            out[f][q, a] = v
    want.update(n_stable=n_stable, **out)
    return want
