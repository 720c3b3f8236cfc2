"""Primers and probes on the oligo search of :meth:`seqwin_amd.device.Batch.oligo_hits` (csrc/oligo.hip):
the check of the oligos themselves, the products of primer pairs and two summaries.  NumPy on the site list; the list is small.

None of this has a counterpart in the reference.  It is not BLAST (no e-values): a site is a window with at most ``max_mismatch``
mismatches under IUPAC sets, a product is two sites that face each other at a distance inside the caller's bounds.  The names are
deliberately not those of ``MarkerMetrics``.

:class:`ThermoModel` is a nearest-neighbour model as integer tables that the caller owns: the device sums
them per hit, exactly; :func:`melting_temperature` is the one floating-point step, on the host.
"""
from __future__ import annotations

import numpy as np

MIN_LEN, MAX_LEN, MAX_OLIGOS, MAX_MISMATCH, MAX_THREE_PRIME, MAX_EDITS = 8, 32, 4096, 8, 8, 4
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT",
         "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
AMPLICON_FIELDS = ("pair", "assembly", "record", "start", "end", "orientation", "mm_f", "mm_r")


def check_oligos(oligos, max_mismatch: int = 0, three_prime: int = 0, max_edits=None):
    """The oligos as a list of ``bytes``, after the checks the library makes again: 1..4096 oligos of 8..32 IUPAC letters (either
    case, ``U`` = ``T``), ``max_mismatch`` in 0..8 and below the shortest oligo, ``three_prime`` in 0..8; with ``max_edits`` (the
    search with indels): 0..4, ``max_edits + three_prime`` below the shortest oligo, and ``max_mismatch``
    must be 0.  ValueError otherwise."""
    if isinstance(oligos, (str, bytes, bytearray)):
        raise ValueError("oligos must be a list of str or bytes, not one string")
    out = []
    for q in oligos:
        try:
            out.append(q.encode("ascii") if isinstance(q, str) else bytes(q))
        except UnicodeEncodeError:
            raise ValueError(f"oligo {len(out)} holds a character that is no IUPAC letter") from None
    if not 1 <= len(out) <= MAX_OLIGOS:
        raise ValueError(f"{len(out)} oligos; 1..{MAX_OLIGOS} are taken")
    for i, q in enumerate(out):
        if not MIN_LEN <= len(q) <= MAX_LEN:
            raise ValueError(f"oligo {i} has {len(q)} letters; {MIN_LEN}..{MAX_LEN} are taken")
        for j, c in enumerate(q):
            if chr(c).upper() not in IUPAC:
                raise ValueError(f"oligo {i} holds byte 0x{c:02x} at {j}, which is no IUPAC letter")
    shortest = min(len(q) for q in out)
    if int(max_mismatch) != max_mismatch or not 0 <= max_mismatch <= MAX_MISMATCH or max_mismatch >= shortest:
        raise ValueError(f"max_mismatch must lie in 0..{MAX_MISMATCH} and below the shortest oligo's {shortest} letters (got {max_mismatch})")
    if int(three_prime) != three_prime or not 0 <= three_prime <= MAX_THREE_PRIME:
        raise ValueError(f"three_prime must lie in 0..{MAX_THREE_PRIME} (got {three_prime})")
    if max_edits is not None:
        if max_mismatch:
            raise ValueError("max_edits and a non-zero max_mismatch exclude each other")
        if int(max_edits) != max_edits or not 0 <= max_edits <= MAX_EDITS:
            raise ValueError(f"max_edits must lie in 0..{MAX_EDITS} (got {max_edits})")
        if max_edits + three_prime >= shortest:
            raise ValueError(f"max_edits + three_prime must lie below the shortest oligo's {shortest} letters (got {max_edits} + {three_prime})")
    return out


def _sites(hits):
    return hits if isinstance(hits, dict) else hits.sites()


def amplicons(hits, lengths, pairs, min_len: int, max_len: int, n_assemblies=None):
    """The products of primer pairs on a site list.  ``hits`` is an :class:`~seqwin_amd.device.OligoHits` made with ``sites=True`` or
    its ``sites()`` dict; ``lengths[q]`` the length of oligo q; ``pairs`` an (n, 2) array of ``(f, r)`` oligo indices.  Per pair and
    record there are two orientations: ``+`` (0), a hit of f on strand 0 at ``pf`` and a hit of r on strand 1 at ``pr >= pf``, product
    ``[pf, pr + L_r)``; ``-`` (1), a hit of r on strand 0 at ``pr`` and a hit of f on strand 1 at ``pf >= pr``, product ``[pr, pf +
    L_f)``.  A product is kept iff ``min_len <= end - start <= max_len``; every combination counts; with ``f == r`` only ``+`` is
    counted; a product may span invalid bases.  Where the sites carry an ``end`` (a search with ``max_edits``: a site with a bulge is
    not L bases long) the product ends at the last site's ``end`` and ``mm_f`` / ``mm_r`` are the sites' ``dist``.  Returns ``(products, n_amplicons)``: a dict of arrays ``pair``, ``assembly``,
    ``record``, ``start``, ``end``, ``orientation``, ``mm_f``, ``mm_r``, ordered by those fields in that order, and
    ``n_amplicons[n_pairs, n_assemblies]`` (uint32).  ``n_assemblies`` is read from ``hits`` unless given.
    The same on the device, with probes and a ``dg`` filter: :meth:`seqwin_amd.device.OligoHits.amplicons` (this function is its yardstick)."""
    S = _sites(hits)
    lengths = np.asarray(lengths, np.int64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if n_assemblies is None:
        if isinstance(hits, dict):
            raise ValueError("n_assemblies must be given with a dict of sites")
        n_assemblies = hits.sizes()[1]
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(lengths)):
        raise ValueError("a pair names an oligo outside lengths")
    if min_len > max_len:
        raise ValueError(f"min_len {min_len} exceeds max_len {max_len}")
    oligo, strand = S["oligo"].astype(np.int64), S["strand"].astype(np.int64)
    rec, pos, asm, mm = S["record"].astype(np.int64), S["pos"].astype(np.int64), S["assembly"].astype(np.int64), (S["mm"] if "mm" in S else S["dist"]).astype(np.int64)
    site_end = S["end"].astype(np.int64) if "end" in S else pos + lengths[oligo]
    cols = []

    def side(q, s):
        idx = np.nonzero((oligo == q) & (strand == s))[0]
        return idx[np.lexsort((pos[idx], rec[idx]))]

    def products(pi, first, last, len_last, orientation, f_is_first):
        """every (site of `first` on strand 0, site of `last` on strand 1) of one record with a product length inside the bounds"""
        if not len(first) or not len(last):
            return
        slack = MAX_EDITS if "end" in S else 0     # a site spans len_last -+ slack bases; the bounds are applied to the true ends below
        key_last = (rec[last] << 32) + pos[last]   # pr in [pf + max(min_len - L, 0), pf + max_len - L] of the same record
        lo = np.searchsorted(key_last, (rec[first] << 32) + pos[first] + max(min_len - len_last - slack, 0), "left")
        hi = np.searchsorted(key_last, (rec[first] << 32) + np.minimum(pos[first] + max_len - len_last + slack, 0xFFFFFFFF), "right")
        n = np.maximum(hi - lo, 0)
        a = np.repeat(np.arange(len(first)), n)
        b = np.concatenate([np.arange(x, y) for x, y in zip(lo, hi) if y > x]) if n.sum() else np.zeros(0, np.int64)
        i, j = first[a], last[b]
        keep = (pos[j] >= pos[i]) & (site_end[j] - pos[i] >= min_len) & (site_end[j] - pos[i] <= max_len)
        i, j = i[keep], j[keep]
        start, end = pos[i], site_end[j]
        mf, mr = (mm[i], mm[j]) if f_is_first else (mm[j], mm[i])
        cols.append(np.stack([np.full(len(i), pi), asm[i], rec[i], start, end, np.full(len(i), orientation), mf, mr], 1))

    for pi, (f, r) in enumerate(pairs):
        products(pi, side(f, 0), side(r, 1), int(lengths[r]), 0, True)
        if f != r:
            products(pi, side(r, 0), side(f, 1), int(lengths[f]), 1, False)
    rows = np.concatenate(cols) if cols else np.zeros((0, 8), np.int64)
    rows = rows[np.lexsort(rows.T[::-1])] if len(rows) else rows
    out = {f: rows[:, i].astype(np.uint8 if f == "orientation" else np.uint32) for i, f in enumerate(AMPLICON_FIELDS)}
    n_amp = np.zeros((len(pairs), int(n_assemblies)), np.uint32)
    np.add.at(n_amp, (rows[:, 0], rows[:, 1]), 1)
    return out, n_amp


def oligo_summary(hits, n_tar: int) -> dict:
    """Per oligo, over the targets (assemblies below ``n_tar``) and the others: ``f_tar`` / ``f_neg``, the fraction of them with a
    hit (``nan`` for an empty side), and ``mean_best_mm_tar``, the mean ``best_mm`` over the targets with a hit (``nan`` without one);
    on a result with ``max_edits`` it is the mean ``best_dist``."""
    n = np.asarray(hits.n_sites() if hasattr(hits, "n_sites") else hits["n_sites"])
    if hasattr(hits, "best_dist"):
        best = np.asarray(hits.best_dist())
    else:
        best = np.asarray(hits["best_mm"] if "best_mm" in hits else hits["best_dist"])
    if not 0 <= n_tar <= n.shape[1]:
        raise ValueError(f"n_tar {n_tar} lies outside the {n.shape[1]} assemblies")
    has = n > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        f_tar = has[:, :n_tar].sum(1) / np.float64(n_tar) if n_tar else np.full(len(n), np.nan)
        f_neg = has[:, n_tar:].sum(1) / np.float64(n.shape[1] - n_tar) if n.shape[1] > n_tar else np.full(len(n), np.nan)
        s = np.where(has[:, :n_tar], best[:, :n_tar], 0).sum(1, dtype=np.float64)
        mean = s / has[:, :n_tar].sum(1)
    return dict(f_tar=f_tar, f_neg=f_neg, mean_best_mm_tar=mean)


def assay_summary(n_amplicons, n_tar: int) -> dict:
    """Per pair of :func:`amplicons`' ``n_amplicons``: ``f_tar_amplified`` (targets with a product), ``f_tar_single`` (targets with
    exactly one) and ``f_neg_amplified`` (the others with a product), as fractions; ``nan`` for an empty side."""
    n = np.asarray(n_amplicons)
    if not 0 <= n_tar <= n.shape[1]:
        raise ValueError(f"n_tar {n_tar} lies outside the {n.shape[1]} assemblies")
    n_neg = n.shape[1] - n_tar
    with np.errstate(invalid="ignore", divide="ignore"):
        f_amp = (n[:, :n_tar] > 0).sum(1) / np.float64(n_tar) if n_tar else np.full(len(n), np.nan)
        f_one = (n[:, :n_tar] == 1).sum(1) / np.float64(n_tar) if n_tar else np.full(len(n), np.nan)
        f_neg = (n[:, n_tar:] > 0).sum(1) / np.float64(n_neg) if n_neg else np.full(len(n), np.nan)
    return dict(f_tar_amplified=f_amp, f_tar_single=f_one, f_neg_amplified=f_neg)


# ---- nearest-neighbour thermodynamics of Hamming sites -----------------------------------------------------
MAX_DG = 15000           # |dg| of every entry and of init, cal/mol: 31 stacks + 2 ends + init stay below 2^19
NO_SUM = -2 ** 31        # a signed stable_* field of a cell without a hit (INT32_MIN)
GAS_CONSTANT = 1.987     # cal/(K mol)
PLANES = ("dh", "ds", "dg")


def _round_half_even(x):
    return np.rint(np.asarray(x, np.float64))   # (rint rounds halves to even)


class ThermoModel:
    """A nearest-neighbour model as integer tables owned by the caller.  Base codes A=0, C=1, G=2, T=3.

    ``stack`` int16[3, 4, 4, 4, 4]: planes ``dh`` (100 cal/mol), ``ds`` (0.1 cal/(K mol)) and ``dg`` (cal/mol), index ``[x1][x2][y1][y2]``
    -- ``x1 x2`` two consecutive oligo bases 5'->3', ``y1 y2`` the bases of the bound strand that face them (``y1`` pairs with ``x1``, so
    ``y`` is read 3'->5').  ``end`` int16[3, 2, 4, 4]: the terminal pair ``[x][y]`` at the oligo's 5' end (0) and 3' end (1).  ``init``
    int32[3].  Every ``dg`` entry and ``init[2]`` must satisfy ``|v| <= 15000``; ValueError otherwise and for a wrong shape or dtype
    (nothing is converted silently)."""

    def __init__(self, stack, end, init):
        for name, a, shape, dt in (("stack", stack, (3, 4, 4, 4, 4), np.int16), ("end", end, (3, 2, 4, 4), np.int16), ("init", init, (3,), np.int32)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape:
                raise ValueError(f"{name} must be a NumPy array of {np.dtype(dt).name}{list(shape)}")
        for name, a in (("stack", stack[2]), ("end", end[2]), ("init", init[2:])):
            if np.abs(a.astype(np.int64)).max() > MAX_DG:
                raise ValueError(f"a dg entry of {name} exceeds {MAX_DG} cal/mol in magnitude")
        self.stack, self.end, self.init = np.ascontiguousarray(stack), np.ascontiguousarray(end), np.ascontiguousarray(init)

    @classmethod
    def from_dh_ds(cls, stack_dh, stack_ds, end_dh, end_ds, init_dh, init_ds, temperature_K: float = 310.15) -> "ThermoModel":
        """The model of the ``dh`` / ``ds`` planes (integers in the tables' units: int-valued arrays of [4, 4, 4, 4], [2, 4, 4] and two
        scalars); the ``dg`` plane is filled per entry as ``round_half_even(100 * dh - temperature_K * ds / 10)`` -- a site's dG is
        the sum of ROUNDED entries, as a published dG37 table is used; the device never multiplies by a temperature."""
        def plane(dh, ds, shape, what):
            dh, ds = np.asarray(dh), np.asarray(ds)
            if dh.shape != shape or ds.shape != shape:
                raise ValueError(f"{what}_dh and {what}_ds must have the shape {list(shape)}")
            for a in (dh, ds):
                if not np.array_equal(a, np.rint(a)):
                    raise ValueError(f"{what}: dh and ds are integers, in 100 cal/mol and 0.1 cal/(K mol)")
            dg = _round_half_even(100.0 * dh.astype(np.float64) - np.float64(temperature_K) * ds.astype(np.float64) / 10.0)
            return np.stack([dh.astype(np.float64), ds.astype(np.float64), dg])

        st, en, ini = plane(stack_dh, stack_ds, (4, 4, 4, 4), "stack"), plane(end_dh, end_ds, (2, 4, 4), "end"), plane(init_dh, init_ds, (), "init")
        for name, a, dt in (("stack", st, np.int16), ("end", en, np.int16), ("init", ini, np.int32)):
            if np.abs(a).max() > np.iinfo(dt).max:
                raise ValueError(f"an entry of {name} does not fit {np.dtype(dt).name}")
        return cls(st.astype(np.int16), en.astype(np.int16), ini.astype(np.int32))


# SantaLucia 1998 (PNAS 95:1460), Table 2, the unified parameters: x1x2/y1y2 -> (dH kcal/mol, dS cal/(K mol))
_SANTALUCIA98 = {"AA/TT": (-7.9, -22.2), "AT/TA": (-7.2, -20.4), "TA/AT": (-7.2, -21.3), "CA/GT": (-8.5, -22.7), "GT/CA": (-8.4, -22.4),
                 "CT/GA": (-7.8, -21.0), "GA/CT": (-8.2, -22.2), "CG/GC": (-10.6, -27.2), "GC/CG": (-9.8, -24.4), "GG/CC": (-8.0, -19.9)}
_SANTALUCIA98_END_AT, _SANTALUCIA98_END_GC = (2.3, 4.1), (0.1, -2.8)


def santalucia98(mismatch_stack=(0, 0), mismatch_end=(0, 0), temperature_K: float = 310.15) -> ThermoModel:
    """The unified nearest-neighbour parameters of SantaLucia 1998 (PNAS 95:1460, Table 2) as a :class:`ThermoModel`: the ten
    Watson-Crick stacks and the six that follow by reading the duplex from its other strand, a terminal A.T / T.A pair (2.3 kcal/mol,
    4.1 cal/(K mol)) or G.C / C.G pair (0.1, -2.8) at whichever end it stands, ``init`` 0 and no symmetry term (an oligo against a
    genome is not a self-complementary duplex).

    A stack that contains a non-Watson-Crick pair takes ``mismatch_stack`` and a non-Watson-Crick terminal pair ``mismatch_end``, each
    ``(dh, ds)`` in the tables' integer units (100 cal/mol, 0.1 cal/(K mol)).  **The defaults (0, 0) are not published values**: no
    mismatch parameters are shipped.  A caller with the Allawi-SantaLucia mismatch tables passes them through
    :meth:`ThermoModel.from_dh_ds`."""
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    sdh = np.full((4, 4, 4, 4), int(mismatch_stack[0]), np.int64)
    sds = np.full((4, 4, 4, 4), int(mismatch_stack[1]), np.int64)
    for name, (dh, ds) in _SANTALUCIA98.items():
        x1, x2, y1, y2 = (code[c] for c in name.replace("/", ""))
        for a, b, c, d in ((x1, x2, y1, y2), (y2, y1, x2, x1)):       # the same duplex read from its other strand
            sdh[a, b, c, d], sds[a, b, c, d] = round(dh * 10), round(ds * 10)
    edh = np.full((2, 4, 4), int(mismatch_end[0]), np.int64)
    eds = np.full((2, 4, 4), int(mismatch_end[1]), np.int64)
    for x in range(4):
        dh, ds = _SANTALUCIA98_END_AT if x in (0, 3) else _SANTALUCIA98_END_GC
        edh[:, x, 3 - x], eds[:, x, 3 - x] = round(dh * 10), round(ds * 10)
    return ThermoModel.from_dh_ds(sdh, sds, edh, eds, 0, 0, temperature_K)


def melting_temperature(dh, ds, length, oligo_molar: float = 2.5e-7, na_molar: float = 0.05, divisor: float = 4.0):
    """A two-state estimate of Tm in degrees Celsius from a site's sums (``dh`` in 100 cal/mol, ``ds`` in 0.1 cal/(K mol)), float64 on
    the host: ``100 dh / (ds / 10 + 0.368 (length - 1) ln(na_molar) + R ln(oligo_molar / divisor)) - 273.15`` with R = 1.987; ``nan``
    where the denominator is not negative.  Not a replacement for a melting-curve tool."""
    dh, ds, length = np.asarray(dh, np.float64), np.asarray(ds, np.float64), np.asarray(length, np.float64)
    den = ds / 10.0 + 0.368 * (length - 1.0) * np.log(np.float64(na_molar)) + GAS_CONSTANT * np.log(np.float64(oligo_molar) / np.float64(divisor))
    with np.errstate(invalid="ignore", divide="ignore"):
        tm = 100.0 * dh / den - 273.15
    return np.where(den < 0, tm, np.nan)


def thermo_summary(o, n_tar: int) -> dict:
    """Per oligo of a result made with ``thermo=``, over the targets (assemblies below ``n_tar``) and the others: ``f_tar_stable`` /
    ``f_neg_stable``, the fraction of them with a stable hit (``n_stable > 0``; ``nan`` for an empty side), ``mean_stable_dg_tar``, the
    mean ``stable_dg`` (cal/mol) over the targets with a hit, and ``min_stable_dg_neg``, the least ``stable_dg`` over the others
    (``nan`` without a hit)."""
    n = np.asarray(o.n_stable() if hasattr(o, "n_stable") else o["n_stable"])
    dg = np.asarray(o.stable_dg() if hasattr(o, "stable_dg") else o["stable_dg"]).astype(np.int64)
    if not 0 <= n_tar <= n.shape[1]:
        raise ValueError(f"n_tar {n_tar} lies outside the {n.shape[1]} assemblies")
    n_neg = n.shape[1] - n_tar
    stable, has = n > 0, dg != NO_SUM
    with np.errstate(invalid="ignore", divide="ignore"):
        f_tar = stable[:, :n_tar].sum(1) / np.float64(n_tar) if n_tar else np.full(len(n), np.nan)
        f_neg = stable[:, n_tar:].sum(1) / np.float64(n_neg) if n_neg else np.full(len(n), np.nan)
        mean = np.where(has[:, :n_tar], dg[:, :n_tar], 0).sum(1, dtype=np.float64) / has[:, :n_tar].sum(1)
    least = np.where(has[:, n_tar:], dg[:, n_tar:], np.iinfo(np.int64).max).min(1, initial=np.iinfo(np.int64).max).astype(np.float64)
    least[~has[:, n_tar:].any(1)] = np.nan
    return dict(f_tar_stable=f_tar, f_neg_stable=f_neg, mean_stable_dg_tar=mean, min_stable_dg_neg=least)
