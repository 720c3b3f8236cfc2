"""Hand-made and random inputs for the loci of DESIGN.md section 3.2g, shared by tests/test_loci_cpu.py (the two forms of
tests/tools/loci_host.py against each other and against the lists written out here) and tests/test_gpu_best_hits_loci.py (the
device against loci_host).

k = 11 and one query of m = 60 bases unless a case says otherwise.  An exact copy of the query at record position P has its 50
k-mers at p = P + i, so every hit implies e = P + 49 and falls into band (P + 49) >> 6 with 50 seeds; the reverse complement planted
at P gives the same e with orientation 1.  A case is ``(queries, assemblies, rows)``; a row is the list entry (query, assembly,
record, strand, band, seeds, dist, end, start, nident, mismatch, gaps, dup) at min_seeds = 1, with None where the construction does
not determine the value (an alignment against random text)."""
import random

import hits_host as H

K = 11
COLS = ("query", "assembly", "record", "strand", "band", "seeds", "dist", "end", "start", "nident", "mismatch", "gaps", "dup")


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _other(base: int) -> int:
    return b"ACGT"[(b"ACGT".index(base) + 1) % 4]


def hand_made() -> dict:
    rng = random.Random(20)
    q = _rand(rng, 60)
    rc = H.revcomp(q)
    R = lambda n: _rand(rng, n)   # noqa: E731
    exact = lambda P: (0, P + 60, P, 60, 0, 0)   # noqa: E731  (dist, end, start, nident, mismatch, gaps)
    cases = {}

    # two exact copies five bands apart: two loci
    cases["two_copies"] = ([q], [[R(79) + q + R(260) + q + R(100)]],
                           [(0, 0, 0, 0, 2, 50) + exact(79) + (0,), (0, 0, 0, 0, 7, 50) + exact(399) + (0,)])

    # copies one band apart: band 2 scores 50 + 50 and suppresses band 3; copies two bands apart score 50 each: the smaller band wins
    cases["suppression"] = ([q], [[R(79) + q + R(4) + q + R(200)], [R(79) + q + R(68) + q + R(200)]],
                            [(0, 0, 0, 0, 2, 100) + exact(79) + (0,), (0, 1, 1, 0, 2, 50) + exact(79) + (0,)])

    # both strands on one record, and a second record of the same assembly
    cases["strands_records"] = ([q], [[R(79) + q + R(100) + rc + R(50), R(143) + rc + R(100)]],
                                [(0, 0, 0, 0, 2, 50) + exact(79) + (0,), (0, 0, 0, 1, 4, 50) + exact(239) + (0,),
                                 (0, 0, 1, 1, 3, 50) + exact(143) + (0,)])

    # a second and third assembly: a substitution at query position 30 (k-mers 20 .. 30 lost), a deletion of a query base d that
    # differs from both neighbours (the 11 k-mers that hold it are lost, and deleting it is deleting no other base)
    sub = q[:30] + bytes([_other(q[30])]) + q[31:]
    d = next(x for x in range(30, 45) if q[x - 1] != q[x] != q[x + 1])
    dele = q[:d] + q[d + 1:]
    cases["mutations"] = ([q], [[R(79) + q + R(100)], [R(79) + sub + R(100)], [R(89) + dele + R(100)]],
                          [(0, 0, 0, 0, 2, 50) + exact(79) + (0,), (0, 1, 1, 0, 2, 39, 1, 139, 79, 59, 1, 0, 0),
                           (0, 2, 2, 0, 2, 39, 1, 148, 89, 59, 0, 1, 0)])

    # one k-mer of the query (bases 20 .. 30) alone in an assembly, the bases around it not the query's: a locus of one seed
    lone = bytes([_other(q[19])]) + q[20:31] + bytes([_other(q[31])])
    cases["single_seed"] = ([q], [[R(79) + q + R(100)], [R(99) + lone + R(299)]],
                            [(0, 0, 0, 0, 2, 50) + exact(79) + (0,), (0, 1, 1, 0, 2, 1) + (None,) * 6 + (0,)])

    # the query's first 20 bases in band 2 (10 seeds) and a whole copy in band 5 that ends where band 2's window ends: both windows
    # settle on the whole copy
    cases["duplicate"] = ([q], [[R(89) + q[:20] + R(162) + q + R(100)]],
                          [(0, 0, 0, 0, 2, 10) + exact(271) + (0,), (0, 0, 0, 0, 5, 50) + exact(271) + (1,)])

    # the longest record (880) ends with the query's first 20 bases: e = 909, band 14 = (880 + 60) >> 6, the largest a key can hold
    # short of one; a band field of 4 bits makes 14 + 2 the band 0 of orientation 1, where the reverse complement sits with 50 seeds
    cases["last_band"] = ([q], [[rc + R(800) + q[:20]]],
                          [(0, 0, 0, 0, 14, 10) + (None,) * 6 + (0,), (0, 0, 0, 1, 0, 50) + exact(0) + (0,)])

    # a query shorter than k, an empty query, an assembly without a hit
    cases["empty"] = ([b"ACGTACG", b"", q], [[R(400)], [R(79) + q + R(100)]], [(2, 1, 1, 0, 2, 50) + exact(79) + (0,)])
    return cases


def random_small(seed: int):
    """A few short queries against a few short assemblies with copies planted at random: for the invariants."""
    rng = random.Random(seed)
    queries = [_rand(rng, rng.randint(40, 70)) for _ in range(3)]
    asms = []
    for _ in range(3):
        recs = []
        for _ in range(rng.randint(1, 2)):
            rec = bytearray(_rand(rng, rng.randint(300, 900)))
            for _ in range(rng.randint(0, 4)):
                c = bytearray(rng.choice(queries))
                if rng.random() < 0.5:
                    c = bytearray(H.revcomp(bytes(c)))
                for _ in range(rng.randint(0, 2)):
                    c[rng.randrange(len(c))] = rng.choice(b"ACGT")
                at = rng.randrange(len(rec))
                rec[at:at + rng.choice([0, len(c)])] = c[:rng.randint(15, len(c))]
            recs.append(bytes(rec))
        asms.append(recs)
    return queries, asms


def random_large(seed: int = 5):
    """The seeded case of the GPU test: 6 queries of 50 .. 200 nt and one above 64 x 64 nt (a unit twice and a tail); 5 assemblies of 2 .. 3 records of 2 .. 6
    knt; planted copies: exact, mutated, reverse-strand, tandem at 1, 2, 3 and 5 bands' spacing, a copy flush with a record's end,
    lone k-mers."""
    rng = random.Random(seed)
    unit = _rand(rng, 2080)
    queries = [_rand(rng, rng.randint(50, 200)) for _ in range(6)] + [unit + unit + _rand(rng, 40)]   # (seeds at the joint and the tail only:
    #                                   a k-mer inside the unit has two windows, so few lone hits ask for an alignment of 4200 rows)
    asms = []
    for a in range(5):
        recs = [bytearray(_rand(rng, rng.randint(2000, 6000))) for _ in range(rng.randint(2, 3))]
        for x, q in enumerate(queries[:6]):
            rec = recs[rng.randrange(len(recs))]
            if (a, x) == (1, 3):                                           # no copy, two seeds: a winner below min_seeds = 3
                rec[640:640 + K + 1] = q[20:20 + K + 1]
                continue
            at = 64 * rng.randint(4, (len(rec) - 1200) // 64)
            gap = 64 * (1, 2, 3, 5)[(a + x) % 4] - len(q) % 64
            for copy in range(3 if (a + x) % 2 else 1):                    # a tandem of three, or one copy
                c = bytearray(q if (a ^ x) & 1 else H.revcomp(q))
                if copy == 1 or a == 3:
                    for _ in range(rng.randint(1, 3)):
                        c[rng.randrange(len(c))] = rng.choice(b"ACGT")
                    if rng.random() < 0.5:
                        del c[rng.randrange(len(c))]
                p = at + copy * (len(q) + gap)
                rec[p:p + len(c)] = c
            if a == 4:
                rec[100:100 + K + 1] = q[7:7 + K + 1]                      # two seeds of their own
        if a % 2 == 0:
            big = queries[6] if a else H.revcomp(queries[6])
            recs.append(bytearray(_rand(rng, 300) + big[:2000] + _rand(rng, 3) + big[2000:] + _rand(rng, 200)))
        recs[0][len(recs[0]) - len(queries[a]):] = queries[a]              # flush with the record's end
        if a == 1:   # query 0's first 20 bases in band 4, a whole copy in band 7 that ends where band 4's window ends: a duplicate
            q, m = queries[0], len(queries[0])
            recs.append(bytearray(_rand(rng, 64 * 4 + 10 - (m - K)) + q[:20] + _rand(rng, 162) + q + _rand(rng, 150)))
        asms.append([bytes(r) for r in recs])
    return queries, asms
