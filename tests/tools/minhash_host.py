"""Host restatement, in numpy, of the MinHash specification the device code follows (csrc/minhash.hip):
Mash 2.x at its defaults -- `mash sketch -k K -s S`, one sketch per file, and `mash dist` on the result.  Written from the
project's own specification, not from any Mash source; agreement with the `mash` binary itself has never been observed.

  hash     MurmurHash3_x64_128 (seed 42) over the k upper-case ASCII bytes of the canonical k-mer -- the smaller of the k-mer and its
           reverse complement as byte strings; h1 (the first 8 bytes) for k >= 17, its low 4 bytes for k <= 16; k in 1..32
  k-mers   every window of k valid bases (ACGTacgt) inside one record
  sketch   the S smallest distinct hash values of an assembly, ascending (fewer if it has fewer)
  pair     the merge walk of `mash dist` (pair_walk)
"""
from __future__ import annotations

import numpy as np

_C1 = np.uint64(0x87c37b91114253d5)
_C2 = np.uint64(0x4cf5ad432745937f)
U64 = np.uint64


def _rotl(x, r):
    return (x << U64(r)) | (x >> U64(64 - r))


def _fmix(k):
    k = k ^ (k >> U64(33))
    k = k * U64(0xff51afd7ed558ccd)
    k = k ^ (k >> U64(33))
    k = k * U64(0xc4ceb9fe1a85ec53)
    return k ^ (k >> U64(33))


def murmur3_x64_128(keys: np.ndarray, seed: int):
    """(h1, h2) of every row of ``keys`` (uint8[n, length]; all rows have the same length), vectorised over the rows."""
    keys = np.ascontiguousarray(keys, np.uint8)
    n, length = keys.shape
    n_words = 2 * ((length + 15) // 16)
    padded = np.zeros((n, max(n_words, 2) * 8), np.uint8)     # zero bytes behind the tail do not enter the tail words
    padded[:, :length] = keys
    w = padded.view("<u8")
    h1 = np.full(n, seed, U64)
    h2 = np.full(n, seed, U64)
    nb = length // 16
    with np.errstate(over="ignore"):
        for b in range(nb):
            k1, k2 = w[:, 2 * b].copy(), w[:, 2 * b + 1].copy()
            k1 = _rotl(k1 * _C1, 31) * _C2
            h1 = h1 ^ k1
            h1 = (_rotl(h1, 27) + h2) * U64(5) + U64(0x52dce729)
            k2 = _rotl(k2 * _C2, 33) * _C1
            h2 = h2 ^ k2
            h2 = (_rotl(h2, 31) + h1) * U64(5) + U64(0x38495ab5)
        tail = length & 15
        if tail > 8:
            h2 = h2 ^ (_rotl(w[:, 2 * nb + 1] * _C2, 33) * _C1)
        if tail > 0:
            h1 = h1 ^ (_rotl(w[:, 2 * nb] * _C1, 31) * _C2)
        h1 = h1 ^ U64(length)
        h2 = h2 ^ U64(length)
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = _fmix(h1), _fmix(h2)
        h1 = h1 + h2
        h2 = h2 + h1
    return h1, h2


def murmur3_bytes(data: bytes, seed: int) -> bytes:
    """The 16 result bytes for one key."""
    h1, h2 = murmur3_x64_128(np.frombuffer(data, np.uint8).reshape(1, len(data)), seed)
    return int(h1[0]).to_bytes(8, "little") + int(h2[0]).to_bytes(8, "little")


def smhasher_verification() -> int:
    """SMHasher's verification value of the function: keys bytes(range(i)) with seed 256 - i for i in 0..255, the 256 results
    concatenated and hashed with seed 0, first 4 bytes."""
    blob = b"".join(murmur3_bytes(bytes(range(i)), 256 - i) for i in range(256))
    return int.from_bytes(murmur3_bytes(blob, 0)[:4], "little")


def hash_bits(k: int) -> int:
    return 32 if k <= 16 else 64


def check_k(k: int) -> None:
    if not 1 <= k <= 32:
        raise ValueError(f"k-mer length must lie in 1..32, got {k}")


_CODE = np.full(256, 255, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i          # lower case counts as upper case
_ASCII = np.frombuffer(b"ACGT", np.uint8)


def canonical_kmers(seq: bytes, k: int) -> np.ndarray:
    """uint8[n, k]: the canonical form (upper-case ASCII) of every window of k valid bases of one record, in order."""
    check_k(k)
    codes = _CODE[np.frombuffer(seq, np.uint8)]
    if len(codes) < k:
        return np.zeros((0, k), np.uint8)
    bad = np.concatenate([[0], np.cumsum(codes == 255)])
    ok = (bad[k:] - bad[:-k]) == 0
    win = np.lib.stride_tricks.sliding_window_view(codes, k)[ok]
    if len(win) == 0:
        return np.zeros((0, k), np.uint8)
    rc = (3 - win[:, ::-1]).astype(np.uint8)
    # A < C < G < T is the order of the codes: compare the two as integers with the first base most significant
    shifts = (2 * np.arange(k - 1, -1, -1)).astype(U64)
    f_int = (win.astype(U64) << shifts).sum(axis=1, dtype=U64)
    r_int = (rc.astype(U64) << shifts).sum(axis=1, dtype=U64)
    canon = np.where((r_int < f_int)[:, None], rc, win)
    return _ASCII[canon]


def kmer_hashes(seq: bytes, k: int, seed: int = 42) -> np.ndarray:
    """The hash (uint64; below 2^32 for k <= 16) of every valid k-mer of one record, in order."""
    km = canonical_kmers(seq, k)
    if len(km) == 0:
        return np.zeros(0, U64)
    h1, _ = murmur3_x64_128(km, seed)
    return h1 & U64(0xFFFFFFFF) if k <= 16 else h1


def hash_kmer(kmer: bytes, seed: int = 42) -> int:
    """The hash of one k-mer given as text (its canonical form is taken)."""
    return int(kmer_hashes(kmer, len(kmer), seed)[0])


def sketch(records, k: int, s: int, seed: int = 42) -> np.ndarray:
    """The sketch of one assembly (an iterable of record sequences as bytes): its s smallest distinct hashes, ascending."""
    check_k(k)
    parts = [kmer_hashes(r, k, seed) for r in records]
    allh = np.unique(np.concatenate(parts)) if parts else np.zeros(0, U64)
    return allh[:s].astype(U64)


def read_fasta(path) -> list:
    """Record sequences of a plain FASTA file (what the library's reader keeps of a sequence line: everything but blanks)."""
    recs, cur = [], None
    for line in open(path, "rb").read().split(b"\n"):
        line = line.strip()
        if line.startswith(b">"):
            cur = []
            recs.append(cur)
        elif line and cur is not None:
            cur.append(line)
    return [b"".join(r) for r in recs]


def pair_walk(a, b, s: int):
    """(shared, total) of two ascending lists as `mash dist` computes them -- the literal walk."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    i = j = common = denom = 0
    while denom < s and i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif b[j] < a[i]:
            j += 1
        else:
            i += 1
            j += 1
            common += 1
        denom += 1
    if denom < s:
        denom += (len(a) - i) + (len(b) - j)
        denom = min(denom, s)
    return common, denom


def pair_fast(a, b, s: int):
    """The same two numbers without the walk (tests/test_minhash_cpu.py pins it to pair_walk): the walk visits the distinct
    values of the union in ascending order, so `total` is min(s, |union|) and `shared` counts the common values among the
    first s of the union (every common value lies before the place where a list runs out)."""
    a, b = np.asarray(a, U64), np.asarray(b, U64)
    u = np.union1d(a, b)
    common = np.intersect1d(a, b, assume_unique=True)
    shared = int(np.count_nonzero(np.searchsorted(u, common) + 1 <= s))
    return shared, int(min(s, len(u)))


def counts_block(offsets, hashes, s: int, rows, cols, pair=pair_fast):
    """(shared, total) as uint32[len(rows), len(cols)] for sketches in CSR form."""
    o = np.asarray(offsets, np.int64)
    sh = np.zeros((len(rows), len(cols)), np.uint32)
    to = np.zeros((len(rows), len(cols)), np.uint32)
    for i, r in enumerate(rows):
        ar = hashes[o[r]:o[r + 1]]
        for j, c in enumerate(cols):
            sh[i, j], to[i, j] = pair(ar, hashes[o[c]:o[c + 1]], s)
    return sh, to


def jaccard(shared, total) -> np.ndarray:
    """float64 shared / total as Python divides two ints; 0 / 0 raises ZeroDivisionError."""
    if np.any(np.asarray(total) == 0):
        raise ZeroDivisionError("division by zero")
    return np.asarray(shared, np.float64) / np.asarray(total, np.float64)


def expected_frac(j: np.ndarray) -> float:
    """kmers._expected_frac: mean(2J / (1 + J))."""
    return float(np.mean(2 * j / (1 + j)))
