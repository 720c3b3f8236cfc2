"""GPU (-m gpu): the unsort's first pass inside k_nodes (index.hip: k_nodes<.., SCAT>, SEQWIN_AMD_UNSORT_FUSED) against the two
passes behind a plain k_nodes (the route it replaces, kept behind SEQWIN_AMD_UNSORT_FUSED=0) and against the oracle.

The fused route is taken where radix_unsort_perm takes its two unstable passes: more than 2^(UNSORT_BITS + 8) = 2^22 occurrences
(the index's top digit then has hi_bits = nbit - 22 bits), no direct scatter (by default up to 2^25 occurrences: lowered here with
SEQWIN_AMD_UNSORT_DIRECT) and the own radix sort (by default from 2^23 keys on: forced here with SEQWIN_AMD_SORT=own).  So the
smallest shapes at which it can go wrong lie just above 2^22 occurrences; with w = 4 (two minimizers in five bases) that is
~10 Mbp of synthetic genomes, not the workload.

A case that needs an exact number of occurrences gets it from a homopolymer record appended to the last assembly: every window
of it is a tie, the rightmost k-mer wins, so every further base is one further occurrence (and all of them are one node: a run
of RANK_REP words across tiles and digits).  The helper measures what the synthetic genomes give and sizes that record.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from seqwin_amd.device import Batch, host_checksums

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
K, W = 21, 4
TILE = 8192                    # NODES_TILE: occurrences per k_nodes workgroup
GENOMES = 8
SEED = 20261017


def _route_env(monkeypatch, fused):
    monkeypatch.setenv("SEQWIN_AMD_UNSORT_DIRECT", "0")     # no direct scatter at any size
    monkeypatch.setenv("SEQWIN_AMD_SORT", "own")            # radix.hip's passes below 2^23 keys too
    monkeypatch.setenv("SEQWIN_AMD_DEBUG_NODES", "1")
    if fused is None:
        monkeypatch.delenv("SEQWIN_AMD_UNSORT_FUSED", raising=False)
    else:
        monkeypatch.setenv("SEQWIN_AMD_UNSORT_FUSED", "1" if fused else "0")


def _routes(err):
    return [ln.split("unsort route ")[1].split(",")[0] for ln in err.splitlines() if ln.startswith("[nodes]")]


def _write_fasta(b, n_genomes, tmp, pad=0):
    """The first n_genomes assemblies of the batch as FASTA, one file each (a slice of the job, as bench.py --genomes takes
    one); pad > 0: a poly-A record of pad + K + W - 2 bases -- pad windows -- behind the last assembly's records."""
    offs, ids = b.records()
    paths = []
    for a in range(n_genomes):
        p = tmp / f"g{a}.fa"
        with open(p, "wb") as f:
            for r in range(int(offs[a]), int(offs[a + 1])):
                f.write(b">" + ids[a][r - int(offs[a])].encode() + b"\n" + b.record(r) + b"\n")
            if pad > 0 and a == n_genomes - 1:
                f.write(b">polyA\n" + b"A" * (pad + K + W - 2) + b"\n")
        paths.append(p)
    return paths


def _sized_paths(tmp, lo, hi, want=None, low_complexity=False):
    """FASTA files of GENOMES assemblies whose index at (K, W) has lo < n <= hi occurrences (n == want where given): synthetic
    genomes sized a little below, and the homopolymer record for the rest."""
    target = want if want is not None else (lo + hi + 1) // 2
    room = 40_000                                          # left to the homopolymer: well above the spread of the estimate
    rl = int((target - room) * (W + 1) / 2 / GENOMES)      # density 2 / (w + 1)
    tar = [i % 2 == 0 for i in range(GENOMES)]
    for _ in range(3):
        b = Batch.synthetic(GENOMES, 1, rl, n_ancestors=2, snp_ppm=20000, seed=SEED)
        ix = b.build_index(K, W, tar)
        n0 = ix.sizes()[0]
        ix.close()
        if 0 < target - n0 <= 4 * room:
            break
        b.close()
        rl = int(rl * (target - room) / n0)
    else:
        raise AssertionError(f"no synthetic batch within {4 * room} below {target} occurrences (last: {n0})")
    paths = _write_fasta(b, GENOMES, tmp, pad=target - n0)
    if want is not None:   # an exact number is wanted: count what the files give, and let the record make up a difference
        fb = Batch.from_fasta(paths, n_cpu=4)
        ix = fb.build_index(K, W, tar)
        n = ix.sizes()[0]
        ix.close()
        fb.close()
        if n != want:
            paths = _write_fasta(b, GENOMES, tmp, pad=target - n0 + want - n)
    b.close()
    if low_complexity:   # tandem repeats as test_low_complexity_and_ties builds them, in a ninth assembly
        p = tmp / "lc.fa"
        p.write_text(">polyA\n" + "A" * 20000 + "\n>at\n" + "AT" * 9000 + "\n>rep7\n" + "ACGGTCA" * 3000 + "\n>mix\n" +
                     "A" * 500 + "N" + "C" * 700 + "ACGT" * 300 + "\n")
        paths.append(p)
    return paths


def _build(paths, monkeypatch, capfd, fused):
    _route_env(monkeypatch, fused)
    tar = [i % 2 == 0 for i in range(len(paths))]
    b = Batch.from_fasta(paths, n_cpu=4)
    capfd.readouterr()
    ix = b.build_index(K, W, tar)
    routes = _routes(capfd.readouterr().err)
    out = ix.export()
    ix.close()
    b.close()
    assert routes == ["fused" if fused else "two passes"], routes
    return out


def _oracle(paths):
    tar = [i % 2 == 0 for i in range(len(paths))]
    ek, en, ee, eo, _ = oracle.build(paths, K, W)
    oracle.get_penalty(ek, en, eo, tar)
    return ek, en, ee


def _check(paths, monkeypatch, capfd, lo, hi, mod=None, with_oracle=False):
    got = _build(paths, monkeypatch, capfd, True)
    n = len(got[0])
    with capfd.disabled():
        print(f"occurrences: {n} = {n // TILE} tiles + {n % TILE}, index bits {int(n - 1).bit_length()}")
    assert lo < n <= hi, (n, lo, hi)
    if mod is not None:
        assert n % TILE == mod, (n, n % TILE)
    ref = _build(paths, monkeypatch, capfd, False)
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    if with_oracle:
        for a, b in zip(got, _oracle(paths)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    return got


def test_just_above_two_to_the_22_one_bit_digit_second_group_nearly_empty(tmp_path, monkeypatch, capfd):
    lo = 1 << 22
    _check(_sized_paths(tmp_path, lo, lo + TILE), monkeypatch, capfd, lo, lo + TILE, with_oracle=True)


@pytest.mark.parametrize("side", ["below", "above"])
def test_around_two_to_the_23_digit_of_one_and_of_two_bits(tmp_path, monkeypatch, capfd, side):
    edge = 1 << 23
    lo, hi = (edge - TILE, edge) if side == "below" else (edge, edge + TILE)
    got = _check(_sized_paths(tmp_path, lo, hi), monkeypatch, capfd, lo, hi)
    assert int(len(got[0]) - 1).bit_length() == (23 if side == "below" else 24)


@pytest.mark.parametrize("mod", [1, TILE - 1])
def test_partial_last_tile(tmp_path, monkeypatch, capfd, mod):
    """One occurrence, and all but one, in the last tile (both n are odd: the last live lane holds one occurrence)."""
    want = (1 << 22) + 3 * TILE + mod
    _check(_sized_paths(tmp_path, want - 1, want, want=want), monkeypatch, capfd, want - 1, want, mod=mod)


def test_odd_number_of_occurrences_mid_tile(tmp_path, monkeypatch, capfd):
    want = (1 << 22) + 5 * TILE + 2049                      # the last live lane sits in the second row's first wave, with one occurrence
    got = _check(_sized_paths(tmp_path, want - 1, want, want=want), monkeypatch, capfd, want - 1, want, mod=2049)
    assert len(got[0]) % 2 == 1


def test_two_to_the_24_two_bit_digit_several_groups(tmp_path, monkeypatch, capfd):
    lo, hi = (1 << 24) - (1 << 19), 1 << 24                 # four groups of 2^22, the last one nearly full
    _check(_sized_paths(tmp_path, lo, hi), monkeypatch, capfd, lo, hi)


def test_low_complexity_runs_across_tiles_and_digits(tmp_path, monkeypatch, capfd):
    """Tandem repeats and homopolymers: nodes of thousands of occurrences, whose RANK_REP words straddle tiles of k_nodes and
    digits of the scatter (the indices of one node's occurrences are consecutive: whole tiles of one digit)."""
    lo = 1 << 22
    _check(_sized_paths(tmp_path, lo + TILE, lo + (1 << 17), low_complexity=True), monkeypatch, capfd, lo, lo + (1 << 18),
           with_oracle=True)


def test_twelve_builds_alternating_two_sizes(tmp_path, monkeypatch, capfd):
    """Cursors and tickets are set up per build: nothing of an earlier build -- of another size, so of other digit ranges -- may
    be left for the next."""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    small = _sized_paths(tmp_path / "a", 1 << 22, (1 << 22) + TILE)
    large = _sized_paths(tmp_path / "b", 1 << 23, (1 << 23) + TILE)
    ref = {id(p): _build(p, monkeypatch, capfd, False) for p in (small, large)}
    _route_env(monkeypatch, True)
    batches = {id(p): Batch.from_fasta(p, n_cpu=4) for p in (small, large)}
    tar = [i % 2 == 0 for i in range(GENOMES)]
    for i in range(12):
        p = (small, large)[i % 2]
        capfd.readouterr()
        ix = batches[id(p)].build_index(K, W, tar)
        assert _routes(capfd.readouterr().err) == ["fused"]
        assert ix.checksums() == host_checksums(*ref[id(p)]), i
        if i >= 10:   # (the arrays themselves once per size: the checksums carry every field with its index)
            for a, b in zip(ix.export(), ref[id(p)]):
                assert np.array_equal(a, b), i
        ix.close()


_RETRY_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.environ["SW_ROOT"])
import oracle
from seqwin_amd._lib import check, lib
from seqwin_amd.device import Batch

def trips():
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    check(lib.sw_order_guard_trips(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value

paths = json.loads(os.environ["SW_PATHS"])
tar = [i % 2 == 0 for i in range(len(paths))]
ek, en, ee, eo, _ = oracle.build(paths, 21, 4)
oracle.get_penalty(ek, en, eo, tar)
b = Batch.from_fasta(paths, n_cpu=4)
out = {"trips_before": trips()}
os.environ["SEQWIN_AMD_FAULT_INJECT"] = "rank"          # the pair passes of the node sort mis-rank: k_nodes' order guard trips
for rnd in ("first", "second"):
    ix = b.build_index(21, 4, tar)
    K, N, E = ix.export()
    out[rnd + "_equal"] = bool(np.array_equal(K, ek) and np.array_equal(N, en) and np.array_equal(E, ee))
    out[rnd + "_trips"] = trips()
    out[rnd + "_n"] = len(K)
    ix.close()
print("RESULT " + json.dumps(out))
"""


def test_order_guard_retry_finds_fresh_cursors(tmp_path):
    """SEQWIN_AMD_FAULT_INJECT=rank (the hook of test_order_guard_detects_and_recovers_from_misranked_passes) above 2^22
    occurrences: k_nodes runs twice in the first build -- the second time after the cursors were used up by the first --, the
    result is the oracle's, and the next build trips nothing.  (Own process: the demotion lasts for the rest of the process.)"""
    lo = 1 << 22
    paths = _sized_paths(tmp_path, lo, lo + TILE)
    env = dict(os.environ, SW_ROOT=str(ROOT), SW_PATHS=json.dumps([str(p) for p in paths]), SEQWIN_AMD_SORT="own",
               SEQWIN_AMD_UNSORT_DIRECT="0", SEQWIN_AMD_UNSORT_FUSED="1", SEQWIN_AMD_DEBUG_NODES="1")
    env.pop("SEQWIN_AMD_RADIX_RANK", None)
    r = subprocess.run([sys.executable, "-c", _RETRY_CHILD], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    assert lo < out["first_n"] <= lo + TILE, out
    assert out["trips_before"] == [0, 0] and out["first_trips"] == [1, 0] and out["second_trips"] == [1, 0], out
    assert out["first_equal"] and out["second_equal"], out
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("[nodes]")]
    assert _routes(r.stderr) == ["fused"] * 3, lines        # attempt 0 (guard trips), attempt 1, and the second build
    assert "attempt 0" in lines[0] and "order guard 0" not in lines[0] and "attempt 1" in lines[1] and "attempt 0" in lines[2], lines
    assert lines[1].endswith("order guard 0") and lines[2].endswith("order guard 0"), lines


_RELEASE_CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["SW_ROOT"])
import oracle
from seqwin_amd._lib import LIB_PATH
from seqwin_amd.device import Batch
assert str(LIB_PATH).endswith("libseqwin_hip.so"), LIB_PATH
G, rl, k, w = 6, 5_700_000, 21, 1                      # w = 1: every k-mer an occurrence, 6 x (rl - 20) > 2^25
b = Batch.synthetic(G, 1, rl, n_ancestors=2, snp_ppm=20000, seed=20261017)
tar = [i % 2 == 0 for i in range(G)]
offs, ids = b.records()
paths = []
for a in range(G):
    p = os.path.join(os.environ["SW_TMP"], "r%d.fa" % a)
    with open(p, "wb") as f:
        for r in range(int(offs[a]), int(offs[a + 1])):
            f.write(b">" + ids[a][r - int(offs[a])].encode() + b"\n" + b.record(r) + b"\n")
    paths.append(p)
ix = b.build_index(k, w, tar)
K, N, E = ix.export()
ek, en, ee, eo, _ = oracle.build(paths, k, w)
oracle.get_penalty(ek, en, eo, tar)
assert np.array_equal(K, ek) and np.array_equal(N, en) and np.array_equal(E, ee)
print("RESULT", len(K))
"""


def test_release_library_default_routing_matches_oracle(tmp_path):
    """The library that ships, in a fresh interpreter, no switch set: above 2^25 occurrences (below, the ranks are scattered
    directly) the build takes the default unsort route; its arrays are the oracle's.  (The smallest shape that reaches that
    route without a switch: 34 M occurrences, most of the test's time is the oracle's -- about 0.7 s per million on the host.)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEQWIN_AMD_")}
    env.update(SW_ROOT=str(ROOT), SW_TMP=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", _RELEASE_CHILD], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    n = int([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0].split()[1])
    assert (1 << 25) < n <= (1 << 25) + (1 << 20), n
