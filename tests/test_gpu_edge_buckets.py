"""The bucket route of the edge sort (radix_edge_buckets, csrc/radix.hip): two unstable bucket passes and an LDS finish per
sub-bucket instead of the LSD passes, the repair and the run-length pass.  By default only graphs of 2^26 keys and more take it;
SEQWIN_AMD_EDGE_SORT=bucket|lsd (test library) forces either route, SEQWIN_AMD_EDGE_BUCKET_CAP / _SLOTS lower its capacities so
small graphs reach the fallbacks.  Every case is compared with the oracle AND with the LSD route, byte for byte; which route ran
is read from the log line of SEQWIN_AMD_DEBUG_EDGE_REPAIR."""
from __future__ import annotations

import re

import numpy as np
import pytest

import oracle
from seqwin_amd import KmerGraph

pytestmark = pytest.mark.gpu

_LOG = re.compile(r"\[edge buckets\] (\d+) keys, (\d+) sentinels, digits (\d+)\+(\d+)\+(\d+) of (\d+) bits, largest sub-bucket (\d+) "
                  r"\(capacity (\d+), (\d+) slots\)(: radix passes instead)?")


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def _mutate(rng, s, rate):
    a = np.array(list(s))
    hit = rng.random(len(a)) < rate
    a[hit] = rng.choice(list("ACGT"), int(hit.sum()))
    return "".join(a)


def _write(path, records):
    path.write_text("".join(f">{name}\n{seq}\n" for name, seq in records))
    return path


def _family(tmp_path, rng, length, n_asm, rate=0.01):
    """n_asm assemblies of one ancestor: most pairs occur in every assembly (several copies of every edge key)"""
    base = _rand(rng, length)
    return [_write(tmp_path / f"fam{i}.fa", [("c1", _mutate(rng, base, rate)), ("c2", _rand(rng, 3000))]) for i in range(n_asm)]


def _hub(tmp_path, rng):
    """one 40-mer between 1500 different random spacers (a hub node with many neighbours), tandem repeats and homopolymers
    (pairs that repeat inside one assembly: the candidate search and k_subtract_repeats)"""
    motif = _rand(rng, 40)
    hubseq = "".join(motif + _rand(rng, 35) for _ in range(1500))
    paths = []
    for i in range(3):
        paths.append(_write(tmp_path / f"hub{i}.fa", [("hub", _mutate(rng, hubseq, 0.002 * i)), ("at", "AT" * 6000), ("rep7", "ACGGTCA" * 2500),
                                                        ("polyA", "A" * 9000), ("mix", "A" * 500 + "N" + "C" * 700 + "ACGT" * 300)]))
    return paths


def _tiny_records(tmp_path, rng, k, w):
    """one record per assembly, and records of exactly one window (one minimizer): hardly anything but record boundaries"""
    paths = [_write(tmp_path / f"one{i}.fa", [("r", _rand(rng, 4000))]) for i in range(3)]
    paths.append(_write(tmp_path / "windows.fa", [(f"r{j}", _rand(rng, k + w - 1)) for j in range(300)]))
    return paths


def _edges(paths, k, w, monkeypatch, route, **env):
    monkeypatch.setenv("SEQWIN_AMD_EDGE_SORT", route)
    monkeypatch.setenv("SEQWIN_AMD_DEBUG_EDGE_REPAIR", "1")
    for name in ("SEQWIN_AMD_EDGE_BUCKET_CAP", "SEQWIN_AMD_EDGE_BUCKET_SLOTS", "SEQWIN_AMD_SORT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, str(value))
    g = KmerGraph(paths, kmerlen=k, windowsize=w, n_cpu=2)
    return g.kmers, g.nodes, g.edges, g.record_offsets


def _check(paths, k, w, monkeypatch, capfd, expect_route="bucket", **env):
    """both routes against the oracle; returns the parsed log line of the bucket run"""
    ek, en, ee, eo, _ = oracle.build(paths, k, w)
    capfd.readouterr()
    lsd = _edges(paths, k, w, monkeypatch, "lsd", **{n: v for n, v in env.items() if n == "SEQWIN_AMD_SORT"})
    assert "[edge buckets]" not in capfd.readouterr().err
    got = _edges(paths, k, w, monkeypatch, "bucket", **env)
    err = capfd.readouterr().err
    for arrays in (lsd, got):
        assert np.array_equal(arrays[0], ek) and np.array_equal(arrays[1], en) and np.array_equal(arrays[3], eo)
        assert arrays[2].dtype == ee.dtype and np.array_equal(arrays[2], ee)
    assert got[2].tobytes() == lsd[2].tobytes()
    if len(ek) < 2:
        return None
    m = _LOG.search(err)
    assert m, err[-2000:]
    fell_back = m.group(10) is not None or "distinct keys: radix passes instead" in err
    assert fell_back == (expect_route == "lsd"), err[-2000:]
    keys, sentinels, b1, b2, b3, bits, largest, cap, slots = (int(x) for x in m.groups()[:9])
    assert keys == len(ek) - 1 and sentinels == len(np.unique(ek["record_idx"])) - 1 and bits % 2 == 0
    return dict(bits=bits, digits=(b1, b2, b3), largest=largest, n_nodes=len(en), n_edges=len(ee))


@pytest.mark.parametrize("sort", [None, "own"], ids=["counted-here", "counts-from-producer"])
@pytest.mark.parametrize("length,k,w,nb", [(20000, 21, 10, 14), (50000, 21, 10, 15), (60000, 17, 200, 11)])
def test_bucket_route_matches_lsd_route_and_oracle(tmp_path, monkeypatch, capfd, length, k, w, nb, sort):
    """nb even and odd, 2 nb no multiple of the digit width; a small graph leaves most of the 2^18 sub-buckets empty"""
    paths = _family(tmp_path, np.random.default_rng(length + w), length, 5)
    info = _check(paths, k, w, monkeypatch, capfd, **({"SEQWIN_AMD_SORT": sort} if sort else {}))
    assert info["bits"] == 2 * nb and info["bits"] % 9 and info["bits"] % 8, info
    assert info["n_edges"] > 1000


def test_hub_node_and_tandem_repeats(tmp_path, monkeypatch, capfd):
    paths = _hub(tmp_path, np.random.default_rng(5))
    for k, w in [(21, 20), (15, 10), (21, 200)]:
        info = _check(paths, k, w, monkeypatch, capfd)
        assert info["largest"] >= 50, info   # (the hub's and the repeats' pairs crowd one sub-bucket; the mean is below 3)


def test_records_of_one_minimizer(tmp_path, monkeypatch, capfd):
    paths = _tiny_records(tmp_path, np.random.default_rng(6), 21, 200)
    _check(paths, 21, 200, monkeypatch, capfd)
    _check(paths[3:], 21, 200, monkeypatch, capfd)   # nothing but records of one minimizer: every key a sentinel, no edge


def test_sub_bucket_at_below_and_above_capacity(tmp_path, monkeypatch, capfd):
    """the largest sub-bucket (sentinels not counted) decides before the second pass runs: at capacity and one below it the
    buckets are finished, one above it the radix passes sort the untouched multiset"""
    paths = _hub(tmp_path, np.random.default_rng(7))
    largest = _check(paths, 21, 20, monkeypatch, capfd)["largest"]
    assert largest > 2
    _check(paths, 21, 20, monkeypatch, capfd, SEQWIN_AMD_EDGE_BUCKET_CAP=largest)
    _check(paths, 21, 20, monkeypatch, capfd, SEQWIN_AMD_EDGE_BUCKET_CAP=largest + 1)
    _check(paths, 21, 20, monkeypatch, capfd, expect_route="lsd", SEQWIN_AMD_EDGE_BUCKET_CAP=largest - 1)
    _check(paths, 21, 20, monkeypatch, capfd, expect_route="lsd", SEQWIN_AMD_EDGE_BUCKET_CAP=largest - 1, SEQWIN_AMD_SORT="own")


def test_more_distinct_keys_than_lds_slots(tmp_path, monkeypatch, capfd):
    """a sub-bucket whose distinct keys overflow the LDS table is noticed in the finish kernel: radix passes on the same multiset
    (at k 15, w 10 the hub's sub-bucket holds 531 different pairs -- counted from the oracle's edges)"""
    paths = _hub(tmp_path, np.random.default_rng(5))
    info = _check(paths, 15, 10, monkeypatch, capfd, SEQWIN_AMD_EDGE_BUCKET_SLOTS=1024)
    assert info["largest"] >= 531, info
    for slots in (64, 256):
        _check(paths, 15, 10, monkeypatch, capfd, expect_route="lsd", SEQWIN_AMD_EDGE_BUCKET_SLOTS=slots)
    _check(paths, 15, 10, monkeypatch, capfd, expect_route="lsd", SEQWIN_AMD_EDGE_BUCKET_SLOTS=256, SEQWIN_AMD_SORT="own")


def test_small_graphs_keep_the_lsd_route_by_default(tmp_path, monkeypatch, capfd):
    """without the switch a small graph never takes the bucket route, whoever sorts it (the order-guard test relies on that)"""
    paths = _family(tmp_path, np.random.default_rng(9), 20000, 3)
    for name in ("SEQWIN_AMD_EDGE_SORT", "SEQWIN_AMD_EDGE_BUCKET_CAP", "SEQWIN_AMD_EDGE_BUCKET_SLOTS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SEQWIN_AMD_DEBUG_EDGE_REPAIR", "1")
    for sort in ("own", "rocprim"):
        monkeypatch.setenv("SEQWIN_AMD_SORT", sort)
        capfd.readouterr()
        g = KmerGraph(paths, kmerlen=21, windowsize=10, n_cpu=2)
        assert len(g.edges) > 1000 and "[edge buckets]" not in capfd.readouterr().err
