"""The oligo windows on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the tests of
tests/test_gpu_windows_direct.py and tests/test_gpu_best_hits_windows.py that need no hook, in a fresh interpreter with
SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_align.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_both_libraries_export_the_windows():
    rel, tst = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    assert rel.exists() and tst.exists()
    for lib in (rel, tst):
        blob = lib.read_bytes()
        for name in (b"sw_batch_infix_windows\0", b"sw_batch_best_hits_windows\0", b"sw_windows_export\0", b"sw_windows_stats\0"):
            assert name in blob, (lib.name, name)


@pytest.mark.gpu
def test_the_windows_pass_on_the_release_library():
    hooks = ("SEQWIN_AMD_LIB", "SEQWIN_AMD_SCR_TABLE_BITS", "SEQWIN_AMD_HIT_BUFFER_KB", "SEQWIN_AMD_HIT_MAX_BLOCKS", "SEQWIN_AMD_DIST_LDS_CAP",
             "SEQWIN_AMD_SEQ_MAX_BLOCKS", "SEQWIN_AMD_SCR_MAX_BLOCKS", "SEQWIN_AMD_ALN_SCRATCH_KB")
    env = {k: v for k, v in os.environ.items() if k not in hooks}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    pick = ("test_crafted_pairs or test_shuffled_order or test_other_lengths_bounds_tails_and_groups or test_a_pair_on_the_bound or "
            "test_malformed_calls_raise or test_windows_of_the_winners or test_the_exhaustive_scan_finds_what_the_windows_promise or "
            "test_markers_best_hits_windows")
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_windows_direct.py"),
                        str(ROOT / "tests" / "test_gpu_best_hits_windows.py"), "-x", "-q", "-m", "gpu", "-k", pick, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 12, tail
