"""The alignments on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the tests of
tests/test_gpu_infix_alignments_direct.py and tests/test_gpu_best_hits_aligned.py that need no hook, in a fresh interpreter with
SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_hits.py); and the scratch hook's name is not in that binary
(the manner of tests/test_abi_cpu.py::test_release_library_carries_no_test_hooks)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_the_scratch_hook_is_in_the_test_library_only():
    rel, tst = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    assert rel.exists() and tst.exists()
    name = b"SEQWIN_AMD_ALN_SCRATCH_KB\0"
    assert name not in rel.read_bytes(), "SEQWIN_AMD_ALN_SCRATCH_KB is readable in the release library"
    assert name in tst.read_bytes(), "SEQWIN_AMD_ALN_SCRATCH_KB is missing from the test library"


@pytest.mark.gpu
def test_alignments_pass_on_the_release_library():
    hooks = ("SEQWIN_AMD_LIB", "SEQWIN_AMD_SCR_TABLE_BITS", "SEQWIN_AMD_HIT_BUFFER_KB", "SEQWIN_AMD_HIT_MAX_BLOCKS", "SEQWIN_AMD_DIST_LDS_CAP",
             "SEQWIN_AMD_SEQ_MAX_BLOCKS", "SEQWIN_AMD_SCR_MAX_BLOCKS", "SEQWIN_AMD_ALN_SCRATCH_KB")
    env = {k: v for k, v in os.environ.items() if k not in hooks}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    pick = ("test_crafted_pairs or test_without_scripts or test_malformed_pairs_raise or test_aligned_fields or test_votes_aligned or "
            "test_intervals_fetch_and_replay or test_alignment_summary or test_markers_best_hits_aligned")
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_infix_alignments_direct.py"),
                        str(ROOT / "tests" / "test_gpu_best_hits_aligned.py"), "-x", "-q", "-m", "gpu", "-k", pick, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 8, tail
