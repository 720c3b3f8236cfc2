"""The loci on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the tests of
tests/test_gpu_best_hits_loci.py that need no hook, in a fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of
tests/test_release_library_align.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_loci_pass_on_the_release_library():
    hooks = ("SEQWIN_AMD_LIB", "SEQWIN_AMD_SCR_TABLE_BITS", "SEQWIN_AMD_HIT_BUFFER_KB", "SEQWIN_AMD_HIT_MAX_BLOCKS", "SEQWIN_AMD_DIST_LDS_CAP",
             "SEQWIN_AMD_SEQ_MAX_BLOCKS", "SEQWIN_AMD_SCR_MAX_BLOCKS", "SEQWIN_AMD_ALN_SCRATCH_KB")
    env = {k: v for k, v in os.environ.items() if k not in hooks}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    pick = ("test_hand_made_cases or test_random_case or test_loci_fetch_and_replay or test_accessors_need_loci or test_repeat_summary or "
            "test_markers_best_hits_loci")
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_best_hits_loci.py"), "-x", "-q", "-m", "gpu", "-k", pick,
                        "--deselect", "tests/test_gpu_best_hits_loci.py::test_random_case_under_the_hooks", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 8 + 3 + 4, tail
