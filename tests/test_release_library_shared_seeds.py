"""The shared seeds on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the duplication identity and the
cap of tests/test_gpu_best_hits_shared.py, which need no hook, in a fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of
tests/test_release_library_hits.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_shared_seeds_pass_on_the_release_library():
    hooks = ("SEQWIN_AMD_LIB", "SEQWIN_AMD_SCR_TABLE_BITS", "SEQWIN_AMD_HIT_BUFFER_KB", "SEQWIN_AMD_HIT_MAX_BLOCKS", "SEQWIN_AMD_DIST_LDS_CAP",
             "SEQWIN_AMD_SEQ_MAX_BLOCKS", "SEQWIN_AMD_SCR_MAX_BLOCKS")
    env = {k: v for k, v in os.environ.items() if k not in hooks}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_best_hits_shared.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_a_query_set_given_twice or test_the_cap", "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=str(ROOT), env=env,
                       timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 3 * 4 + 2, tail
