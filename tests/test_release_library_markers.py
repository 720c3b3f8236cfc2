"""The marker step on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the goldens through the resident
route, which needs no hook, in a fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_marker_goldens_pass_on_the_release_library():
    env = {k: v for k, v in os.environ.items() if k != "SEQWIN_AMD_LIB"}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_markers.py"), "-x", "-q", "-m", "gpu", "-k",
                        "golden_through_the_resident_route or get_cks", "-p", "no:cacheprovider"], capture_output=True, text=True,
                       cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) >= 9, tail


def test_the_real_spills_pass_on_the_release_library():
    """A pair of 385 items, a vote over 1 537 rows and spilling votes on either side of one in LDS: they need no hook."""
    env = {k: v for k, v in os.environ.items() if k != "SEQWIN_AMD_LIB"}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_markers_bounds.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_bounds_at_the_default_bounds and (pair_n385 or vote_T1537 or two_votes_mixed)", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 3, tail
