"""MinHash on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): one real-shaped case -- a few assemblies of
a few 10^4 bases, k = 21, S = 1000, sketches and counts against the restatement -- and mash.jaccard_matrix on paths, in a fresh
interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_markers.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_minhash_passes_on_the_release_library():
    env = {k: v for k, v in os.environ.items() if k not in ("SEQWIN_AMD_LIB", "SEQWIN_AMD_MH_CAND_CAP")}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_minhash.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_real_shaped_case or test_jaccard_matrix_on_paths", "-p", "no:cacheprovider"], capture_output=True, text=True,
                       cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 2, tail
