"""The k-mer containment screen on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the realistic shape --
64 synthetic genomes, 50 queries, k = 21 and 11 -- and the bitmap word bounds of tests/test_gpu_screen.py, which need no hook, in a
fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_minhash.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_screen_passes_on_the_release_library():
    hooks = ("SEQWIN_AMD_LIB", "SEQWIN_AMD_SCR_TABLE_BITS", "SEQWIN_AMD_SCR_BITMAP_KB", "SEQWIN_AMD_SCR_MAX_BLOCKS")
    env = {k: v for k, v in os.environ.items() if k not in hooks}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_screen.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_realistic_shape or test_bitmap_word_bounds", "-p", "no:cacheprovider"], capture_output=True, text=True,
                       cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 3, tail
