"""The node stage on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the sizes, run-boundary,
assembly-change and bitmap-word cases of tests/test_gpu_nodes_direct.py at default routing -- they set no hook --, in a fresh
interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_minhash.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_crafted_node_cases_pass_on_the_release_library():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SEQWIN_AMD_")}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_nodes_direct.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_sizes or test_run_boundaries or test_assembly_changes or test_bitmap_words", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 17 + 3 + 2 + 3, tail
