"""The interval fetch and the edit distances on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the
golden cases that need no hook -- two marker goldens through Markers, get_cks with save_markers, the crafted intervals at every
alignment and the crafted pairs at the default block bound -- in a fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern
of tests/test_release_library_minhash.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_seqs_pass_on_the_release_library():
    env = {k: v for k, v in os.environ.items() if k not in ("SEQWIN_AMD_LIB", "SEQWIN_AMD_DIST_LDS_CAP", "SEQWIN_AMD_SEQ_MAX_BLOCKS")}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    pick = ("pan_a_k15_w20_c15 or smoke_k17_w10_c6 or test_get_cks_with_a_batch_and_save_markers or test_fetch_at_every_alignment_and_length "
            "or test_fetch_at_the_run_boundaries or default")
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_marker_seqs.py"), str(ROOT / "tests" / "test_gpu_seqs_direct.py"),
                        "-x", "-q", "-m", "gpu", "-k", pick, "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=str(ROOT), env=env,
                       timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 6, tail
