"""The amplicon stage on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): one plain case and one probe case
of tests/test_gpu_amplicons.py, in a fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_oligo.py),
and the two hook names, which the release library must not carry."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOOKS = ("SEQWIN_AMD_AMP_WAVE_RANGE", "SEQWIN_AMD_AMP_MAX_BLOCKS")


@pytest.mark.gpu
def test_amplicons_pass_on_the_release_library():
    env = {k: v for k, v in os.environ.items() if k not in HOOKS + ("SEQWIN_AMD_LIB",)}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_amplicons.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_length_bounds or test_probes", "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 2, tail


def test_the_release_library_carries_no_hook_name():
    rel, test = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    blob, tblob = rel.read_bytes(), test.read_bytes()
    for name in HOOKS:
        assert name.encode() not in blob, name
        assert name.encode() in tblob, name
