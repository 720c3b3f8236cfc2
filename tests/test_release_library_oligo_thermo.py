"""The oligo search with a nearest-neighbour model on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out):
the cases of tests/test_gpu_oligo_thermo.py that need no hook, in a fresh interpreter with SEQWIN_AMD_RELEASE_LIB=1 (the pattern of
tests/test_release_library_oligo.py)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HOOKS = ("SEQWIN_AMD_OLIGO_GROUP", "SEQWIN_AMD_OLIGO_BUFFER_KB", "SEQWIN_AMD_OLIGO_MAX_BLOCKS")


@pytest.mark.gpu
def test_oligo_thermo_passes_on_the_release_library():
    env = {k: v for k, v in os.environ.items() if k not in HOOKS + ("SEQWIN_AMD_LIB",)}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_oligo_thermo.py"), "-x", "-q", "-m", "gpu", "-k",
                        "test_sums_and_stable_sites or test_santalucia98_and_the_summary or test_the_key_bias_on_both_signs "
                        "or test_max_dg_counts_a_site_of_exactly_that_dg or test_blocks or test_refusals", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 12, tail
