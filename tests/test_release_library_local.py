"""The local alignments on the RELEASE library (seqwin_amd/libseqwin_hip.so: test hooks compiled out): the tests of
tests/test_gpu_local_direct.py and tests/test_gpu_best_hits_local.py that need no hook, in a fresh interpreter with
SEQWIN_AMD_RELEASE_LIB=1 (the pattern of tests/test_release_library_hits.py); and the two hooks' names are not in that binary (the
manner of tests/test_abi_cpu.py::test_release_library_carries_no_test_hooks)."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
LOCAL_HOOKS = ("SEQWIN_AMD_LOCAL_ROWS", "SEQWIN_AMD_LOCAL_LDS_KB")


def test_the_local_hooks_are_in_the_test_library_only():
    rel, tst = ROOT / "seqwin_amd" / "libseqwin_hip.so", ROOT / "seqwin_amd" / "libseqwin_hip_test.so"
    assert rel.exists() and tst.exists()
    rel_bytes, tst_bytes = rel.read_bytes(), tst.read_bytes()
    for hook in LOCAL_HOOKS:
        name = hook.encode() + b"\0"
        assert name not in rel_bytes, f"{hook} is readable in the release library"
        assert name in tst_bytes, f"{hook} is missing from the test library"
    assert b"sw_batch_local_alignments\0" in rel_bytes and b"sw_batch_best_hits_local\0" in rel_bytes


@pytest.mark.gpu
def test_local_alignments_pass_on_the_release_library():
    hooks = ("SEQWIN_AMD_LIB", "SEQWIN_AMD_SCR_TABLE_BITS", "SEQWIN_AMD_HIT_BUFFER_KB", "SEQWIN_AMD_HIT_MAX_BLOCKS", "SEQWIN_AMD_DIST_LDS_CAP",
             "SEQWIN_AMD_SEQ_MAX_BLOCKS", "SEQWIN_AMD_SCR_MAX_BLOCKS", "SEQWIN_AMD_ALN_SCRATCH_KB") + LOCAL_HOOKS
    env = {k: v for k, v in os.environ.items() if k not in hooks}
    env["SEQWIN_AMD_RELEASE_LIB"] = "1"
    pick = ("test_crafted_pairs or test_outputs_may_be_absent or test_malformed_calls_raise or test_winners_against_the_restatement or "
            "test_loci_columns_against_the_restatement or test_half_a_copy_reads_as_a_clean_local_hit_and_local_summary or "
            "test_markers_best_hits_local")
    r = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_gpu_local_direct.py"),
                        str(ROOT / "tests" / "test_gpu_best_hits_local.py"), "-x", "-q", "-m", "gpu", "-k", pick, "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=str(ROOT), env=env, timeout=600)
    tail = r.stdout[-1500:]
    assert r.returncode == 0, tail + r.stderr[-1500:]
    assert " passed" in tail and "failed" not in tail and "skipped" not in tail, tail
    assert int(tail.split(" passed")[0].split()[-1]) == 9, tail
