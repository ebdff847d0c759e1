"""Run test files of this suite again on the bf16 build, in ONE fresh child process (a plain helper module, not a conftest).

The library is chosen at import (fedfr_amd/_C.py: FEDFR_HIP_LIB_NAME), so a process that has loaded libfedfr_hip.so cannot test
libfedfr_hip_bf16.so: run_on_bf16 starts a child whose environment names the bf16 library.  The child first asserts that the library it
loaded stores bfloat16 — the proof that the bf16 build ran is in the child itself, not in a pattern over parametrise ids — then runs pytest
on the given files and exits with its status.  A skip inside the child is how a bf16 run would hide a test, so the summary line must carry
passed tests and no skipped / xfailed / xpassed ones.

Stop rule of shared GPU machines: a child that faulted, aborted, was killed or hung ends the whole session (pytest.exit), so that nothing
further starts on the GPU after it; a child that merely has failing tests is an ordinary assertion failure."""
import os
import re
import subprocess
import sys
import time

import pytest
import torch

from fedfr_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_LIB = "libfedfr_hip_bf16.so"
NO_GRANDCHILD = "not child_process and not bf16_build"                 # the tests that start a bf16 child themselves
FATAL_RC = (-6, -11, -9, 134, 139, 137)                                  # abort, segmentation fault, kill: as a signal or as a shell status
FAULT_TEXT = "illegal memory access"

CHILD = """
import sys
import torch
from fedfr_amd import _C
assert _C.storage_dtype() == torch.bfloat16, (_C.LIB_PATH, _C.storage_dtype())
import pytest
sys.exit(int(pytest.main(%r)))
"""


def child_k(k):
    """the child's -k expression: ``k`` (may be empty) and never a test that starts a child of its own"""
    return "(%s) and %s" % (k, NO_GRANDCHILD) if k else NO_GRANDCHILD


def summary_counts(stdout):
    """{'passed': n, 'skipped': m, ...} of pytest's last summary line ('12 passed, 3 deselected in 4.05s')"""
    for line in reversed(stdout.splitlines()):
        if re.search(r"\bin [\d.]+s\b", line) and re.search(r"\d+ (passed|failed|error|errors|skipped|deselected)\b", line):
            return {w: int(n) for n, w in re.findall(r"(\d+) ([a-z]+)", line.split(" in ")[0])}
    return {}


def run_on_bf16(files, k, timeout_s):
    """``files`` (names under tests/) under -k ``k`` on libfedfr_hip_bf16.so in one child process; returns the number of tests that passed"""
    if _C.storage_dtype() != torch.float16:
        pytest.skip("this process already runs on the bf16 build")
    assert os.path.exists(os.path.join(ROOT, "fedfr_amd", BF16_LIB)), BF16_LIB + " is not built (make -C fedfr_amd/csrc bf16)"
    paths = [os.path.join(ROOT, "tests", f) for f in files]
    argv = [*paths, "-x", "-q", "-s", "-rs", "-p", "no:cacheprovider", "-k", child_k(k)]
    env = dict(os.environ, FEDFR_HIP_LIB_NAME=BF16_LIB)
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-c", CHILD % (argv,)], env=env, capture_output=True, text=True, timeout=timeout_s, cwd=ROOT)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        pytest.exit("the bf16 child of %s did not end within %d s (counts as hung: nothing further runs on the GPU)\n%s"
                    % (files, timeout_s, out[-3000:]), returncode=3)
    wall = time.perf_counter() - t0
    tail = r.stdout[-4000:] + r.stderr[-2000:]
    if r.returncode in FATAL_RC or FAULT_TEXT in r.stdout or FAULT_TEXT in r.stderr:
        pytest.exit("the bf16 child of %s faulted (status %d: nothing further runs on the GPU)\n%s" % (files, r.returncode, tail), returncode=3)
    assert r.returncode == 0, tail
    n = summary_counts(r.stdout)
    assert n.get("passed", 0) >= 1 and not any(n.get(w, 0) for w in ("skipped", "xfailed", "xpassed")), (n, tail)
    print("bf16 build, %s: %d passed in %.1f s" % (" ".join(files), n["passed"], wall))
    print("\n".join(t for t in r.stdout.splitlines() if "worst error" in t or "MEASURED" in t))
    return n["passed"]
