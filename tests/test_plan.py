"""The host scheduler's planner (csrc/ct_plan.hpp) on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/sanitize/plan_driver.cpp plans pixel lists, job lists, chunks and measured orders over synthetic class planes and costs
and checks the properties of any correct plan (every listed pixel once, every group's subframes covered once, queues and
chunks that abut, orders that are permutations).  The bit-for-bit parity tests cannot see a bad plan -- the order and the job
lengths only change the schedule -- so this is where the schedule is checked.  The program is a stand-alone executable: it is
run directly, nothing is preloaded."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
SAN = ROOT / "tests" / "sanitize"


def _gcc_file(name):
    out = subprocess.run(["gcc", f"-print-file-name={name}"], capture_output=True, text=True).stdout.strip()
    return out if os.path.isabs(out) and Path(out).exists() else None


pytestmark = pytest.mark.skipif(not (_gcc_file("libasan.so") and shutil.which("make")), reason="gcc's libasan is not installed")


def test_planner_properties_under_sanitizers():
    subprocess.run(["make", "-C", str(SAN), "-s", "_build/plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(SAN / "_build" / "plan_asan")], env=env, capture_output=True, text=True, timeout=300)
    report = "AddressSanitizer" in r.stderr or "runtime error:" in r.stderr or "AddressSanitizer" in r.stdout
    assert r.returncode == 0 and not report, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "plan ok" in r.stdout
