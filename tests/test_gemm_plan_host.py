"""The GEMM launch planner (ffmi::plan_gemm, csrc/kernels/gemm_plan.h) checked
on the CPU: tests/gemm_plan_check.cpp is compiled with gemm_plan.cpp for the
host, under the address and undefined-behaviour sanitizers, and run as a
child process.  It sweeps T 1-1100 over the shapes of test_gemm_planner.py,
both epilogues, the layout flags, deferrable, the fused kinds and four
workspace sizes: every plan is inside the instantiation lists launch_gemm
dispatches over, its grid is non-empty, its split and slabs are consistent and
covered by ffmi_linear_workspace_bytes' formula; and it feeds the
FFMI_GEMM_PLAN parser hostile strings."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "flexflow_amd", "csrc", "kernels")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_every_plan_is_instantiated_and_consistent(tmp_path):
    exe = str(tmp_path / "gemm_plan_check")
    # (the sanitizer runtimes linked statically: no demand on the process's library order)
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "gemm_plan_check.cpp"),
                    os.path.join(KDIR, "gemm_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    # (the library's own switches would change the plans under test)
    env = {k: v for k, v in os.environ.items() if not k.startswith("FFMI_")}
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    m = re.search(r"(\d+) plans, 0 failures", p.stdout)
    assert m and int(m.group(1)) > 1_000_000, p.stdout[-500:]
