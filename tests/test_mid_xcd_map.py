"""The block renumbering of split-K M-split GEMM launches (ffmi::mid_xcd_map,
ffmi_internal.h) checked on the CPU: tests/mid_xcd_map_check.cpp is compiled
for the host only and enumerates every grid (nblk 1-130, S 1-8, 1-3 row
blocks): a bijection, one slice set per XCD residue, row blocks of a weight
tile on equal residues wherever the plain numbering has them there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mid_xcd_map_bijective_and_grouped(tmp_path):
    exe = str(tmp_path / "mid_xcd_map_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17",
                    "-I/opt/rocm/include", os.path.join(ROOT, "tests", "mid_xcd_map_check.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    assert "3120 grids, 0 failures" in p.stdout
