"""Where the tame three-stage stage-wise kernels get their lane step multipliers from: the compile-time tables
(csrc/feasible_set.h kLaneScales) against lane_scale computed on the device, byte for byte, for both long-shot settings --
tools/lane_scale_check.hip, one 64-lane wave, built and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_lane_multipliers_old_and_new_are_byte_equal(tmp_path):
    exe = str(tmp_path / "lane_scale_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-function", "-Wno-pass-failed",
                    "-I", os.path.join(ROOT, "neo_mpc_planner2_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "lane_scale_check.hip"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    text = out.stdout.decode()
    print(text)
    assert out.returncode == 0, text
    assert "0 of 128 pairs differ" in text
