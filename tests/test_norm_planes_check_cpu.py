"""Builds tests/norm_planes_check.cpp -- a stand-alone program around pydynet_amd/csrc/split_tn_index.h, from which the plane
pass of an RMSNorm output (stn_split_xn_kernel of csrc/split_tn_planes.hip) takes every address -- with the host compiler
under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for K = 32768 (the fewest tokens
the route takes), 32768 + 32 and the benchmark's 131072: every 16 bytes of x and every rms read once and inside their buffers,
the exponents written once behind the images, every image equal to the old pass's on the same xn.  Nothing is loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [32768, 32768 + 32, 131072]


def test_plane_pass_indices_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "norm_planes_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "norm_planes_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe] + [str(k) for k in KS], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every image equal to the old pass's") == len(KS)
