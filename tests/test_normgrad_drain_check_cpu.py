"""Builds tests/normgrad_drain_check.cpp -- a stand-alone program around pydynet_amd/csrc/outres_split_index.h, from which the
RMSNorm-backward drain of the split-fp16 output-resident product (ors_main_kernel<0, 1> of csrc/outres_split.hip) takes the
rows, columns and LDS floats it touches -- with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and
runs it as a process of its own for the row counts of tests/test_norm_bwd_fused_gpu.py and the benchmark's 131072: every
row of dx written once, no row >= M touched, the weight-gradient rows in LDS disjoint per wave and inside the allocation,
one partial row per workgroup.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [65536, 65536 + 3 * 128 + 5, 65536 + 1, 131072]


def test_drain_indices_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "normgrad_drain_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "normgrad_drain_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe] + [str(m) for m in ROWS], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every row of dx written once") == len(ROWS)
