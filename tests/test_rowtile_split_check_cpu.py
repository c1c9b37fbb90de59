"""Builds tests/rowtile_split_check.cpp -- a stand-alone program around pydynet_amd/csrc/rowtile_split_index.h, the header
from which the split-fp16 q | k | v and gate | up kernels (csrc/rowtile_split.hip) take every address they form -- with
the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for the shapes
of tests/test_rowtile_split_gpu.py and the benchmark's 131072 x 864 and 131072 x 1536.  The program walks every workgroup,
wave, lane, tile and drain step: global elements inside their buffers, LDS offsets inside the allocation, the W image equal
to what the fragment reads address, every element of qkv / gu / h / xn / rms written exactly once, every gate column beside
its own up column and every RoPE pair on its own table entry, across grid.y cuts too.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (kind, M, D or F, L, hd, up_first): kind 3 = q | k | v, kind 1 = gate | up
SHAPES = [(3, 16384, 288, 256, 48, 0), (3, 16384 + 64, 288, 64, 96, 0), (3, 65536, 288, 64, 96, 0), (3, 131072, 288, 256, 48, 0),
          (1, 16384, 768, 0, 0, 0), (1, 16384 + 37, 768, 0, 0, 1), (1, 65536, 192, 0, 0, 0), (1, 16384 + 37, 192, 0, 0, 0),
          (1, 131072, 768, 0, 0, 1)]


def test_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rowtile_split_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "rowtile_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    args = [str(v) for shape in SHAPES for v in shape]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every output element written once") == len(SHAPES)
