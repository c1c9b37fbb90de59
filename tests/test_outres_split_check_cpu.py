"""Builds tests/outres_split_check.cpp -- a stand-alone program around pydynet_amd/csrc/outres_split_index.h, the header
from which the split-fp16 output-resident products (csrc/outres_split.hip) take every address they form -- with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for the shapes of
tests/test_outres_split_gpu.py and the benchmark's 131072 x {864 as 3 x 288, 1536 as 2 x 768 at falling addresses, 768 NN}.
The program replays the W pass and the persistent main kernel: global elements inside their buffers, LDS offsets inside the
allocation, every weight read once, the image equal to what the fragments address and conflict free, every chunk of A
fetched exactly once and found where its lane reads it, every row block visited exactly once, every element of C written
exactly once, rows past M never touched.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (form, M, K, blocks, falling addresses, lda - K, ldc - 288): form 0 = NT, 1 = NN
SHAPES = [(0, 65536, 864, 3, 0, 0, 0), (0, 65536 + 40, 1536, 2, 1, 64, 32), (0, 65536 + 16, 256, 1, 0, 0, 0),
          (1, 65536, 768, 1, 0, 0, 0), (1, 65536, 4096, 1, 0, 0, 0),
          (0, 131072, 864, 3, 0, 0, 0), (0, 131072, 1536, 2, 1, 0, 0), (1, 131072, 768, 1, 0, 0, 0)]


def test_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "outres_split_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "outres_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    args = [str(v) for shape in SHAPES for v in shape]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every output element written once") == len(SHAPES)
