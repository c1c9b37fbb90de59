"""The 288 x 288 products that pdn_gemm_f32 sends to the split-fp16 output-resident kernel (csrc/outres_split.hip) have nine
pieces of 32 contraction values, one more than the shortest K that kernel takes.  This builds tests/outres_split_check.cpp
-- the stand-alone program around pydynet_amd/csrc/outres_split_index.h, from which the kernel takes every address it forms
-- with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer and runs it as a process of its own for the
shapes of tests/test_rowtile_split_forms_gpu.py and the benchmark's 131072 x 288, NN and NT: global elements inside their
buffers, LDS offsets inside the allocation, every weight read once, every chunk of A fetched exactly once and found where its
lane reads it, every row block visited exactly once, every element of C written exactly once, rows past M never touched.
Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (form, M, K, blocks, falling addresses, lda - K, ldc - 288): form 0 = NT, 1 = NN
SHAPES = [(1, 65536, 288, 1, 0, 0, 0), (1, 65536 + 37, 288, 1, 0, 64, 128), (0, 65536, 288, 1, 0, 0, 0),
          (0, 65536 + 37, 288, 1, 0, 0, 0), (1, 131072, 288, 1, 0, 0, 0), (0, 131072, 288, 1, 0, 0, 0)]


def test_nine_piece_walk_under_sanitizers(tmp_path):
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
