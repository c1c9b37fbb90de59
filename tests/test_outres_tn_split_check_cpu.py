"""Builds tests/outres_tn_split_check.cpp -- a stand-alone program around pydynet_amd/csrc/split_tn_index.h, the
header from which the split-fp16 kernel of the packed layer weight gradients (csrc/outres_tn_split.hip) takes every address
it forms -- with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own
for the shapes of tests/test_outres_tn_split_gpu.py and the benchmark's 131072 x 864 and 131072 x 1536.  The program walks
every workgroup, wave, lane and piece: global byte ranges inside their buffers (clamped ones and padded rows included), LDS
offsets inside the allocation, every 16-byte chunk of g fetched exactly once, every slab element stored exactly once in the
block of its column, the plane pass's image equal to what the DMA copies and the fragment reads address, the transposed read
of g on the right token and column and free of bank conflicts, and the running exponent's rule.  Nothing is loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (K, columns per block, blocks, row stride of g)
SHAPES = [(32768, 288, 3, 864), (32768 + 96, 768, 2, 1536 + 64), (32768, 256, 3, 768), (131072, 288, 3, 864), (131072, 768, 2, 1536)]


def test_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "outres_tn_split_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "outres_tn_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    args = [str(v) for shape in SHAPES for v in shape]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every g chunk fetched once") == len(SHAPES)
    # both benchmark shapes: 64 and 42 K ranges, never fewer than the fp32 kernel's plan
    assert "K 131072 columns 3 x 288 (ldg 864): 64 K ranges of 2048 tokens (plan 64)" in run.stdout
    assert "K 131072 columns 2 x 768 (ldg 1536): 42 K ranges of 3136 tokens (plan 40)" in run.stdout
