"""Builds tests/lm_head_dw_split_check.cpp -- a stand-alone program around pydynet_amd/csrc/split_tn_index.h, the
header from which the split-fp16 lm_head weight-gradient kernel (csrc/lm_head_dw_split.hip) takes every address it forms --
with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for the
shapes of tests/test_lm_head_dw_split_gpu.py and the benchmark's 131072 x 32000.  The program walks every workgroup, wave,
lane and piece: global byte ranges inside their buffers (clamped ones included), LDS offsets inside the allocation, every
16-byte chunk of the logits fetched exactly once, the plane pass's image equal to what the DMA copies and the fragment reads
address, the transposed read of the logits on the right token and column and free of bank conflicts.  Nothing is loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32768, 4000), (32768 + 160, 4000), (32768, 32000), (131072, 32000)]


def test_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lm_head_dw_split_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "lm_head_dw_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    args = [str(v) for shape in SHAPES for v in shape]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every logits chunk fetched once") == len(SHAPES)
