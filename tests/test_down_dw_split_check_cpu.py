"""Builds tests/down_dw_split_check.cpp -- a stand-alone program around pydynet_amd/csrc/split_tn_index.h, the header from
which the down-projection weight gradient on split-fp16 MFMA (csrc/outres_tn_split.hip, one block, transposed store) and the
whole-line plane pass (csrc/split_tn_planes.hip) take every address they form -- with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for the shapes of
tests/test_down_dw_split_gpu.py and the benchmark's 131072 x 768.  The program walks every workgroup, wave, lane and piece:
global byte ranges inside their buffers (clamped ones and padded rows included), every 16-byte chunk of h fetched exactly once,
every element of every (M x 288) slab stored exactly once by aligned 16-byte stores of one output row, no store behind the
last slab; and the plane pass: every chunk of a piece loaded once, every unit of the image written once in image order in
whole lines, found in LDS where it was staged.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (K, rows of dW_down = columns of h, row stride of h, row stride of g2)
SHAPES = [(32768, 768, 768, 288), (32768 + 96, 768, 768 + 64, 288 + 32), (32768, 592, 592, 288), (32768 + 96, 592, 592, 288),
          (131072, 768, 768, 288)]


def test_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "down_dw_split_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "down_dw_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    args = [str(v) for shape in SHAPES for v in shape]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every slab element stored once") == len(SHAPES)
    assert run.stdout.count("every unit in image order, whole lines") == len(SHAPES) + 1
    # the benchmark's shape: one round of 6 x 42 workgroups; 592 rows: 5 column blocks, the last with three idle waves, and
    # 1027 pieces in ranges of 21 (256 / 5 = 51 ranges asked for): 49 ranges, the last of 19 pieces
    assert "K 131072 rows 768 (ldh 768, ldg2 288): 42 K ranges of 3136 tokens, 6 column blocks" in run.stdout
    assert "K 32864 rows 592 (ldh 592, ldg2 288): 49 K ranges of 672 tokens, 5 column blocks" in run.stdout
