"""Builds tests/rowtile_split_bwd_check.cpp -- a stand-alone program around pydynet_amd/csrc/rowtile_split_index.h for the
dh + SwiGLU backward form of csrc/rowtile_split.hip (rts_main_kernel<2>, the transposed source of rts_w_kernel) -- with the host
compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for the shapes of
tests/test_rowtile_split_bwd_gpu.py and the benchmark's 131072 x 768.  The program walks every workgroup, wave, lane, tile and
store step: every weight read once, the image where the fragments address it, every gu element read once by the lane that
writes the matching dgu element, every dgu element written once and none behind row M or column 2F, whole aligned 128-byte
lines per eight lanes, LDS offsets inside the allocation, every tile in one grid.y range.  For the A prologue of all three
forms (whole 128-byte lines, csrc/rowtile_split.hip), at the same shapes plus the benchmark's 131072 x 864 (q | k | v) and
131072 x 1536 (gate | up): every A element read once, eight whole lines per load instruction, the staging round trip, at most
two lanes per bank, xn and rms written once by the first column range only.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16384, 768), (16384 + 37, 768), (16384, 192), (65536, 96), (131072, 768)]      # (M, F)
# (kind, M, F or D): kinds 1 and 2 at the shapes above, kind 3 (D = 288: 864 columns) at their row counts, and 131072 x 1536
PROLOGUE = [(k, M, F) for k in (1, 2) for M, F in SHAPES] + [(3, M, 288) for M in (16384, 16384 + 37, 65536, 131072)]


def test_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rowtile_split_bwd_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "rowtile_split_bwd_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    args = [str(v) for shape in SHAPES for v in ("b",) + shape] + [str(v) for shape in PROLOGUE for v in ("p",) + shape]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every dgu element written once") == len(SHAPES)
    assert run.stdout.count("every A element read once by whole lines") == len(PROLOGUE)
