"""Builds tests/weight_images_check.cpp -- a stand-alone program around pydynet_amd/csrc/weight_images_index.h, the header
from which the batched weight-image builder (csrc/weight_images.hip) takes its job table, its arena layout and its keys --
with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own.  The
program walks every workgroup and thread of sets that mix all five forms (the GPU tests' shapes, the benchmark's two layer
shapes, more descriptors than one launch takes): every tile, unit and exponent written exactly once, every write inside
its own image, the images disjoint, aligned and inside pdnw_set_bytes, every read inside the weight, and the descriptor
constructors' keys equal to the products' own.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_job_table_and_arena_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "weight_images_check")
    build = subprocess.run([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "weight_images_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("every one written once") == 4 and "the constructors' keys equal the products'" in run.stdout
    assert "all sets pass" in run.stdout
