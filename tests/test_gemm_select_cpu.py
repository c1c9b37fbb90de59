"""Builds tests/gemm_select_check.cpp -- a stand-alone program around pydynet_amd/csrc/gemm_select.h, the host-only header in
which pdn_gemm_f32 chooses between the wave-streaming and the tiled kernel, their tile shape and their k-split -- with the
host compiler under AddressSanitizer and UndefinedBehaviorSanitizer, and runs it as a process of its own for every case of
tests/test_gemm_variants.py that pins a route, with the case's routing variables in that process's environment.  The program
gets the numbers `_gemm_pass` and `_mask_pass` hand to the library (extents, strides from `_layout`, base offsets as address
low bits, the batch, the slab workspace size, the entry's mask flags) and prints the route line from the formatter the library
prints it from; `_check_route` judges it as it judges the library's on a GPU.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import test_gemm_variants as gv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every table test_gemm_variants.py registers: (name, cases, parameter values)
TABLES = (("tiled_every_configuration_and_layout", gv.tiled_cases, range(len(gv.KCFGS))),
          ("scalar_staging", gv.scalar_cases, None),
          ("fused_column_sums", gv.colsum_cases, range(len(gv.KCFGS))),
          ("fused_column_sums_refused", gv.colsum_refused_cases, None),
          ("batches_over_two_splits", gv.batch_cases, None),
          ("slab_reduce_both_forms", gv.reduce_cases, None),
          ("degenerate_extents", gv.degenerate_cases, None),
          ("grid_y_limit", gv.grid_limit_cases, None),
          ("mask_epilogues", gv.mask_cases, gv.MASK_CFGS),
          ("mask_epilogues_scalar", gv.mask_scalar_cases, None),
          ("stream_kernels", gv.stream_cases, range(len(gv.STREAM_VARIANTS))),
          ("stream_batches_and_length_threshold", gv.stream_batch_and_threshold_cases, None))


def _all_cases():
    out = []
    for _, make, values in TABLES:
        for v in ([()] if values is None else [(v,) for v in values]):
            out.extend(make(*v))
    return out


def _call_numbers(c):
    """The arguments of gemm_select_check for a case: what `_gemm_pass` / `_mask_pass` pass to the library."""
    if c.entry == "gemm":
        _, a_str, _ = gv._layout(c.M, c.K, c.at, c.a_pad, c.nb, c.gaps[0], c.a_bcast)
        _, b_str, _ = gv._layout(c.K, c.N, c.bt, c.b_pad, c.nb, c.gaps[1])
        c_shape, _, _ = gv._layout(c.M, c.N, False, c.ldc_pad, c.nb, c.gaps[2], extra_rows=2)
        ws_bytes = int(np.prod(c_shape)) * 4 * c.slabs           # `_workspace`
        nb, flags = c.nb, (0, int(c.colsum >= 0), 0)
    else:
        _, a_str, _ = gv._layout(c.M, c.K, False, c.a_pad, (1, 1))
        _, b_str, _ = gv._layout(c.K, c.N, c.bt, c.b_pad, (1, 1))
        a_str = (0, 0, a_str[2], 1)                              # the mask entries take x / g with a row stride only, unbatched
        b_str = (0, 0, b_str[2], b_str[3])
        ws_bytes, nb, flags = 0, (1, 1), (1, 0, int(c.entry == "dx" and c.partials))
    return [c.M, c.N, c.K, nb[0], nb[1], a_str[2], a_str[3], b_str[2], b_str[3], a_str[0], a_str[1], b_str[0], b_str[1],
            4 * c.a_off, 4 * c.b_off, ws_bytes, *flags]


def test_the_tables_listed_here_are_the_registered_ones():
    registered = {n[len("test_"):-len("_gpu")] for n in vars(gv) if n.startswith("test_") and n.endswith("_gpu")}
    assert registered == {name for name, _, _ in TABLES}


def test_every_pinned_route_is_what_the_selector_chooses(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_select_check")
    build = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "gemm_select_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = _all_cases()
    routed = sum(1 for c in cases if c.route)
    # the cases without a route never reach the choice: refused calls and empty extents
    assert all(c.refuse or not c.writes for c in cases if not c.route)
    base = {k: v for k, v in os.environ.items() if k not in gv.ROUTING_VARS and k != "PDN_GEMM_NO_FIXED"}
    checked = 0
    for c in cases:
        if not c.route:
            continue
        assert all(k in gv.ROUTING_VARS for k in c.env), c.name
        run = subprocess.run([exe] + [str(v) for v in _call_numbers(c)], env={**base, **c.env}, capture_output=True, text=True,
                             timeout=60)
        assert run.returncode == 0, (c.name, run.stdout + run.stderr)
        gv._check_route(c, run.stdout)
        checked += 1
    print(f"{checked} routed cases checked, {len(cases) - routed} without a route left out")
    assert checked == routed and routed > 0
