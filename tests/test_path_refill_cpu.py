"""The refill schedule of path queries without a GPU (ptss_trace_paths_opt / ptss_path_refill_stats): the options'
layout against the header, the exported symbols and what they refuse before touching a device, and the refill rule itself as a
pure-Python model (tests/path_refill_common.py): every ray is claimed once, the lane iterations are the paths' own, and the wave
iterations stay within the bound the GPU test holds the kernel's counters to."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from path_refill_common import BLOCK, CHUNKS, WAVES, plain_wave_iterations, simulate, wave_iteration_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
EINVAL = -1


def test_options_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes mirror."""
    fields = ("structSize", "schedule", "maxWorkgroups", "reserved")
    body = "".join('printf("%%zu\\n", offsetof(ptss_path_options, %s));' % f for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss.h"\nint main(void) { printf("%zu\\n", sizeof(ptss_path_options)); ' + body +
                   ' printf("%d %d\\n", PTSS_PATHS_LANE_PER_RAY, PTSS_PATHS_REFILL); return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = ptss_types.PathOptions
    assert got[0] == C.sizeof(P) == 16
    assert got[1:5] == [getattr(P, f).offset for f in fields] == [0, 4, 8, 12]
    assert got[5:] == [ptss.PATHS_LANE_PER_RAY, ptss.PATHS_REFILL] == [0, 1]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_library_exports_the_symbols_and_the_defaults():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_path_options", "ptss_trace_paths_opt", "ptss_path_refill_stats"):
        assert hasattr(L, name), name
    assert L.ptss_version() == 300
    o = ptss_types.PathOptions(77, 77, 77, 77)
    assert L.ptss_default_path_options(C.byref(o)) == 0
    assert (o.structSize, o.schedule, o.maxWorkgroups, o.reserved) == (16, ptss.PATHS_LANE_PER_RAY, 0, 0)
    assert L.ptss_default_path_options(None) == EINVAL
    p = ptss.path_options()
    assert (p.structSize, p.schedule, p.maxWorkgroups, p.reserved) == (16, 0, 0, 0)
    p = ptss.path_options("refill", 7)
    assert (p.structSize, p.schedule, p.maxWorkgroups, p.reserved) == (16, ptss.PATHS_REFILL, 7, 0)
    # a null context is refused before anything touches a device
    assert L.ptss_trace_paths_opt(None, None, None, None, 0, 4, C.byref(p), None) == EINVAL
    assert L.ptss_path_refill_stats(None, (C.c_ulonglong * 5)()) == EINVAL


# ---- the refill rule ------------------------------------------------------------------------------------------------------------------
def batches():
    """(what, bounces, maxIterations): random lengths 1 .. maxIterations, uniform and skewed like a scene's (most paths short, a few
    long), and the two extremes."""
    g = np.random.default_rng(2024)
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257, 1000, 3072, 5000):
        for max_iterations in (1, 2, 8, 15, 64):
            out.append((f"uniform n={n}", g.integers(1, max_iterations + 1, n), max_iterations))
            skew = np.minimum(1 + g.geometric(0.3, n), max_iterations) if max_iterations > 1 else np.ones(n, dtype=np.int64)
            out.append((f"skewed n={n}", skew, max_iterations))
    out.append(("all short", np.ones(3072, dtype=np.int64), 15))
    out.append(("all long", np.full(3072, 15, dtype=np.int64), 15))
    one_long = np.ones(3072, dtype=np.int64)
    one_long[::64] = 15   # the plain schedule's worst case: one long path in every wave
    out.append(("one long path per 64", one_long, 15))
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_refill_rule(chunk):
    order = np.random.default_rng(chunk)
    gained = 0
    for what, bounces, max_iterations in batches():
        n = len(bounces)
        full = (n + BLOCK - 1) // BLOCK
        for grid in sorted({1, 2, 7, full} & set(range(1, full + 1))):
            W = grid * WAVES
            run = simulate(bounces, grid, chunk, order)
            where = (what, max_iterations, grid, chunk)
            assert (run.claimed == 1).all(), where                       # every ray, exactly once
            assert run.lane_iterations == int(bounces.sum()), where      # the paths' own iterations, no more
            assert run.non_full_after_drain_only, where                  # every dead lane got a ray while the reserve or the head had any
            bound = wave_iteration_bound(bounces, W, max_iterations)
            assert run.wave_iterations <= bound, (where, run.wave_iterations, bound)
            assert run.per_wave.sum() == run.wave_iterations
            # at most one dequeue per chunk of the queue, plus the one per wave that finds the head past n
            queue = max(0, n - grid * BLOCK)
            assert run.dequeues <= (queue + chunk - 1) // chunk + W, where
            assert (run.dequeues > 0) == (queue > 0), where
            if grid == 1 and max_iterations == 15 and what in ("uniform n=3072", "skewed n=3072", "one long path per 64"):
                assert run.wave_iterations < plain_wave_iterations(bounces), where   # where the schedule is meant to pay
                gained += 1
    assert gained == 3


def test_the_plain_count_and_the_bound():
    b = np.array([3] * 64 + [1] * 63 + [15] + [2] * 10)
    assert plain_wave_iterations(b) == 3 + 15 + 2
    assert wave_iteration_bound(b, 4, 15) == (192 + 63 + 15 + 20) // 64 + 60
    one_long = np.ones(3072, dtype=np.int64)
    one_long[::64] = 15
    run = simulate(one_long, 1, 256, np.random.default_rng(1))
    assert plain_wave_iterations(one_long) == 48 * 15
    assert run.wave_iterations <= wave_iteration_bound(one_long, 4, 15) == (3072 + 48 * 14) // 64 + 60 < 48 * 15
