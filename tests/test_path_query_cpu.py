"""Batched path queries without a GPU (ptss_seed_path_rng / ptss_trace_paths): the record layouts against the
header, the three exported symbols, and the condition under which the frame identity of tests/test_gpu_path_query.py holds — every
case of tests/path_query_common.py keeps more than 128 rays alive in every iteration on the oracle, so the frame's loop guard, which
a path query does not have, never fires. The condition is not a tolerance: a case that violates it is replaced in the common
module."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from path_query_common import CASES, ITERATIONS, SCENES, expected, expected_moved, make_scene, satisfies_identity_condition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_dtypes_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the numpy and ctypes mirrors."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ptss_path_rng), '
                   'offsetof(ptss_path_rng, v), offsetof(ptss_path_rng, d), sizeof(ptss_path_result), offsetof(ptss_path_result, radiance), '
                   'offsetof(ptss_path_result, bounces)); return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    rng, res = ptss_types.PATH_RNG_DTYPE, ptss_types.PATH_RESULT_DTYPE
    assert got == [rng.itemsize, rng.fields["v"][1], rng.fields["d"][1], res.itemsize, res.fields["radiance"][1], res.fields["bounces"][1]]
    assert got == [24, 0, 20, 16, 0, 12]
    assert got == [C.sizeof(ptss_types.PathRng), ptss_types.PathRng.v.offset, ptss_types.PathRng.d.offset, C.sizeof(ptss_types.PathResult),
                   ptss_types.PathResult.radiance.offset, ptss_types.PathResult.bounces.offset]
    assert rng.fields["v"][0].shape == (5,) and res.fields["radiance"][0].shape == (3,)
    assert ptss.PATH_RNG_DTYPE is rng and ptss.PATH_RESULT_DTYPE is res
    header = open(os.path.join(INC, "ptss_types.h")).read()
    for row in ("ptss_path_rng", "ptss_path_result"):   # asserted in C++ and in C, as the other rows are
        assert len(re.findall(r"\bstatic_assert\(sizeof\(%s\)" % row, header)) == 1 and len(re.findall(r"_Static_assert\(sizeof\(%s\)" % row, header)) == 1
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_library_exports_the_three_symbols():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_seed_path_rng", "ptss_trace_paths", "ptss_path_launches"):
        assert hasattr(L, name), name
    assert L.ptss_version() == 300
    # refused before anything touches a device
    assert L.ptss_trace_paths(None, None, None, None, 0, 4, None) == -1
    assert L.ptss_seed_path_rng(None, None, 0, 1, 0, 0, None) == -1
    assert L.ptss_path_launches(None, (C.c_ulonglong * 2)()) == -1


@pytest.mark.parametrize("name,iterations", CASES)
def test_case_keeps_the_loop_guard_silent(name, iterations):
    e = expected(name, iterations)
    assert satisfies_identity_condition(e.live_counts, iterations), (name, iterations, e.live_counts.tolist())
    assert e.live_counts[0] == 64 * 48


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_moved_mesh_keeps_the_loop_guard_silent(iterations):
    e = expected_moved(iterations)
    assert satisfies_identity_condition(e.live_counts, iterations), (iterations, e.live_counts.tolist())
    assert not np.array_equal(e.radiance, expected("mesh", iterations).radiance)   # the new pose is another image


def test_padding_changes_the_placement_and_nothing_else():
    """in_place() moves every scene of the cases from LDS to global memory, keeps its image kind, and leaves the tables the oracle
    reads as they were."""
    for name, (_, every, _, _) in SCENES.items():
        a, b = make_scene(name), make_scene(name, "in_place")
        la, _, lds_a = ptss.probe_pack_scene(a, every_sphere_loop=every)
        lb, _, lds_b = ptss.probe_pack_scene(b, every_sphere_loop=every)
        assert lds_a and not lds_b, name
        for field in ("numSpheres", "numTriangles", "numPointLights", "numAreaLights", "accelSpheres", "triClassed", "numChunks"):
            assert la[field] == lb[field], (name, field)
        assert (la["numLeaves"] > 0) == (lb["numLeaves"] > 0) or la["triClassed"], name
        assert b.desc.numTriangles == a.desc.numTriangles and b.desc.numMaterials == a.desc.numMaterials + 900
    kinds = {name: ptss.probe_pack_scene(make_scene(name), every_sphere_loop=SCENES[name][1])[0] for name in ("mesh", "many_spheres", "every_sphere_loop")}
    assert kinds["mesh"]["numTriangles"] >= 512 and not kinds["mesh"]["triClassed"] and kinds["mesh"]["numLeaves"] > 0   # the mesh image
    assert kinds["many_spheres"]["numSpheres"] >= 64 and kinds["many_spheres"]["accelSpheres"] == 1                       # the many-sphere image
    assert kinds["every_sphere_loop"]["accelSpheres"] == 0
