"""Rays from surface points, the atlas and the gutter fill without a GPU (ptss_generate_rays_surface / ptss_dilate_linear /
ptss_surface_atlas): the record layouts against the header, the exported symbols, the host build of csrc/ptsurface.h
(the specification of the device's rays) against a model that restates it in numpy float32 and Python integers
(tests/surface_common.py), the basis at the normals where the reference's rotation is 0 / 0, the rays' length against the existing
generator's, the cosine distribution at a fixed seed, the atlas, the gutter fill, and the sanitizers over a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from film_common import advance, turned_camera
from surface_common import (DILATE_SIZES, TRIANGLE, bad_points, chained_states, dilate_films, first_difference, good_points, host_states, make_points,
                            model_dilate, model_surface_rays, same_bytes, words)
from scene_update_common import triangles_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
MODES = ("normal", "cosine")


@pytest.fixture(scope="module")
def mixed():
    """(triangles, spheres) of the "mixed" preset: both kinds of primitive."""
    tri, sph = ptss.scene_records(ptss.Scene("mixed"))
    assert len(tri) >= 12 and len(sph) >= 12
    return tri, sph


def test_dtypes_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes and numpy mirrors."""
    point, params = ("surface", "a", "b", "flags"), ("structSize", "mode", "maxDistance", "reserved")
    body = "".join('printf("%%zu\\n", offsetof(ptss_surface_point, %s));' % f for f in point)
    body += "".join('printf("%%zu\\n", offsetof(ptss_surface_params, %s));' % f for f in params)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { printf("%zu\\n%zu\\n", sizeof(ptss_surface_point), '
                   'sizeof(ptss_surface_params)); ' + body +
                   ' printf("%d %d %u %d\\n", PTSS_SURFACE_NORMAL, PTSS_SURFACE_COSINE, PTSS_SURFACE_BACK, PTSS_SURFACE_TRIANGLE); return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    D, P = ptss.SURFACE_POINT_DTYPE, ptss_types.SurfaceParams
    assert got[:2] == [D.itemsize, C.sizeof(P)] == [16, 16]
    assert got[2:6] == [D.fields[f][1] for f in point] == [0, 4, 8, 12]
    assert got[6:10] == [getattr(P, f).offset for f in params] == [0, 4, 8, 12]
    assert got[10:] == [ptss.SURFACE_NORMAL, ptss.SURFACE_COSINE, ptss.SURFACE_BACK, ptss.SURFACE_TRIANGLE] == [0, 1, 1, 0x40000000]
    assert ptss_types.SPHERE_DTYPE.itemsize == C.sizeof(ptss_types.Sphere)


def test_libraries_export_the_symbols():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_generate_rays_surface", "ptss_dilate_linear", "ptss_surface_launches", "ptss_surface_rejected", "ptss_debug_dilate_linear_form"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_surface_rays", "ptss_probe_dilate_linear", "ptss_surface_atlas"):
        assert hasattr(ptss.host_lib(), name), name
    p = ptss.surface_params()
    # refused before anything touches a device
    assert L.ptss_generate_rays_surface(None, C.byref(p), None, 0, 0, None, 0, None, None, None, None) == -1
    assert L.ptss_dilate_linear(None, None, 1, 1, None, None) == -1
    assert L.ptss_surface_launches(None, (C.c_ulonglong * 2)()) == -1
    assert L.ptss_surface_rejected(None, C.byref(C.c_ulonglong())) == -1
    assert L.ptss_debug_dilate_linear_form(None, 0) == -1
    assert ptss.surface_draws(ptss.surface_params("normal")) == 0 and ptss.surface_draws(ptss.surface_params("cosine")) == 2


# ---- the probe against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_probe_equals_the_model(mixed, mode):
    """Triangles and spheres, both sides, corners and edges, with an index that holds duplicates; the streams move by draws(mode)."""
    tri, sph = mixed
    params = ptss.surface_params(mode, max_distance=float("inf") if mode == "cosine" else 2.5)
    pts = good_points(len(tri), len(sph), 96, seed=3)
    assert {int(f) for f in pts["flags"]} == {0, 1} and (pts["surface"] >= TRIANGLE).any() and (pts["surface"] < TRIANGLE).any()
    n = 160
    s0 = host_states(n)
    index = np.random.default_rng(5).integers(0, len(pts), n).astype(np.uint32)
    for idx, first in ((None, 7), (index, 0)):
        m = n if idx is not None else len(pts) - first
        rays, after, surfels, rejected = ptss.probe_surface_rays(tri, sph, pts, s0[:m], params, first_point=first, index=idx, surfels=True)
        want = model_surface_rays(tri, sph, pts, s0[:m], params, first_point=first, index=idx)
        assert rejected == want[3] == 0
        assert same_bytes(rays, want[0]), first_difference(rays, want[0])
        assert same_bytes(surfels, want[2]), first_difference(surfels, want[2])
        assert same_bytes(after, want[1])
        draws = ptss.surface_draws(params)
        for i in (0, m // 2, m - 1):
            assert np.array_equal(words(after)[i], advance(s0[i], draws)[0])
        assert (rays["tmax"] == params.maxDistance).all() and (rays["pad"] == 0).all() and (surfels["distance"] == 0).all()
        spheres = surfels["kind"] == 1
        assert spheres.any() and (surfels["w1"][spheres] == 0).all() and (surfels["w2"][spheres] == 0).all()
    # surfels=None: the same rays
    rays2, after2, none, _ = ptss.probe_surface_rays(tri, sph, pts, s0, params, index=index)
    assert none is None and same_bytes(rays2, rays) and same_bytes(after2, after)


@pytest.mark.parametrize("mode", MODES)
def test_every_rejection_is_counted_and_leaves_row_and_stream(mixed, mode):
    tri, sph = mixed
    params = ptss.surface_params(mode)
    names, bad = bad_points(len(tri), len(sph))
    good = good_points(len(tri), len(sph), 8, seed=9)
    pts = np.concatenate([good, bad])
    n = len(pts) + 3
    index = np.concatenate([np.arange(len(pts)), [len(pts), 2 ** 31, 2 ** 32 - 1]]).astype(np.uint32)   # three indices beyond the points
    s0 = host_states(n)
    marked_rays = np.full((n, 8), 7.5, dtype=np.float32)
    marked_surfels = np.full((n, 12), -3.25, dtype=np.float32)
    rays, after, surfels, rejected = ptss.probe_surface_rays(tri, sph, pts, s0, params, index=index, rays=marked_rays, surfels=marked_surfels)
    want = model_surface_rays(tri, sph, pts, s0, params, index=index, rays=marked_rays, surfels=marked_surfels)
    assert rejected == want[3] == len(bad) + 3
    assert same_bytes(rays, want[0]) and same_bytes(surfels, want[2]) and same_bytes(after, want[1])
    for k, name in enumerate(list(names) + ["index = numPoints", "index 2^31", "index 2^32 - 1"]):
        i = len(good) + k
        assert np.array_equal(words(rays)[i], words(marked_rays)[i]) and np.array_equal(words(surfels)[i], words(marked_surfels)[i]), name
        assert np.array_equal(words(after)[i], s0[i]), name
    for i in range(len(good)):
        assert not np.array_equal(words(rays)[i], words(marked_rays)[i])
    # each one alone is one rejection
    for k, name in enumerate(names):
        assert ptss.probe_surface_rays(tri, sph, bad[k:k + 1], s0[:1], params)[3] == 1, name


def test_the_probe_refuses_what_the_device_call_refuses(mixed):
    tri, sph = mixed
    pts, s0 = good_points(len(tri), len(sph), 4, seed=1), host_states(4)
    for change in (dict(structSize=12), dict(mode=2), dict(mode=-1), dict(reserved=1), dict(maxDistance=0.0), dict(maxDistance=-1.0),
                   dict(maxDistance=float("nan"))):
        p = ptss.surface_params()
        for k, v in change.items():
            setattr(p, k, v)
        with pytest.raises(ptss.PtssError):
            ptss.probe_surface_rays(tri, sph, pts, s0, p)
    with pytest.raises(ptss.PtssError):
        ptss.probe_surface_rays(tri, sph, pts, s0, first_point=1)   # firstPoint + n leaves the points
    assert ptss.probe_surface_rays(tri, sph, pts, s0[:3], first_point=1)[3] == 0
    assert ptss.probe_surface_rays(tri, sph, pts, s0, ptss.surface_params(max_distance=float("inf")))[3] == 0


# ---- the basis ------------------------------------------------------------------------------------------------------------------------
def flat_triangles(normals):
    """One triangle per normal: some geometry, all three vertex normals the given one (the interpolation then returns it)."""
    n = np.asarray(normals, dtype=np.float32)
    k = len(n)
    v0 = np.tile(np.array([[0.5, -1.0, -3.0]], dtype=np.float32), (k, 1))
    t = triangles_of(v0, v0 + np.float32([1, 0, 0]), v0 + np.float32([0, 0, 1]), 0, normals=np.repeat(n[:, None, :], 3, axis=1))
    return t


def unit_normals():
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.6, 0.8, -0.0), (0.0, 1.0, -0.0), (-1.0, 0.0, -0.0)]
    g = np.random.default_rng(17).normal(size=(300, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return np.concatenate([np.array(axes, dtype=np.float32), g.astype(np.float32)])


def test_the_basis_is_finite_and_keeps_every_sample_above_the_surface():
    """Every cosine direction is finite and dot(direction, n) > 0, for n over the six axis normals — (0, -1, 0), where the reference's
    rotation from (0, 1, 0) is 0 / 0, and (0, 0, -1), the basis' own pole —, n.z = -0.0 and 300 random unit normals, 48 samples each."""
    normals = unit_normals()
    assert np.signbit(normals[6][2]) and normals[6][2] == 0
    tri = flat_triangles(normals)
    per = 48
    pts = make_points([(TRIANGLE | t, 0.25, 0.25, 0) for t in range(len(tri))])
    index = np.repeat(np.arange(len(tri)), per).astype(np.uint32)
    rays, _, surfels, rejected = ptss.probe_surface_rays(tri, None, pts, chained_states(len(index), 2), ptss.surface_params("cosine"), index=index,
                                                         surfels=True)
    assert rejected == 0
    d, n = rays["direction"].astype(np.float64), surfels["normal"].astype(np.float64)
    assert np.isfinite(d).all() and np.isfinite(rays["origin"]).all()
    assert np.abs(n - normals[index].astype(np.float64)).max() < 2e-7   # the surfel's normal is the one asked for
    assert np.signbit(surfels["normal"][6 * per][2])                   # ... -0.0 included
    cos = (d * n).sum(axis=1)
    assert cos.min() > 0, (cos.min(), index[cos.argmin()])
    # the normal mode returns n itself
    rays_n = ptss.probe_surface_rays(tri, None, pts, np.zeros((len(pts), 6), np.uint32), ptss.surface_params("normal"))[0]
    assert np.abs(rays_n["direction"].astype(np.float64) - normals.astype(np.float64)).max() < 2e-7


def unit_error(rays):
    d = rays["direction"].astype(np.float64)
    return np.abs((d * d).sum(axis=1) - 1.0).max()


def test_directions_are_as_close_to_unit_length_as_the_film_generators(mixed):
    """|dot(d, d) - 1| over the probe's rays is at most twice the largest value ptss_probe_film_rays shows over as many pinhole rays: the
    yardstick is the existing generator, not a constant. (Measured: DESIGN.md §3.38.)"""
    tri, sph = mixed
    n = 128 * 128
    film = ptss.film_camera("pinhole", 128, 128, turned_camera())
    s0 = chained_states(n, 2)
    yardstick = unit_error(ptss.probe_film_rays(film, s0)[0])
    pts = good_points(len(tri), len(sph), 512, seed=21)
    index = np.random.default_rng(2).integers(0, len(pts), n).astype(np.uint32)
    worst = {mode: unit_error(ptss.probe_surface_rays(tri, sph, pts, s0, ptss.surface_params(mode), index=index)[0]) for mode in MODES}
    print(f"unit length: film {yardstick:.3e}, surface {worst}")
    assert 0 < yardstick < 1e-6
    assert max(worst.values()) <= 2 * yardstick, (worst, yardstick)


SKEW = np.array([0.36, -0.48, 0.8], dtype=np.float32)


@pytest.mark.parametrize("normal", [(0, 1, 0), (0, -1, 0), tuple(SKEW)])
def test_the_cosine_distribution_at_a_fixed_seed(normal):
    """Deterministic: seed 0x5EED, N = 65,536 pairs of draws at one point. The mean of dot(d, n) is within 6 sigma of 2 / 3 (sigma^2 =
    1 / 18 per draw: 0.0056) and each tangential mean within 6 sigma of 0 (sigma = 1 / 2 per draw: 0.0118)."""
    N = 65536
    tri = flat_triangles([normal])
    rays, _, _, rejected = ptss.probe_surface_rays(tri, None, make_points([(TRIANGLE, 0.3, 0.3, 0)]), chained_states(N, 2, seed=0x5EED),
                                                   ptss.surface_params("cosine"), index=np.zeros(N, np.uint32))
    assert rejected == 0
    n = np.asarray(normal, dtype=np.float64)
    n /= np.linalg.norm(n)
    helper = np.array([1.0, 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1.0, 0])
    t1 = np.cross(n, helper)
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    d = rays["direction"].astype(np.float64)
    mean_cos, mean_t1, mean_t2 = (d @ n).mean(), (d @ t1).mean(), (d @ t2).mean()
    print(f"normal {normal}: mean cos {mean_cos:.5f}, tangential {mean_t1:.5f} {mean_t2:.5f}")
    assert abs(mean_cos - 2.0 / 3.0) <= 6 * np.sqrt(1.0 / 18.0 / N)
    assert abs(mean_t1) <= 6 * 0.5 / np.sqrt(N) and abs(mean_t2) <= 6 * 0.5 / np.sqrt(N)


# ---- the atlas -----------------------------------------------------------------------------------------------------------------------
MIN_SIDE, MAX_SIDE, ATLAS_WIDTH = 2, 48, 128


def atlas_triangles():
    """Triangles whose longest edge is exactly k = 1 .. MAX_SIDE + 3 (sides MIN_SIDE .. MAX_SIDE at one texel per unit, both clamps), a tiny
    one, a huge one and one with a NaN vertex."""
    rows = [((0, 0, 0), (k, 0, 0), (0.5 * k, 0.125, 0)) for k in range(1, MAX_SIDE + 4)]
    rows += [((0, 0, 0), (1e-6, 0, 0), (0, 1e-6, 0)), ((0, 0, 0), (1e20, 0, 0), (0, 1e20, 0)), ((0, 0, 0), (float("nan"), 0, 0), (0, 1, 0))]
    v = np.array(rows, dtype=np.float32)
    return triangles_of(v[:, 0], v[:, 1], v[:, 2], 0, normals=np.tile(np.float32([0, 0, 1]), (len(v), 3, 1)))


def test_the_atlas():
    tri = atlas_triangles()
    points, texels, height = ptss.surface_atlas(tri, 1.0, ATLAS_WIDTH, MIN_SIDE, MAX_SIDE)
    assert ptss.surface_atlas(tri, 1.0, ATLAS_WIDTH, MIN_SIDE, MAX_SIDE, fill=False) == (len(points), height)   # the count-only call
    # every point lies strictly inside its triangle as float32 adds, and the probe accepts it
    a, b = points["a"], points["b"]
    assert (a > 0).all() and (b > 0).all() and ((a + b).astype(np.float32) < np.float32(1)).all() and (points["flags"] == 0).all()
    assert ptss.probe_surface_rays(tri, None, points, np.zeros((len(points), 6), np.uint32), ptss.surface_params("normal"))[3] == 0
    # one block per triangle, in the caller's order, of the side the rule gives
    owner = points["surface"] - TRIANGLE
    assert (np.diff(owner) >= 0).all() and set(owner.tolist()) == set(range(len(tri)))   # every triangle has at least one texel
    x, y = texels % ATLAS_WIDTH, texels // ATLAS_WIDTH
    assert len(set(texels.tolist())) == len(texels)
    blocks = []
    for t in range(len(tri)):
        mine = owner == t
        s = (int(x[mine].max()) - int(x[mine].min())) + 1
        assert mine.sum() == s * (s + 1) // 2 and int(y[mine].max()) - int(y[mine].min()) + 1 == s
        i, j = x[mine] - x[mine].min(), y[mine] - y[mine].min()
        assert (i + j <= s - 1).all()
        assert np.array_equal(a[mine], ((3 * i + 1).astype(np.float32) / np.float32(3 * s))), t
        assert np.array_equal(b[mine], ((3 * j + 1).astype(np.float32) / np.float32(3 * s))), t
        blocks.append((int(x[mine].min()), int(y[mine].min()), s))
    want = [min(max(k, MIN_SIDE), MAX_SIDE) for k in range(1, MAX_SIDE + 4)] + [MIN_SIDE, MAX_SIDE, MIN_SIDE]
    assert [s for _, _, s in blocks] == want and set(want) == set(range(MIN_SIDE, MAX_SIDE + 1))   # every side from minSide to maxSide
    assert height == max(y0 + s for _, y0, s in blocks) and all(x0 + s <= ATLAS_WIDTH for x0, _, s in blocks)
    for p, (xa, ya, sa) in enumerate(blocks):   # disjoint, and one texel apart
        for xb, yb, sb in blocks[p + 1:]:
            assert xa + sa + 1 <= xb or xb + sb + 1 <= xa or ya + sa + 1 <= yb or yb + sb + 1 <= ya, (p, (xa, ya, sa), (xb, yb, sb))
    # shelves: left to right, a new shelf when the next block does not fit
    assert blocks[0][:2] == (0, 0) and blocks[1][:2] == (blocks[0][2] + 1, 0)
    # a range of the table names the caller's indices
    sub, _, _ = ptss.surface_atlas(tri, 1.0, ATLAS_WIDTH, MIN_SIDE, MAX_SIDE, first=5, count=3)
    assert set((sub["surface"] - TRIANGLE).tolist()) == {5, 6, 7}
    # texelsPerUnit scales the sides
    assert ptss.surface_atlas(tri[:1], 7.5, ATLAS_WIDTH, 1, MAX_SIDE, fill=False)[0] == 8 * 9 // 2
    for bad in (dict(texels_per_unit=0.0), dict(texels_per_unit=float("nan")), dict(min_side=0), dict(max_side=MIN_SIDE - 1), dict(max_side=4097),
                dict(max_side=ATLAS_WIDTH + 1)):
        args = dict(texels_per_unit=1.0, width=ATLAS_WIDTH, min_side=MIN_SIDE, max_side=MAX_SIDE)
        args.update(bad)
        with pytest.raises(ptss.PtssError):
            ptss.surface_atlas(tri, **args)


def test_the_atlas_points_keep_a_plus_b_below_one_at_every_side():
    """a + b <= 1 in float32 for every texel of every side up to the largest the atlas allows (4096): the formula by itself."""
    for s in range(1, 4097):
        i = np.arange(s, dtype=np.int64)
        a = (3 * i + 1).astype(np.float32) / np.float32(3 * s)
        # the texels on the diagonal i + j = s - 1 have the largest sum
        b = (3 * (s - 1 - i) + 1).astype(np.float32) / np.float32(3 * s)
        assert ((a + b).astype(np.float32) < np.float32(1)).all(), s


# ---- the gutter fill -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", DILATE_SIZES)
def test_the_dilate_probe_equals_the_integer_model(width, height):
    for name, film in dilate_films(width, height).items():
        got = ptss.probe_dilate_linear(film, width, height)
        want = model_dilate(film, width, height)
        assert same_bytes(got, want), (name, first_difference(got, want))
        full = film["samples"] > 0
        assert same_bytes(got[full], film[full]), name   # a texel with samples is copied
        if name == "all empty":
            assert not words(got).any()
        # two passes equal the model's two passes
        assert same_bytes(ptss.probe_dilate_linear(got, width, height), model_dilate(want, width, height)), name
    if (width, height) == (17, 9):
        film = dilate_films(width, height)["wraps"]
        got = ptss.probe_dilate_linear(film, width, height)
        filled = (film["samples"] == 0) & (got["samples"] != 0)
        assert filled.any() and (got["r"][filled] != 0).any()


def test_the_dilate_probe_refuses_what_the_device_call_refuses():
    H = ptss.host_lib()
    film, out = np.zeros((4, 4), dtype=np.uint64), np.zeros((4, 4), dtype=np.uint64)
    f, o = film.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert H.ptss_probe_dilate_linear(f, 2, 2, o) == 0
    assert H.ptss_probe_dilate_linear(None, 2, 2, o) == -1 and H.ptss_probe_dilate_linear(f, 2, 2, None) == -1
    assert H.ptss_probe_dilate_linear(f, 2, 2, f) == -1                                           # never in place
    assert H.ptss_probe_dilate_linear(f, 0, 2, o) == -3 and H.ptss_probe_dilate_linear(f, 2, -1, o) == -3
    assert H.ptss_probe_dilate_linear(f, 1 << 16, 1 << 15, o) == -3                               # 2^31 texels


def test_the_dilate_fills_with_the_sample_weighted_mean():
    """An empty texel between a texel of 1 sample of value 10 and one of 3 samples of value 2: sums 16 over 4 samples, mean 4."""
    film = np.zeros(3, dtype=ptss.LINEAR_DTYPE)
    film[0], film[2] = (10, 10, 10, 1, 0), (6, 6, 6, 3, 1)
    got = ptss.probe_dilate_linear(film, 3, 1)
    assert tuple(got[1]) == (16, 16, 16, 4, 1) and same_bytes(got[[0, 2]], film[[0, 2]])


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------------
def test_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/surface_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host
    build of csrc/ptsurface.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "surface_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "surface_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("surface_sanitize ok"), r.stdout + r.stderr
