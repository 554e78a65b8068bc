"""Per-pixel motion and reprojection across moving triangles, without a GPU (ptss_render_features_motion / ptss_reproject_motion;
DESIGN.md §3.20): the new C-ABI symbols and the layout of ptss_pixel_motion, the argument checks that must not touch a device,
csrc/ptmotion.h through ptss_probe_motion against a float64 restatement, the identity with ptss_probe_reproject when nothing moved,
and ptss_probe_reproject_motion against an independent float64 model of §3.19 with the point of §3.20.

The tolerance of the moved-triangle rows is derived, not tuned (see motion_tolerance). The float64 model of the reprojection
leaves out the pixels at which a threshold decision lies within a relative 1e-4 of its threshold (cap: 2 % of a case's pixels;
measured below 0.01 % in all four cases). The floor of a tap coordinate is NOT such a decision here, unlike in
tests/test_reproject_cpu.py: the output is continuous across it (the tap that appears or disappears carries a bilinear weight of
the order of the rounding), and with a fixed camera every static pixel sits exactly on it. Measured on the host build (x86-64)
over the kept pixels of the four cases, largest |host - model|: colour 2.46e-03 on the 0..255 scale (both cases with the camera
fixed: a static pixel's tap coordinate is its own integer up to a few ulps of 63, about 1e-5, and that much bilinear weight moves
to a neighbouring entry of a history whose noise spans up to 100 units; with the camera moved 4.19e-04), weight 4.03e-04 on
weights up to 68; the tolerances are four times that."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptss
from ptss_types import PixelMotion, SURFACE_TRIANGLE
from test_reproject_cpu import (BAD_PARAMS, H, W, camera, colours, features_of, near, noisy_accum, noisy_history, pack, params, plane_hit,
                                quat_rotate, rays_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

MEASURED_MAX_COLOUR = 2.46e-03
MEASURED_MAX_WEIGHT = 4.03e-04
COLOUR_TOLERANCE = 4 * MEASURED_MAX_COLOUR
WEIGHT_TOLERANCE = 4 * MEASURED_MAX_WEIGHT
assert COLOUR_TOLERANCE < 0.5   # beyond that the model and the header are not the same arithmetic
MAX_LEFT_OUT = 0.02


# ---- symbols, layouts, argument checks ------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    dev, host = C.CDLL(ptss.DEVICE_LIB), C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_render_features_motion", "ptss_reproject_motion"):
        assert hasattr(dev, name), name
    for name in ("ptss_probe_motion", "ptss_probe_reproject_motion"):
        assert hasattr(host, name), name


def test_pixel_motion_matches_the_c_layout(tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ptss.h"\n#include "ptss_host.h"\n'
           'int main(void){printf("%zu %zu %zu %d", sizeof(ptss_pixel_motion), offsetof(ptss_pixel_motion, prevPoint), '
           'offsetof(ptss_pixel_motion, surface), PTSS_SURFACE_TRIANGLE); return 0;}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got == [16, 0, 12, 0x40000000]
    assert C.sizeof(PixelMotion) == 16 and PixelMotion.surface.offset == 12 and SURFACE_TRIANGLE == 0x40000000
    assert ptss.MOTION_DTYPE.itemsize == 16 and ptss.MOTION_DTYPE.fields["surface"][1] == 12 and ptss.MOTION_DTYPE.fields["prevPoint"][1] == 0
    assert ptss.device_lib().ptss_version() == 300


def test_argument_checks_without_a_device():
    """Null pointers, misaligned buffers, parameters out of range and aliased histories are answered on the host. (The range check
    of ptss_render_features_motion reads the context's triangle count: tests/test_gpu_motion.py.)"""
    L = ptss.device_lib()
    buf, other = (C.c_float * 64)(), (C.c_float * 64)()
    ctx = C.c_void_p(1)   # never dereferenced: every call below fails before the context is looked at
    assert C.addressof(buf) % 16 == 0 and C.addressof(other) % 16 == 0
    assert L.ptss_render_features_motion(None, buf, 0, 1, buf, other, None) == -1
    assert L.ptss_render_features_motion(ctx, buf, 0, 1, None, other, None) == -1
    assert L.ptss_render_features_motion(ctx, buf, 0, 1, buf, None, None) == -1
    assert L.ptss_render_features_motion(ctx, None, 0, 1, buf, other, None) == -1
    assert b"dev_triangles_prev" in L.ptss_last_error_detail()
    assert L.ptss_render_features_motion(ctx, buf, 0, 1, buf, C.c_void_p(C.addressof(other) + 4), None) == -1
    assert L.ptss_render_features_motion(ctx, C.c_void_p(C.addressof(buf) + 2), 0, 1, buf, other, None) == -1

    cam = ptss.default_camera()
    good = params()

    def call(ctx=ctx, now=buf, motion=buf, cam=cam, fprev=buf, hprev=buf, p=good, out=other):
        return L.ptss_reproject_motion(ctx, now, motion, C.byref(cam) if cam is not None else None, fprev, hprev,
                                       C.byref(p) if p is not None else None, out, None)

    assert call(ctx=None) == -1
    assert call(now=None) == -1
    assert call(motion=None) == -1
    assert call(motion=None, hprev=None, fprev=None, cam=None) == -1   # required with or without a history
    assert call(out=None) == -1
    assert call(p=None) == -1
    assert call(cam=None) == -1 and call(fprev=None) == -1
    assert call(out=buf) == -1
    assert b"dev_history_prev" in L.ptss_last_error_detail()
    assert call(motion=C.c_void_p(C.addressof(buf) + 4)) == -1
    bad = params()
    bad.structSize += 4
    assert call(p=bad) == -1
    for kw in BAD_PARAMS:
        assert call(p=params(**kw)) == -1, kw
        assert call(hprev=None, p=params(**kw)) == -1, kw


def test_probe_argument_checks():
    Hh = ptss.host_lib()
    acc = np.zeros(12, dtype=np.uint32)
    feat = np.zeros(4, dtype=ptss.FEATURE_DTYPE)
    mot = np.zeros(4, dtype=ptss.MOTION_DTYPE)
    hist, out = np.ones(4, dtype=ptss.HISTORY_DTYPE), np.zeros(4, dtype=ptss.HISTORY_DTYPE)
    cam = ptss.default_camera()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    a, f, m, h, o = acc.ctypes.data_as(C.POINTER(C.c_uint32)), vp(feat), vp(mot), vp(hist), vp(out)
    good = params()

    def call(a=a, n=1, now=cam, prev=cam, w=2, fnow=f, motion=m, fprev=f, hprev=h, p=good, out=o):
        return Hh.ptss_probe_reproject_motion(a, 1.0, n, C.byref(now) if now is not None else None, C.byref(prev) if prev is not None else None,
                                              w, 2, fnow, motion, fprev, hprev, C.byref(p) if p is not None else None, out)

    assert call() == 0
    assert call(prev=None, fprev=None, hprev=None) == 0   # no history
    for kw in (dict(a=None), dict(now=None), dict(fnow=None), dict(motion=None), dict(out=None), dict(p=None), dict(w=0), dict(n=-1),
               dict(prev=None), dict(fprev=None), dict(out=h), dict(motion=None, prev=None, fprev=None, hprev=None)):
        assert call(**kw) < 0, kw
    for kw in BAD_PARAMS:
        assert call(p=params(**kw)) < 0, kw

    rays = np.zeros((3, 8), dtype=np.float32)
    hits = np.zeros(3, dtype=ptss.HIT_DTYPE)
    tri = np.zeros(5, dtype=ptss.TRIANGLE_DTYPE)
    rows = np.zeros(3, dtype=ptss.MOTION_DTYPE)

    def motion(r=vp(rays), h=vp(hits), n=3, t=vp(tri), first=2, count=5, T=10, out=vp(rows)):
        return Hh.ptss_probe_motion(r, h, n, t, first, count, T, out)

    assert motion() == 0
    assert motion(t=None, first=0, count=0, T=0) == 0        # nothing moved
    assert motion(r=None, h=None, out=None, n=0) == 0        # no rows
    assert motion(first=5, count=5, T=10) == 0               # the last triangles
    for kw in (dict(r=None), dict(h=None), dict(out=None), dict(t=None), dict(first=6), dict(first=10), dict(count=11, first=0), dict(T=0),
               dict(first=2 ** 40)):
        assert motion(**kw) < 0, kw


# ---- csrc/ptmotion.h against float64 ----------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd in
    float64 (TwoSum gives its error), and 53 bits >= 2 * 24 + 2 make the final rounding to float32 the single rounding of the
    exact value. Finite operands."""
    a, b, c = np.broadcast_arrays(*(np.atleast_1d(np.asarray(x, dtype=np.float32)).astype(np.float64) for x in (a, b, c)))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.uint64).copy()
    inexact = err != 0
    towards_zero = inexact & ((err < 0) == (s > 0)) & (s != 0)   # |exact| < |s|: truncate by one step
    bits[towards_zero] -= np.uint64(1)
    bits[inexact] |= np.uint64(1)
    return bits.view(np.float64).astype(np.float32)


def test_fma32_is_a_single_rounding():
    a = np.array([1 + 2.0 ** -23, 3.0, 1e20, 1.0], dtype=np.float32)
    b = np.array([1 + 2.0 ** -23, 1.0 / 3.0, 1e-20, 2.0 ** -24], dtype=np.float32)
    c = np.array([-1.0, -1.0, 2.0 ** -30, 1.0], dtype=np.float32)
    got = fma32(a, b, c)
    assert got[0] == np.float32(2.0 ** -22 + 2.0 ** -46)                    # a float32 product would have lost the last term
    assert got[1] == np.float32(float(np.float32(3.0)) * float(np.float32(1.0 / 3.0)) - 1.0)
    assert got[3] == np.float32(1.0)                                        # an exact tie goes to even
    assert fma32(np.float32(1.0), np.float32(2.0 ** -24), np.float32(1.0 + 2.0 ** -23)) == np.float32(1.0 + 2.0 ** -22)


def random_motion_inputs(seed, n=4000, T=97, first=13, count=61):
    """Rays, hits and a previous table: every kind of row, triangles on both sides of and inside [first, first + count), weights inside
    and slightly outside the triangle, magnitudes from 1e-3 to just under 2^40, degenerate previous triangles and refused records."""
    rng = np.random.default_rng(seed)
    scale = (2.0 ** rng.uniform(-10, 39.9, size=(count, 1))).astype(np.float32)
    prev = np.zeros(count, dtype=ptss.TRIANGLE_DTYPE)
    for name in ("vertex0", "vertex1", "vertex2"):
        prev[name] = (rng.uniform(-1, 1, size=(count, 3)) * scale).astype(np.float32)
    prev["vertex0"][0] = prev["vertex1"][0] = prev["vertex2"][0]             # a point
    prev["vertex2"][1] = prev["vertex1"][1]                                  # a segment
    prev["vertex1"][2] = np.float32(2.0 ** 40)                               # the largest accepted coordinate
    prev["vertex0"][3] = np.float32(-2.0 ** 40)
    prev["vertex2"][4] = (np.float32(0.99 * 2.0 ** 40), np.float32(-0.999 * 2.0 ** 40), np.float32(2.0 ** 39))
    refused = {5: ("vertex0", 0, np.nan), 6: ("vertex1", 2, np.inf), 7: ("vertex2", 1, -np.inf),
               8: ("vertex2", 0, np.nextafter(np.float32(2.0 ** 40), np.float32(np.inf))), 9: ("vertex0", 1, -3e38)}
    for k, (name, axis, value) in refused.items():
        prev[name][k, axis] = value
    prev["normal0"] = np.nan                                                 # never read
    prev["materialIdx"] = -7
    hits = np.zeros(n, dtype=ptss.HIT_DTYPE)
    hits["kind"] = rng.integers(0, 3, size=n)
    hits["primitive"] = rng.integers(0, T, size=n)
    hits["primitive"][:count] = first + np.arange(count)                     # every record once, as a triangle
    hits["kind"][:count] = 2
    hits["primitive"][count:count + 4] = (first - 1, first + count, 0, T - 1)
    hits["kind"][count:count + 4] = 2
    hits["distance"] = (2.0 ** rng.uniform(-8, 30, size=n)).astype(np.float32)
    w1 = rng.uniform(0, 1, size=n)
    w2 = rng.uniform(0, 1, size=n) * (1 - w1)
    hits["w1"], hits["w2"] = w1, w2
    edge = rng.permutation(n)[:200]
    hits["w1"][edge] += rng.uniform(-1e-6, 1e-6, size=200).astype(np.float32)   # what a hit on an edge carries
    hits["w2"][edge[:50]] = 0
    hits["point"], hits["normal"], hits["materialIdx"] = np.nan, np.nan, 3    # never read
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.uniform(-50, 50, size=(n, 3))
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 3] = np.inf
    return rays, hits, prev, first, T, set(refused)


def motion_tolerance(v0, e1, e2, w1, w2):
    """fma(e2', w2, fma(e1', w1, v0')) with e' = fl(v' - v0') is three fused operations per component behind one subtraction each,
    every one within u = 2^-24 relative of its exact result: the subtractions contribute u |e1| |w1| + u |e2| |w2|, the inner fma
    u (|v0| + |e1| |w1|) and the outer one u (|v0| + |e1| |w1| + |e2| |w2|), second-order terms aside. With M = max(1, |w1|, |w2|)
    that is at most u (2 |v0| + 3 M |e1| + 2 M |e2|) <= 3 u M (|v0| + |e1| + |e2|); asserted: 4 u M (|v0| + |e1| + |e2|)."""
    big = np.maximum(1.0, np.maximum(np.abs(w1), np.abs(w2)))[:, None]
    return 4 * 2.0 ** -24 * big * (np.abs(v0) + np.abs(e1) + np.abs(e2))


@pytest.mark.parametrize("seed", [1, 2])
def test_probe_motion_against_float64(seed):
    rays, hits, prev, first, T, refused = random_motion_inputs(seed)
    got = ptss.probe_motion(rays, hits, prev, first=first, num_triangles=T)
    kind, prim = hits["kind"], hits["primitive"]
    miss = kind == 0
    tri = kind == 2
    in_range = tri & (prim >= first) & (prim < first + len(prev))
    record = np.where(in_range, prim - first, 0)
    vertices = np.stack([prev["vertex0"], prev["vertex1"], prev["vertex2"]], axis=1).astype(np.float64)   # (count, 3, 3)
    accepted = (np.abs(vertices) <= 2.0 ** 40).all(axis=(1, 2))                                          # false for NaN
    assert set(np.flatnonzero(~accepted)) == refused
    moved = in_range & accepted[record]
    assert moved.sum() > 500 and (in_range & ~moved).sum() >= len(refused) and (tri & ~in_range).sum() > 100 and (kind == 1).sum() > 100
    # surface
    want_surface = np.where(miss, -1, np.where(tri, SURFACE_TRIANGLE | prim, prim))
    assert np.array_equal(got["surface"], want_surface)
    # misses and static rows: exactly
    assert not got["prevPoint"][miss].any()
    static = ~miss & ~moved
    want_static = fma32(rays[:, 4:7], hits["distance"][:, None], rays[:, 0:3])
    assert got["prevPoint"][static].tobytes() == want_static[static].tobytes()
    # moved rows: float64 from the float32 vertices, within the derived bound
    v0, v1, v2 = (vertices[record[moved], k] for k in range(3))
    w1, w2 = hits["w1"][moved].astype(np.float64), hits["w2"][moved].astype(np.float64)
    want = v0 + (v1 - v0) * w1[:, None] + (v2 - v0) * w2[:, None]
    diff = np.abs(got["prevPoint"][moved].astype(np.float64) - want)
    bound = motion_tolerance(v0, v1 - v0, v2 - v0, w1, w2)
    worst = float((diff / np.maximum(bound, 1e-300)).max())
    print(f"seed {seed}: {int(moved.sum())} moved rows, largest |host - float64| / bound {worst:.3f}")
    assert (diff <= bound).all()
    # a degenerate previous triangle is its point
    point = moved & (prim == first)
    assert point.any() and (got["prevPoint"][point] == prev["vertex0"][0]).all()
    # count = 0: every hit is static
    none = ptss.probe_motion(rays, hits, None)
    assert np.array_equal(none["surface"], want_surface)
    assert none["prevPoint"][~miss].tobytes() == want_static[~miss].tobytes() and not none["prevPoint"][miss].any()


# ---- nothing moved: ptss_probe_reproject_motion is ptss_probe_reproject ------------------------------------------------------------
def static_motion(keys, features):
    """The rows ptss_render_features_motion writes for these features when count = 0, through the probe."""
    rays = ptss.camera_rays(camera(keys), W, H)
    hits = np.zeros(W * H, dtype=ptss.HIT_DTYPE)
    hit = features["materialIdx"] >= 0
    hits["kind"] = np.where(hit, 1, 0)
    hits["primitive"] = np.where(hit, features["materialIdx"], -1)
    hits["distance"] = features["depth"]
    return ptss.probe_motion(rays, hits, None)


@pytest.mark.parametrize("keys", ["", "df", "wg"])
@pytest.mark.parametrize("name", ["planes", "sphere", "floor"])
def test_static_motion_is_the_identity(name, keys):
    f_prev, f_now = features_of(name, ""), features_of(name, keys)
    motion = static_motion(keys, f_now)
    assert ((motion["surface"] >= 0) == (f_now["materialIdx"] >= 0)).all()
    for n, seed in ((4, 7), (1, 8)):
        accum = noisy_accum(f_now, n, seed)
        hist = noisy_history(f_prev, seed + 1)
        inv = np.float32(1.0) / np.float32(n)
        want = ptss.probe_reproject(accum, inv, n, camera(keys), camera(""), W, H, f_now, f_prev, hist)
        got = ptss.probe_reproject_motion(accum, inv, n, camera(keys), camera(""), W, H, f_now, motion, f_prev, hist)
        assert got.tobytes() == want.tobytes(), (name, keys, n)
        assert (want["weight"] > n).sum() > 0.3 * W * H
        none = ptss.probe_reproject_motion(accum, inv, n, camera(keys), None, W, H, f_now, motion, None, None)
        assert none.tobytes() == ptss.probe_reproject(accum, inv, n, camera(keys), None, W, H, f_now, None, None).tobytes()


# ---- a moving quad before a floor, in float64 ---------------------------------------------------------------------------------------
QUAD_CENTRE = np.array([0.1, 0.3, -4.0])
QUAD_HALF = (1.7, 1.1)
QUAD_CELL = 0.55   # the quad is textured by material: a checker of materials 1 and 2 in its own coordinates
FLOOR = (np.array([0.0, 1.0, 0.0]), -1.0)


def pose(shift=0.0, turn_degrees=0.0):
    """(R, c): the quad's frame (columns: its u, v and normal) and centre; a turn about the vertical axis through the centre."""
    a = np.radians(turn_degrees)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return R, QUAD_CENTRE + np.array([shift, 0.0, 0.0])


POSES = {"rest": pose(), "shift": pose(shift=0.31), "turn": pose(turn_degrees=4.0)}   # 0.31 = 2.48 pixels of 64 at depth 4, fov 90


def quad_scene(keys, pose_now, pose_prev):
    """Features of the quad at pose_now before the floor, seen through camera(keys), and the motion rows towards pose_prev: the
    point with the same coordinates in the quad's own frame; the floor stands still."""
    o, d = rays_of(keys)
    R, c = pose_now
    n = R[:, 2]
    tq = plane_hit(o, d, n, float(c @ n))
    with np.errstate(invalid="ignore"):
        local = (o + d * np.where(np.isinf(tq), 0.0, tq)[:, None] - c) @ R          # coordinates along u, v, n
    on_quad = np.isfinite(tq) & (np.abs(local[:, 0]) <= QUAD_HALF[0]) & (np.abs(local[:, 1]) <= QUAD_HALF[1])
    tq = np.where(on_quad, tq, np.inf)
    tf = plane_hit(o, d, *FLOOR)
    depth = np.minimum(tq, tf)
    quad = on_quad & (tq <= tf)
    checker = (np.floor((local[:, 0] + QUAD_HALF[0]) / QUAD_CELL) + np.floor((local[:, 1] + QUAD_HALF[1]) / QUAD_CELL)).astype(np.int64) % 2
    material = np.where(np.isinf(depth), -1, np.where(quad, 1 + checker, 0))
    features = pack(np.where(quad[:, None], n, FLOOR[0]), depth, material)
    Rp, cp = pose_prev
    local[:, 2] = 0.0
    with np.errstate(invalid="ignore"):
        point = np.where(quad[:, None], local @ Rp.T + cp, o + d * np.where(np.isinf(depth), 0.0, depth)[:, None])
    motion = np.zeros(W * H, dtype=ptss.MOTION_DTYPE)
    motion["prevPoint"] = np.where((material >= 0)[:, None], point, 0.0)
    motion["surface"] = np.where(material < 0, -1, np.where(quad, SURFACE_TRIANGLE | checker, 0))
    return features, motion, quad


def model(accum, inverse_ticks, n, keys_now, cam_prev, f_now, motion_now, f_prev, hist, p):
    """§3.19 in float64 numpy with §3.20's point: for a hit v = prevPoint - o_prev. -> colour (N, 3), weight (N,), near-tie mask,
    history weight w."""
    N = W * H
    c = accum.astype(np.float64) * float(np.float32(inverse_ticks))
    _, d = rays_of(keys_now)
    m = f_now["materialIdx"].astype(np.int64)
    hit = m >= 0
    o_prev = np.array([cam_prev.position.x, cam_prev.position.y, cam_prev.position.z], dtype=np.float64)
    q = cam_prev.rotation
    conj = np.array([-q.x, -q.y, -q.z, q.w], dtype=np.float64)
    v = np.where(hit[:, None], motion_now["prevPoint"].astype(np.float64) - o_prev, d)
    rng_ = np.linalg.norm(v, axis=1)
    l = quat_rotate(conj, v)
    s = -2.0 * np.tan(float(cam_prev.fieldOfView) / 2.0)
    front = l[:, 2] * float(cam_prev.zNear) > 0
    tie = near(l[:, 2], 0.0, np.linalg.norm(l, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        fx = (l[:, 0] / (l[:, 2] * s) + 0.5) * W - 0.5
        fy = (l[:, 1] / (l[:, 2] * s * (H / W)) + 0.5) * H - 0.5
    inside = front & (fx >= -1) & (fx < W) & (fy >= -1) & (fy < H)
    tie |= front & (near(fx, -1.0) | near(fx, float(W)) | near(fy, -1.0) | near(fy, float(H)))
    fx, fy = np.where(inside, fx, 0.0), np.where(inside, fy, 0.0)
    # (the floor is no threshold of the OUTPUT: a coordinate within rounding of an integer only moves a weight of that size between
    # two taps; snap such a coordinate so that float64 noise does not pick the other pair)
    fx = np.where(np.abs(fx - np.rint(fx)) < 1e-9, np.rint(fx), fx)
    fy = np.where(np.abs(fy - np.rint(fy)) < 1e-9, np.rint(fy), fy)
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    mp, np_, zp = f_prev["materialIdx"].astype(np.int64), f_prev["normal"].astype(np.float64), f_prev["depth"].astype(np.float64)
    hc = np.stack([hist["r"], hist["g"], hist["b"]], axis=-1).astype(np.float64)
    hw = hist["weight"].astype(np.float64)
    usable = np.isfinite(hc).all(axis=1) & np.isfinite(hw) & (hw > 0)
    normal = f_now["normal"].astype(np.float64)
    B, csum, wsum = np.zeros(N), np.zeros((N, 3)), np.zeros(N)
    lo, hi = c.copy(), c.copy()
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
            b = np.where(i, tx, 1 - tx) * np.where(j, ty, 1 - ty)
            ok = inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (b > 0)
            qi = np.where(ok, qy * W + qx, 0)
            ok &= mp[qi] == m
            with np.errstate(invalid="ignore"):
                cos = (normal * np_[qi]).sum(axis=1)
                off = np.abs(zp[qi] - rng_)
                tol = p.depthTolerance * rng_
                tie |= ok & hit & (b > 1e-6) & (near(cos, p.cosNormal) | near(off, tol))
                same = ~hit | ((cos >= p.cosNormal) & (off <= tol))
            ok &= same & usable[qi]
            B += np.where(ok, b, 0.0)
            csum += np.where(ok[:, None], b[:, None] * np.nan_to_num(hc[qi], posinf=0.0, neginf=0.0), 0.0)
            wsum += np.where(ok, b * np.nan_to_num(hw[qi], posinf=0.0), 0.0)
            lo = np.where(ok[:, None], np.minimum(lo, hc[qi]), lo)
            hi = np.where(ok[:, None], np.maximum(hi, hc[qi]), hi)
    have = B > 0   # (a lone tap of rounding-size weight stays below minCoverage: w = 0 with or without it)
    tie |= have & near(B, p.minCoverage)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(have[:, None], csum / B[:, None], c)
        w = np.where(have, np.minimum(wsum / B, p.maxHistory), 0.0)
    w = np.where(B < p.minCoverage, 0.0, w)
    total = n + w
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((w > 0)[:, None], c + (h - c) * (w / total)[:, None], c)
    return np.clip(out, lo, hi), total, tie, w


CASES = {"shift, camera fixed": ("shift", ""), "shift, camera moved": ("shift", "df"), "turn, camera fixed": ("turn", ""),
         "turn, camera moved": ("turn", "df")}


def quad_case(name, n=4, seed=17, **kw):
    to, keys = CASES[name]
    f_prev, _, _ = quad_scene("", POSES["rest"], POSES["rest"])
    f_now, motion, quad = quad_scene(keys, POSES[to], POSES["rest"])
    accum = noisy_accum(f_now, n, seed)
    hist = noisy_history(f_prev, seed + 1)
    p = params(**kw)
    inv = np.float32(1.0) / np.float32(n)
    got = ptss.probe_reproject_motion(accum, inv, n, camera(keys), camera(""), W, H, f_now, motion, f_prev, hist, p)
    stale = ptss.probe_reproject(accum, inv, n, camera(keys), camera(""), W, H, f_now, f_prev, hist, p)
    return got, model(accum, inv, n, keys, camera(""), f_now, motion, f_prev, hist, p), quad, stale, f_now


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_build_agrees_with_the_float64_model(name):
    got, (want, want_weight, tie, w), quad, stale, f_now = quad_case(name)
    left_out = float(tie.mean())
    keep = ~tie
    dc = float(np.abs(colours(got).astype(np.float64) - want)[keep].max())
    dw = float(np.abs(got["weight"].astype(np.float64) - want_weight)[keep].max())
    on_quad = float(((w > 0) & quad).sum()) / max(int(quad.sum()), 1)
    print(f"{name}: left out {100 * left_out:.2f} %, quad pixels {int(quad.sum())}, of them with history {100 * on_quad:.1f} %, all pixels with "
          f"history {int((w > 0).sum())} of {W * H}, largest |host - model| colour {dc:.3g}, weight {dw:.3g}")
    assert left_out <= MAX_LEFT_OUT
    assert quad.sum() > 0.12 * W * H and (f_now["materialIdx"] == 0).sum() > 0.15 * W * H     # both surfaces are on screen ...
    assert {1, 2} <= set(np.unique(f_now["materialIdx"][quad]))                               # ... the quad with both materials
    assert on_quad > 0.6 and (w > 0).sum() > 0.3 * W * H                                      # the case does reproject, on the quad too
    assert dc <= COLOUR_TOLERANCE and dw <= WEIGHT_TOLERANCE
    # the motion rows matter: without them (ptss_reproject on the stale history) the quad's pixels come out differently
    assert (stale.view(np.uint32).reshape(-1, 4)[quad] != got.view(np.uint32).reshape(-1, 4)[quad]).any(axis=1).mean() > 0.5


def test_a_surface_turned_too_far_loses_its_history():
    """The documented limit: the normal test compares the current normal with the previous frame's at the tap."""
    f_prev, _, _ = quad_scene("", POSES["rest"], POSES["rest"])
    far = pose(turn_degrees=30.0)   # cos 30 = 0.866 < cosNormal 0.9
    f_now, motion, quad = quad_scene("", far, POSES["rest"])
    accum = noisy_accum(f_now, 4, 3)
    hist = noisy_history(f_prev, 4, broken=False)
    got = ptss.probe_reproject_motion(accum, 0.25, 4, camera(""), camera(""), W, H, f_now, motion, f_prev, hist)
    assert quad.sum() > 200 and (got["weight"][quad] == 4).all()
    open_ = ptss.probe_reproject_motion(accum, 0.25, 4, camera(""), camera(""), W, H, f_now, motion, f_prev, hist, params(cosNormal=0.8))
    assert (open_["weight"][quad] > 4).mean() > 0.6
