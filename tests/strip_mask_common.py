"""Scenes, cameras and eye rays for the strip words of bounce 0 (csrc/ptstrip.h), shared by tests/test_strip_masks_cpu.py and
tests/test_gpu_strip_masks.py. The scenes are the ones a frustum cull gets wrong when its slacks are too small: tiny far spheres
and triangles, spheres tangent to a strip's pyramid, the camera inside a sphere and 1e-4 off one, walls seen edge-on and around
the grazing threshold, a triangle with vertices behind the camera. Not a test module."""
import ctypes as C
import math

import numpy as np

import ptss
from ptss_types import Material, PointLight, RayQuery, SceneDesc, Sphere, Triangle

STRIP = 64
# jitters of a pixel: the corners and edge midpoints of [0, 1]^2, then the centre
EDGE_JITTERS = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.0), (0.5, 1.0), (0.0, 0.5), (1.0, 0.5), (0.5, 0.5)]


def _set3(v, xyz):
    v.x, v.y, v.z = (float(t) for t in xyz)


class Holder:
    pass


def make_scene(spheres, triangles):
    """spheres: (centre3, radius); triangles: (v0, v1, v2). Two Lambert materials, one point light, a grey background."""
    mats = (Material * 2)()
    for k, m in enumerate(mats):
        _set3(m.diffuseColor, (0.8, 0.5 + 0.3 * k, 0.4))
        _set3(m.specularColor, (0.0, 0.0, 0.0))
        _set3(m.absorption, (0.0, 0.0, 0.0))
        _set3(m.emmitance, (0.1 * k, 0.0, 0.05))
        m.specularExponent, m.indexOfRefraction = 1.0, 1.0
        m.diffAvg, m.specAvg, m.refrAvg, m.roughness = 0.7, 0.0, 0.0, 0.5
        m.flags = bytes([0])
    ns, nt = len(spheres), len(triangles)
    sph = (Sphere * max(ns, 1))()
    for i, (c, r) in enumerate(spheres):
        _set3(sph[i].position, c)
        sph[i].radius, sph[i].materialIdx = float(r), i % 2
    tri = (Triangle * max(nt, 1))()
    for i, (a, b, c) in enumerate(triangles):
        a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
        _set3(tri[i].vertex0, a)
        _set3(tri[i].vertex1, b)
        _set3(tri[i].vertex2, c)
        n = np.cross(b - a, c - a)
        n = n / max(np.linalg.norm(n), 1e-30)
        for v in (tri[i].normal0, tri[i].normal1, tri[i].normal2):
            _set3(v, n)
        tri[i].materialIdx = (i + 1) % 2
    pl = (PointLight * 1)()
    _set3(pl[0].position, (0.5, 3.0, -2.0))
    _set3(pl[0].power, (40.0, 40.0, 40.0))
    d = SceneDesc()
    d.spheres, d.numSpheres = (sph if ns else None), ns
    d.triangles, d.numTriangles = (tri if nt else None), nt
    d.materials, d.numMaterials = mats, 2
    d.pointLights, d.numPointLights = pl, 1
    d.areaLights, d.numAreaLights = None, 0
    _set3(d.defaultColor, (0.2, 0.3, 0.4))
    h = Holder()
    h.desc, h.keep = d, (sph, tri, mats, pl)
    return h


def quad(p, a, b):
    """two triangles over the parallelogram p, p + a, p + a + b, p + b"""
    p, a, b = (np.asarray(v, dtype=np.float64) for v in (p, a, b))
    return [(p, p + a, p + b), (p + a + b, p + b, p + a)]


def camera(position=(0.0, 0.0, 0.0), keys="", fov=None, z_near=None):
    cam = ptss.default_camera()
    for k in keys:
        ptss.move_camera(cam, k)
    _set3(cam.position, position)   # (after the moves: the keys w a s d move the position too)
    if fov is not None:
        cam.fieldOfView = fov
    if z_near is not None:
        cam.zNear = z_near
    return cam


def pixel_direction(w, h, x, y):
    """the default camera's eye direction through frame position (x, y) (fractional pixels), in double: looks along -z"""
    s = -2.0 * math.tan(0.5 * ptss.default_camera().fieldOfView)
    u, v = (x / w - 0.5) * s, (y / h - 0.5) * s * (h / w)
    d = -np.array([u, v, 1.0])
    return d / np.linalg.norm(d)


# ---- the adversarial scenes: (name, scene, camera); all for the default camera's pose unless the camera says otherwise, and
# placed for a frame of w x h pixels (the tangent and tiny primitives sit at pixel boundaries of THAT frame) ----------------------
def tiny_scene(w, h):
    """spheres of radius 1e-3 at distances 10 .. 100 and triangles a thousandth of their distance, each on a pixel corner"""
    sph, tri = [], []
    for k, dist in enumerate((10.0, 30.0, 100.0)):
        for x, y in ((w * 0.25, h * 0.5), (w - 1.0, 1.0), (min(64.0, w - 2.0), h - 2.0)):
            sph.append((pixel_direction(w, h, x + k, y) * dist, 1e-3))
    for k, dist in enumerate((20.0, 50.0)):
        for x, y in ((w * 0.6, h * 0.25), (1.0, h - 1.0)):
            c = pixel_direction(w, h, x + k, y) * dist
            e = dist * 1e-3
            tri.append((c, c + np.array([e, 0.0, 0.0]), c + np.array([0.0, e, 0.3 * e])))
    tri += quad((-40.0, -40.0, -120.0), (80.0, 0.0, 0.0), (0.0, 80.0, 0.0))   # a far wall behind everything
    return make_scene(sph, tri)


def tangent_scene(w, h):
    """spheres whose silhouette touches a row boundary, a column boundary at a strip's end, or the frame's edge from outside"""
    sph = []
    for dist, ang in ((3.0, 0.02), (8.0, 0.05), (25.0, 0.004)):
        for x, y, dx, dy in ((w * 0.5, float(h // 2), 0.0, 1.0), (min(64.0, w - 1.0), h * 0.5, 1.0, 0.0), (w * 0.3, 0.0, 0.0, -1.0),
                             (float(w), h * 0.7, 1.0, 0.0)):
            b = pixel_direction(w, h, x, y)                       # a direction ON the boundary
            n = pixel_direction(w, h, x + dx, y + dy) - b         # ... and the side the sphere lies on
            n = n - b * np.dot(n, b)
            n = n / np.linalg.norm(n)
            sph.append(((b * math.cos(ang) + n * math.sin(ang)) * dist, dist * math.sin(ang)))
    return make_scene(sph, quad((-9.0, -9.0, -30.0), (18.0, 0.0, 0.0), (0.0, 18.0, 0.0)))


def inside_scene():
    """the camera inside one sphere, 1e-4 inside another's surface and 1e-4 outside a third's; more spheres beyond"""
    sph = [((0.2, -0.1, 0.3), 6.0), ((0.0, 0.0, -(1.5 - 1e-4)), 1.5), ((0.0, 0.7 + 1e-4, 0.0), 0.7), ((-(0.4 + 1e-4), 0.0, 0.0), 0.4),
           ((0.5, 0.3, -3.0), 0.6), ((-1.0, -0.5, -4.0), 0.8), ((0.0, 0.0, 2.0), 0.5)]
    return make_scene(sph, quad((-3.0, -3.0, -5.0), (6.0, 0.0, 0.0), (0.0, 6.0, 0.0)))


def grazing_scene():
    """floors seen edge-on (through the camera) and at a few angles around the grazing threshold, walls along the view axis, and
    triangles with vertices behind the camera"""
    tri = []
    for k, height in enumerate((0.0, 1e-4, 3e-3, 2e-2, 0.15)):
        tri += quad((-2.0 + 0.7 * k, -height, -1.0), (0.6, 0.0, 0.0), (0.0, 0.0, -40.0))
    tri += quad((1.9, -1.0, -0.5), (0.002, 0.0, -30.0), (0.0, 2.0, 0.0))          # a wall nearly along the view axis
    tri += quad((-1.0, 0.8, -0.5), (2.0, 0.0, 0.0), (0.0, 0.004, -25.0))          # a ceiling nearly along it
    tri.append(((-3.0, -2.0, 5.0), (3.0, -2.0, 5.0), (0.0, 1.5, -6.0)))           # two vertices behind the camera
    tri.append(((0.5, 0.5, 4.0), (0.9, 0.2, -7.0), (0.2, 0.9, -7.0)))             # one vertex behind it
    tri.append(((-4.0, 2.0, 3.0), (-3.0, 2.0, 1.0), (-3.5, 3.0, 2.0)))            # wholly behind it
    sph = [((0.0, 0.0, 3.0), 1.0), ((0.4, 0.2, -6.0), 0.5)]
    return make_scene(sph, tri)


def adversarial_cases(w, h):
    """(name, scene, camera) — every one inside the cull's domain (ptss_probe_strip_masks reports enabled)"""
    return [("tiny", tiny_scene(w, h), camera()), ("tangent", tangent_scene(w, h), camera()), ("inside", inside_scene(), camera()),
            ("grazing", grazing_scene(), camera()), ("grazing-turned", grazing_scene(), camera((0.3, 0.002, -0.4), keys="hhgq")),
            ("inside-turned", inside_scene(), camera((0.1, 0.0, 0.05), keys="ft", fov=1.1, z_near=0.37))]


# ---- pixels and rays ---------------------------------------------------------------------------------------------------------------
def pixel_order(width, rank, world, band_rows, local):
    """local pixel -> (x, frame row): the tile's pixel order, stated independently of csrc/ptlocate.h"""
    local = np.asarray(local, dtype=np.int64)
    x, ly = local % width, local // width
    return x, ((ly // band_rows) * world + rank) * band_rows + ly % band_rows


def eye_rays(cam, w, h, xs, ys, jitters):
    """(n, 6) float32 {origin, direction} of the frame's own eye rays (ptss_camera_ray: bounce 0's operations on the host)"""
    out = np.empty((len(xs), 6), dtype=np.float32)
    q = RayQuery()
    fn, ref_cam, ref_q = ptss.host_lib().ptss_camera_ray, C.byref(cam), C.byref(q)
    buf = np.frombuffer((C.c_float * 8).from_buffer(q), dtype=np.float32)
    for i in range(len(xs)):
        assert fn(ref_cam, w, h, int(xs[i]), int(ys[i]), float(jitters[i][0]), float(jitters[i][1]), ref_q) == 0
        out[i, 0:3], out[i, 3:6] = buf[0:3], buf[4:7]
    return out


def strip_rays(cam, w, h, band_rows, rank, world, rng, strips=None, lanes_per_strip=None, random_jitters=3, dense=()):
    """Eye rays of the rank's local pixels with the strip each belongs to: (rays (n, 6), strip (n,)). strips: which strips (None: all);
    lanes_per_strip: None = every pixel, else the strip's first and last pixel and that many random ones; every chosen pixel gets the
    corner, edge and centre jitters and random_jitters random ones. dense: frame positions (x, y) around which the 3 x 3 pixels get a
    24 x 24 grid of jitters each (tiny primitives)."""
    rows = len(ptss.tile_rows(h, band_rows, rank, world))
    num_pixels = w * rows
    num_strips = (num_pixels + STRIP - 1) // STRIP
    local = []
    for s in (range(num_strips) if strips is None else strips):
        first, last = s * STRIP, min(s * STRIP + STRIP, num_pixels) - 1
        if lanes_per_strip is None:
            local += list(range(first, last + 1))
        else:
            local += [first, last] + [int(v) for v in rng.integers(first, last + 1, size=lanes_per_strip)]
    local = np.array(local, dtype=np.int64)
    x, gy = pixel_order(w, rank, world, band_rows, local)
    xs, ys, js, st = [], [], [], []
    for i in range(len(local)):
        for j in EDGE_JITTERS + [tuple(v) for v in rng.random((random_jitters, 2))]:
            xs.append(x[i]); ys.append(gy[i]); js.append(j); st.append(local[i] // STRIP)
    if not dense:
        return eye_rays(cam, w, h, xs, ys, js), np.array(st, dtype=np.int64)
    # dense grids: only pixels this rank owns
    all_x, all_gy = pixel_order(w, rank, world, band_rows, np.arange(num_pixels))
    where = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(all_x, all_gy))}
    grid = [(a, b) for a in np.linspace(0.0, 1.0, 24) for b in np.linspace(0.0, 1.0, 24)]
    for (cx, cy) in dense:
        for px in range(int(math.floor(cx)) - 1, int(math.floor(cx)) + 2):
            for py in range(int(math.floor(cy)) - 1, int(math.floor(cy)) + 2):
                k = where.get((px, py))
                if k is None:
                    continue
                for j in grid:
                    xs.append(px); ys.append(py); js.append(j); st.append(k // STRIP)
    return eye_rays(cam, w, h, xs, ys, js), np.array(st, dtype=np.int64)


def project(frame, point):
    """frame position (x, y) of a world point for the DEFAULT camera pose (frame = (w, h))"""
    w, h = frame
    s = -2.0 * math.tan(0.5 * ptss.default_camera().fieldOfView)
    p = np.asarray(point, dtype=np.float64)
    u, v = p[0] / p[2], p[1] / p[2]     # p = -(u, v, 1) t with t = -p.z
    return (u / s + 0.5) * w, (v / (s * h / w) + 0.5) * h
