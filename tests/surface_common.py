"""The models and the cases shared by tests/test_surface_cpu.py, tests/test_gpu_surface.py and tests/test_gpu_surface_main.py (rays from
surface points, the atlas, the gutter fill: ptss_generate_rays_surface, ptss_dilate_linear).

model_surface_rays restates csrc/ptsurface.h operation by operation in numpy float32 scalars, with fma rounded once from rationals
(linreproject_common.f32_fma) and ptm::sincos taken through ptss_probe_math; the streams advance through ptss_probe_rng_draw, which
tests/test_film_cpu.py pins to the oracle. model_dilate restates the gutter fill in Python integers. Neither shares code with the header,
and both must agree with the probes byte for byte."""
import ctypes as C

import numpy as np

import ptss
from film_common import advance
from linreproject_common import f32_fma

F32 = np.float32
PI = F32(3.14159265358979323846)
TWO_PI = F32(2) * PI
RAY_BUMP = F32(1e-4)
TRIANGLE = ptss.SURFACE_TRIANGLE
MASK64, MASK32 = (1 << 64) - 1, (1 << 32) - 1
NS = (1, 63, 64, 65, 255, 256, 257, 1025)   # the batch sizes of the GPU tests: around a wave, a workgroup, several workgroups


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def first_difference(a, b):
    a, b = words(a), words(b)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist(), len(bad))


def fma(a, b, c):
    return f32_fma(F32(a), F32(b), F32(c))


def sincos(x):
    """(ptm::sincos(x)) through the host probe: the model does not restate the polynomial."""
    x = np.array([x], dtype=np.float32)
    s, c = np.empty_like(x), np.empty_like(x)
    f32p = C.POINTER(C.c_float)
    assert ptss.host_lib().ptss_probe_math(0, x.ctypes.data_as(f32p), None, s.ctypes.data_as(f32p), 1) == 0
    assert ptss.host_lib().ptss_probe_math(1, x.ctypes.data_as(f32p), None, c.ctypes.data_as(f32p), 1) == 0
    return s[0], c[0]


def dot(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], F32(a[0]) * F32(b[0])))


def normalize(v):
    inv = F32(1) / np.sqrt(dot(v, v))   # the host's sqrt_rcp: the IEEE root, then 1 / root
    return [F32(c) * inv for c in v]


def madd(v, s, o):
    return [fma(v[k], s, o[k]) for k in range(3)]


def vec(record):
    return [F32(c) for c in record]


def model_point_accepted(pt, num_triangles, num_spheres):
    surface, a, b, flags = int(pt["surface"]), F32(pt["a"]), F32(pt["b"]), int(pt["flags"])
    if surface < 0 or flags & ~ptss.SURFACE_BACK:
        return False
    if surface & TRIANGLE:
        return (surface & ~TRIANGLE) < num_triangles and bool(a >= 0) and bool(b >= 0) and bool(F32(a + b) <= F32(1))
    return surface < num_spheres and bool(F32(0) <= a <= F32(1)) and bool(F32(0) <= b <= F32(1))


def model_surfel(pt, triangles, spheres):
    """(point, unit normal as flipped, materialIdx, kind, primitive, w1, w2) of an accepted point."""
    surface, a, b = int(pt["surface"]), F32(pt["a"]), F32(pt["b"])
    if surface & TRIANGLE:
        t = triangles[surface & ~TRIANGLE]
        v0, v1, v2 = vec(t["vertex0"]), vec(t["vertex1"]), vec(t["vertex2"])
        e1, e2 = [v1[k] - v0[k] for k in range(3)], [v2[k] - v0[k] for k in range(3)]
        point = madd(e2, b, madd(e1, a, v0))
        w0 = F32(1) - (a + b)
        n0, n1, n2 = vec(t["normal0"]), vec(t["normal1"]), vec(t["normal2"])
        n = normalize([(n0[k] * w0 + n1[k] * a) + n2[k] * b for k in range(3)])
        hit = (int(t["materialIdx"]), 2, surface & ~TRIANGLE, a, b)
    else:
        s = spheres[surface]
        lon, lat = (a - F32(0.5)) * TWO_PI, (b - F32(0.5)) * PI
        (sl, cl), (se, ce) = sincos(lon), sincos(lat)
        n = [sl * ce, se, -(cl * ce)]
        r = np.sqrt(F32(s["radius"]) * F32(s["radius"]))
        point = madd(n, r, vec(s["position"]))
        hit = (int(s["materialIdx"]), 1, surface, F32(0), F32(0))
    if int(pt["flags"]) & ptss.SURFACE_BACK:
        n = [-c for c in n]
    return (point, n) + hit


def model_about_normal(n, lx, ly, lz):
    s = F32(-1.0) if np.signbit(n[2]) else F32(1.0)
    q = -(F32(1) / (s + n[2]))
    c = (n[0] * n[1]) * q
    t = [fma(s * n[0], n[0] * q, F32(1)), s * c, -(s * n[0])]
    b = [c, fma(n[1], n[1] * q, s), -n[1]]
    return madd(b, lz, madd(n, ly, [t[k] * lx for k in range(3)]))


def model_ray(point, n, mode, max_distance, u1, u2):
    v = n
    if mode == ptss.SURFACE_COSINE:
        azimuth = F32(u1) * F32(2) * PI
        y = np.sqrt(F32(u2))
        A = np.sqrt(F32(1) - y * y)
        sn, cs = sincos(azimuth)
        v = model_about_normal(n, A * cs, y, A * sn)
    origin = [point[k] + RAY_BUMP * n[k] for k in range(3)]
    return origin + [F32(max_distance)] + normalize(v) + [F32(0)]


def model_surface_rays(triangles, spheres, points, rng, params, first_point=0, index=None, rays=None, surfels=None):
    """ptss_probe_surface_rays in the terms above -> (rays (N, 8) float32, streams (N, 6) uint32, surfels (N, 12) float32, rejected).
    rays / surfels: the content beforehand."""
    s = np.array(words(rng), dtype=np.uint32)
    n = len(s)
    out = np.zeros((n, 8), dtype=np.float32) if rays is None else np.array(words(rays).view(np.float32))
    sur = np.zeros((n, 12), dtype=np.float32) if surfels is None else np.array(words(surfels).view(np.float32))
    T, S = (len(triangles) if triangles is not None else 0), (len(spheres) if spheres is not None else 0)
    rejected = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            p = int(index[i]) if index is not None else first_point + i
            if p >= len(points) or not model_point_accepted(points[p], T, S):
                rejected += 1
                continue
            point, normal, material, kind, prim, w1, w2 = model_surfel(points[p], triangles, spheres)
            u = (F32(0), F32(0))
            if params.mode == ptss.SURFACE_COSINE:
                s[i], u = advance(s[i], 2)
            out[i] = model_ray(point, normal, params.mode, params.maxDistance, u[0], u[1])
            sur[i, 0:3], sur[i, 3], sur[i, 4:7] = point, 0.0, normal
            sur[i, 7:10] = np.array([material, kind, prim], dtype=np.int32).view(np.float32)
            sur[i, 10:12] = w1, w2
    return out, s, sur, rejected


# ---- points --------------------------------------------------------------------------------------------------------------------------
def make_points(rows):
    pts = np.zeros(len(rows), dtype=ptss.SURFACE_POINT_DTYPE)
    for k, (surface, a, b, flags) in enumerate(rows):
        pts[k] = (surface, a, b, flags)
    return pts


def good_points(num_triangles, num_spheres, count, seed, interior=False):
    """`count` accepted points spread over both kinds of primitive and both sides; corners and edges among them unless `interior`
    (then a, b >= 0.1 and a + b <= 0.9 on triangles, away from the poles on spheres)."""
    g = np.random.default_rng(seed)
    rows = []
    for k in range(count):
        flags = int(g.integers(0, 2)) if not interior else 0
        if num_triangles and (num_spheres == 0 or k % 3 != 2):
            t = int(g.integers(0, num_triangles))
            a, b = g.uniform(0.1, 0.45, 2) if interior else g.uniform(0.0, 0.5, 2)
            if not interior and k % 16 == 0:
                a, b = ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (0.5, 0.5))[(k // 16) % 4]
            rows.append((TRIANGLE | t, a, b, flags))
        else:
            a, b = g.uniform(0.05, 0.95, 2)
            if not interior and k % 16 == 2:
                a, b = ((0.0, 0.0), (1.0, 1.0), (0.5, 0.0), (0.25, 1.0))[(k // 16) % 4]
            rows.append((int(g.integers(0, num_spheres)), a, b, flags))
    return make_points(rows)


def bad_points(num_triangles, num_spheres):
    """One of every kind of rejected point, by name."""
    nan = float("nan")
    rows = {
        "negative surface": (-1, 0.2, 0.2, 0),
        "negative triangle": (-(1 << 31) | TRIANGLE | 0, 0.2, 0.2, 0),
        "triangle beyond the scene": (TRIANGLE | num_triangles, 0.2, 0.2, 0),
        "triangle far beyond": (TRIANGLE | 0x3FFFFFFF, 0.2, 0.2, 0),
        "sphere beyond the scene": (num_spheres, 0.2, 0.2, 0),
        "sphere far beyond": (0x3FFFFFFF, 0.2, 0.2, 0),
        "reserved flag": ((TRIANGLE | 0) if num_triangles else 0, 0.2, 0.2, 2),
        "every flag": ((TRIANGLE | 0) if num_triangles else 0, 0.2, 0.2, 0xFFFFFFFF),
    }
    if num_triangles:
        rows.update({"a < 0": (TRIANGLE, -1e-6, 0.2, 0), "b < 0": (TRIANGLE, 0.2, -0.0001, 1), "a + b > 1": (TRIANGLE, 0.6, 0.4000001, 0),
                     "a NaN": (TRIANGLE, nan, 0.2, 0), "b NaN": (TRIANGLE, 0.2, nan, 0), "a inf": (TRIANGLE, float("inf"), 0.0, 0)})
    if num_spheres:
        rows.update({"sphere a < 0": (0, -0.01, 0.5, 0), "sphere a > 1": (0, 1.0000001, 0.5, 0), "sphere b < 0": (0, 0.5, -1e-9, 0),
                     "sphere b > 1": (0, 0.5, 1.5, 1), "sphere NaN": (0, nan, nan, 0)})
    names = list(rows)
    pts = np.zeros(len(names), dtype=ptss.SURFACE_POINT_DTYPE)
    for k, name in enumerate(names):
        surface, a, b, flags = rows[name]
        pts[k] = (np.array([surface & MASK32], dtype=np.uint32).view(np.int32)[0], a, b, flags)
    return names, pts


def host_states(n, seed=0x5EED):
    """n streams: curand_init(seed, i, 0) through the host probe (pinned to the oracle by tests/test_film_cpu.py)."""
    out = np.zeros((n, 6), dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    for i in range(n):
        assert ptss.host_lib().ptss_probe_rng_init(seed, i, out[i].ctypes.data_as(u32p)) == 0
    return out


def chained_states(n, draws, seed=0x5EED):
    """n states of ONE stream, each `draws` draws behind the one before: n independent pairs of uniforms from n ptss_probe_rng_draw calls."""
    out = np.zeros((n, 6), dtype=np.uint32)
    s = host_states(1, seed)[0].copy()
    u32p = C.POINTER(C.c_uint32)
    for i in range(n):
        out[i] = s
        assert ptss.host_lib().ptss_probe_rng_draw(s.ctypes.data_as(u32p), None, None, draws) == 0
    return out


# ---- the gutter fill -----------------------------------------------------------------------------------------------------------------
def model_dilate(film, width, height):
    """One pass in Python integers -> a new (P,) LINEAR_DTYPE film."""
    rows = [[int(v) for v in (e["r"], e["g"], e["b"], e["samples"], e["clamped"])] for e in film]
    out = np.zeros(len(rows), dtype=ptss.LINEAR_DTYPE)
    for y in range(height):
        for x in range(width):
            own = rows[y * width + x]
            if own[3] > 0:
                acc = own
            else:
                acc = [0, 0, 0, 0, 0]
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        nx, ny = x + dx, y + dy
                        if (dx or dy) and 0 <= nx < width and 0 <= ny < height and rows[ny * width + nx][3] > 0:
                            acc = [a + b for a, b in zip(acc, rows[ny * width + nx])]
            out[y * width + x] = (acc[0] & MASK64, acc[1] & MASK64, acc[2] & MASK64, acc[3] & MASK32, acc[4] & MASK32)
    return out


DILATE_SIZES = ((1, 1), (1, 7), (7, 1), (17, 9))
DILATE_GPU_SIZES = DILATE_SIZES + ((33, 17), (64, 8))   # the kernel's tile is 32 x 8: one tile and a column and row over, two tiles exactly


def dilate_films(width, height):
    """{name: film} for one size: empties at corners and edges, all empty, none empty, fields near 2^64 and counts near 2^32 that wrap."""
    P = width * height
    g = np.random.default_rng([width, height])

    def filled(holes):
        f = np.zeros(P, dtype=ptss.LINEAR_DTYPE)
        n = g.integers(1, 1000, P).astype(np.uint32)
        for ch in "rgb":
            f[ch] = g.integers(0, 1 << 40, P).astype(np.uint64) * n
        f["samples"], f["clamped"] = n, g.integers(0, 3, P)
        f[holes] = np.zeros(1, dtype=ptss.LINEAR_DTYPE)[0]
        return f

    x, y = np.arange(P) % width, np.arange(P) // width
    border = (x == 0) | (y == 0) | (x == width - 1) | (y == height - 1)
    films = {"empty border": filled(border), "none empty": filled(np.zeros(P, bool)), "all empty": filled(np.ones(P, bool)),
             "sparse": filled(g.random(P) < 0.7), "checker": filled((x + y) % 2 == 0)}
    wrap = filled(g.random(P) < 0.5)
    full = wrap["samples"] > 0
    wrap["r"][full] = np.uint64((1 << 64) - 3)
    wrap["g"][full] = np.uint64(1 << 63)
    wrap["samples"][full] = np.uint32((1 << 32) - 2)
    wrap["clamped"][full] = np.uint32(1 << 31)
    films["wraps"] = wrap
    return films
