"""Soundness of the mesh image's cull (csrc/ptmesh.h; derivation at packMeshBounds in csrc/ptpack.h): a leaf or
group bound may say "provably not" only for a ray that the reference's float test (Triangle::intersectRay, Primitives.h:25-83)
accepts for none of its triangles, at any distance. Checked on the host build of the very predicate the kernels evaluate
(ptss_probe_mesh_bound), against the general form of the triangle test (ptss_probe_triangle_forms, itself pinned to the oracle
here and in tests/test_triangle_forms.py), for random rays, adversarial rays (grazing with |det| swept down to just above
1e-7, hits on shared edges and vertices, limits equal to the hit distance) and origins near the eligibility bound. The same
generators run against the bound with its inflation scaled down, to show that they do find the rays such a bound loses.
No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from meshgen import icosphere

f32p = C.POINTER(C.c_float)


def general_form(tri, o, d, limit):
    """accepted (bool), dist, det of the reference's test for each (triangle, origin, direction, limit) tuple."""
    tri = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 9)
    o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
    lim = np.ascontiguousarray(np.broadcast_to(np.asarray(limit, dtype=np.float32), (len(o),)))
    n = len(o)
    cls = np.zeros(n, dtype=np.int32)
    g = np.zeros((n, 6), dtype=np.float32)
    c = np.zeros((n, 6), dtype=np.float32)
    rc = ptss.host_lib().ptss_probe_triangle_forms(tri.ctypes.data_as(f32p), o.ctypes.data_as(f32p), d.ctypes.data_as(f32p),
                                                   lim.ctypes.data_as(f32p), 0, n, cls.ctypes.data_as(C.POINTER(C.c_int)),
                                                   g.ctypes.data_as(f32p), c.ctypes.data_as(f32p))
    assert rc == 0
    return g[:, 0] == 1.0, g[:, 1], g[:, 5]


def stored(v0, v1, v2):
    """{v0, e1, e2} as the image stores a triangle (the same float subtractions)."""
    v0, v1, v2 = (np.asarray(x, dtype=np.float32) for x in (v0, v1, v2))
    return np.concatenate([v0, v1 - v0, v2 - v0], axis=-1)


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def lost(leaf, o, d, limit=np.inf, margin=1.0):
    """Rays accepted by some triangle of `leaf` that the bound built around `leaf` rejects; and how many were accepted."""
    leaf = np.asarray(leaf, dtype=np.float32).reshape(-1, 9)
    acc = np.zeros(len(o), dtype=bool)
    for t in leaf:
        a, _, _ = general_form(np.broadcast_to(t, (len(o), 9)), o, d, limit)
        acc |= a
    may, _ = ptss.probe_mesh_bound(leaf, o, d, margin)
    return int(np.count_nonzero(acc & (may == 0))), int(np.count_nonzero(acc))


def random_triangle(rng, scale):
    v0 = rng.uniform(-5, 5, 3)
    return stored(v0, v0 + rng.normal(0, scale, 3), v0 + rng.normal(0, scale, 3))


def rays_at(rng, tri, n, spread=0.3, dist=(0.5, 30)):
    """n unit rays aimed at points around the triangle (barycentric weights in [-spread, 1 + spread]) from distances in `dist`."""
    v0, e1, e2 = tri[:3].astype(np.float64), tri[3:6].astype(np.float64), tri[6:].astype(np.float64)
    b = rng.uniform(-spread, 1 + spread, (n, 2))
    target = v0 + b[:, :1] * e1 + b[:, 1:] * e2
    d = unit(rng.normal(size=(n, 3)))
    o = (target - d.astype(np.float64) * rng.uniform(*dist, (n, 1))).astype(np.float32)
    return o, d


def grazing_rays(rng, tri, n, dets, reach=(0.1, 40)):
    """Rays whose |det| = |d . (e1 x e2)| is swept through `dets`: each starts at a float origin `reach` units away, at the height
    above the plane that gives that |det|, and points at a target on the edges, at the vertices, just outside or far outside the
    triangle (where only the rounding of a flat det can make the test accept)."""
    v0, e1, e2 = tri[:3].astype(np.float64), tri[3:6].astype(np.float64), tri[6:].astype(np.float64)
    N = np.cross(e1, e2)
    nl = np.linalg.norm(N)
    nh = N / nl
    os_, ds = [], []
    for det in dets:
        w = rng.normal(size=(n, 3))
        w -= (w @ nh)[:, None] * nh
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        b = rng.choice([0.0, 1.0, 0.5, 0.25, -1e-3, 1e-3, -0.01, -0.1, -0.3, 1.1, -1.0, 2.0, -4.0], (n, 2))
        target = v0 + b[:, :1] * e1 + b[:, 1:] * e2
        L = rng.uniform(*reach, (n, 1))
        h = det * L / nl * rng.choice([-1, 1], (n, 1))
        o = (target - L * w + h * nh).astype(np.float32)
        d = unit(target - o.astype(np.float64))
        os_.append(o)
        ds.append(d)
    return np.concatenate(os_), np.concatenate(ds)


DETS = [1.0000001e-7, 1.05e-7, 1.2e-7, 2e-7, 5e-7, 1e-6, 1e-5, 1e-4]


def test_probe_agrees_with_the_oracles_triangle_test():
    rng = np.random.default_rng(1)
    hits = 0
    for _ in range(40):
        v = rng.uniform(-5, 5, (3, 3)).astype(np.float32)
        t = stored(*v)
        o, d = rays_at(rng, t, 8)
        acc, dist, _ = general_form(np.broadcast_to(t, (8, 9)), o, d, np.inf)
        for k in range(8):
            hit, out = oracle.probe_triangle(v[0], v[1], v[2], o[k], d[k])
            assert hit == bool(acc[k])
            hits += hit
    assert hits > 20


@pytest.mark.parametrize("scale", [1e-3, 0.05, 1.0, 10.0])
def test_random_rays_lose_nothing(scale):
    rng = np.random.default_rng(int(scale * 1000) + 7)
    total = 0
    for _ in range(250):   # 250 triangles x 1,000 rays per scale: a million rays over the four scales
        t = random_triangle(rng, scale)
        o, d = rays_at(rng, t, 1000)
        miss, acc = lost(t, o, d)
        assert miss == 0
        total += acc
    assert total > 10000


def icosphere_leaves(level=3, radius=1.5):
    v, f = icosphere(level)
    p = (radius * v).astype(np.float32)
    tris = np.stack([stored(p[a], p[b], p[c]) for a, b, c in f])
    return [tris[k:k + 16] for k in range(0, len(tris), 16)]


def test_leaves_of_a_mesh_with_shared_edges_lose_nothing():
    rng = np.random.default_rng(3)
    leaves = icosphere_leaves()
    total = 0
    for leaf in leaves[::4]:
        o, d = [], []
        for t in leaf:
            a, b = rays_at(rng, t, 60, spread=0.05)
            o.append(a)
            d.append(b)
            a, b = grazing_rays(rng, t, 6, DETS)
            o.append(a)
            d.append(b)
        miss, acc = lost(leaf, np.concatenate(o), np.concatenate(d))
        assert miss == 0
        total += acc
    assert total > 1000


@pytest.mark.parametrize("scale", [0.05, 1.0, 4.0])
def test_grazing_rays_down_to_the_determinant_floor_lose_nothing(scale):
    rng = np.random.default_rng(11)
    total = 0
    for _ in range(120):
        t = random_triangle(rng, scale)
        o, d = grazing_rays(rng, t, 100, DETS)
        miss, acc = lost(t, o, d)
        assert miss == 0
        total += acc
    assert total > 100


def test_limits_equal_to_the_hit_distance():
    rng = np.random.default_rng(5)
    for _ in range(100):
        t = random_triangle(rng, 1.0)
        o, d = rays_at(rng, t, 200, spread=0.0)
        acc, dist, _ = general_form(np.broadcast_to(t, (200, 9)), o, d, np.inf)
        lim = np.where(acc, dist, np.float32(1.0))
        miss, _ = lost(t, o, d, limit=lim)
        assert miss == 0


def test_origins_near_the_eligibility_bound():
    rng = np.random.default_rng(9)
    far = 2.0 ** 39
    total = 0
    for _ in range(60):
        v0 = rng.uniform(-far, far, 3)
        t = stored(v0, v0 + rng.normal(0, far / 64, 3), v0 + rng.normal(0, far / 64, 3))
        o, d = rays_at(rng, t, 300, dist=(far / 8, far / 2))
        o = np.clip(o, -far * 1.2, far * 1.2)
        assert np.all(np.sum(o.astype(np.float64) ** 2, axis=1) < 2.0 ** 80)
        miss, acc = lost(t, o, d)
        assert miss == 0
        total += acc
        o, d = grazing_rays(rng, t, 20, DETS[:4], reach=(far / 8, far / 2))
        keep = np.sum(o.astype(np.float64) ** 2, axis=1) < 2.0 ** 80
        miss, _ = lost(t, o[keep], d[keep])
        assert miss == 0
    assert total > 100


def test_an_under_inflated_bound_is_caught():
    """The generators above do find what a bound with too small a margin loses: the test can detect an unsound bound."""
    rng = np.random.default_rng(11)
    caught = 0
    for _ in range(120):
        t = random_triangle(rng, 1.0)
        o, d = grazing_rays(rng, t, 100, DETS)
        miss, _ = lost(t, o, d, margin=0.0)
        caught += miss
        assert lost(t, o, d, margin=1.0)[0] == 0
    assert caught > 0
