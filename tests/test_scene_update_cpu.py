"""The refit of the mesh image's bounds (csrc/ptmesh.h refitBound — the arithmetic and reduction shape of meshRefitKernel,
ptss_update_triangles), on the host build of the very code the kernel runs (ptss_probe_mesh_refit): the bounds
hold what they must, checked in float64; the soundness battery of tests/test_mesh_bound.py runs against REFIT bounds — every ray
the oracle's triangle test accepts must get "may touch" — and fails with the margin scaled down; and the argument errors of the new
entry points return before any device call. No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from scene_update_common import deform, m1296, m530, stored
from test_mesh_bound import DETS, general_form, grazing_rays, icosphere_leaves, random_triangle, rays_at

K_B_PER_L2 = 64.0 * 2.0 ** -24 * 1.00001
SLACK_DIR = 2.0 ** -20   # ptmesh.h kSlackDir: what the predicate allows for the axis being rounded to float


def check_bound(b, tris):
    """b: 12 floats; tris: (n, 9) stored rows it was refitted around. Everything in float64 from the exact float inputs."""
    t = tris.astype(np.float64)
    b = b.astype(np.float64)
    v0, e1, e2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    for p in (v0, v0 + e1, v0 + e2):
        assert np.all(np.linalg.norm(p - b[0:3], axis=1) <= b[3])                       # the ball holds every stored vertex
    N = np.cross(e1, e2)
    ln = np.linalg.norm(N, axis=1)
    assert b[9] <= ln.min()                                                             # Nmin
    sides = np.stack([np.linalg.norm(e, axis=1) for e in (e1, e2, e2 - e1)])
    assert b[10] >= sides.max()                                                         # Lmax
    assert b[11] >= K_B_PER_L2 * b[10] * b[10]                                          # B
    assert 0.0 <= b[7] <= 1.0 and 0.0 <= b[8] <= 1.0
    if ln.min() > 0 and b[7] > 0:
        assert abs(np.linalg.norm(b[4:7]) - 1.0) < 1e-6
        cosN = np.abs(N @ b[4:7]) / ln
        assert np.all(cosN >= b[7] - SLACK_DIR)                                         # the cone holds every normal:
        assert np.all(np.sqrt(np.maximum(0.0, 1.0 - cosN * cosN)) <= b[8] + SLACK_DIR)  # cos alpha from below, sin alpha from above
    if ln.min() == 0:
        assert b[7] == 0.0 and b[8] == 1.0 and b[9] == 0.0                              # no cone: every direction may graze


def leaves_and_groups(tris):
    n = len(tris)
    leaves = [tris[k:k + 16] for k in range(0, n, 16)]
    return leaves + [tris[k:k + 256] for k in range(0, n, 256)]


@pytest.mark.parametrize("make", [m530, m1296])
@pytest.mark.parametrize("deformed", [False, True])
def test_refit_bounds_hold_their_triangles(make, deformed):
    t = make().triangles
    rows = stored(deform(t) if deformed else t)
    bounds = ptss.probe_mesh_refit(rows)
    parts = leaves_and_groups(rows)
    assert len(bounds) == len(parts)
    for b, part in zip(bounds, parts):
        check_bound(b, part)


def test_undeformed_refit_against_the_packed_bound():
    """Ball, Nmin, Lmax and B do not depend on the axis rule: the refit gives buildBound's bits. The cone may differ (another,
    equally legal axis) but holds every normal (check_bound) and is no tighter than the data allow."""
    rows = stored(m530().triangles)
    bounds = ptss.probe_mesh_refit(rows)
    for b, part in zip(bounds, leaves_and_groups(rows)):
        _, packed = ptss.probe_mesh_bound(part, np.zeros((0, 3)), np.zeros((0, 3)))
        assert np.array_equal(b[[0, 1, 2, 3, 9, 10, 11]].view(np.uint32), packed[[0, 1, 2, 3, 9, 10, 11]].view(np.uint32))
        check_bound(b, part)


def lost(leaf, o, d, limit=np.inf, margin=1.0, which=0):
    """Rays accepted by some triangle of `leaf` that its REFIT bound rejects (which: 0 the leaf's bound, -1 the group's), and how
    many were accepted."""
    leaf = np.asarray(leaf, dtype=np.float32).reshape(-1, 9)
    acc = np.zeros(len(o), dtype=bool)
    for t in leaf:
        a, _, _ = general_form(np.broadcast_to(t, (len(o), 9)), o, d, limit)
        acc |= a
    may = ptss.probe_mesh_touch(ptss.probe_mesh_refit(leaf)[which], o, d, margin)
    return int(np.count_nonzero(acc & (may == 0))), int(np.count_nonzero(acc))


def test_the_general_form_is_the_oracles_triangle_test():
    rng = np.random.default_rng(2)
    for _ in range(20):
        v = rng.uniform(-5, 5, (3, 3)).astype(np.float32)
        t = np.concatenate([v[0], v[1] - v[0], v[2] - v[0]])
        o, d = rays_at(rng, t, 8)
        acc, _, _ = general_form(np.broadcast_to(t, (8, 9)), o, d, np.inf)
        for k in range(8):
            assert oracle.probe_triangle(v[0], v[1], v[2], o[k], d[k])[0] == bool(acc[k])


@pytest.mark.parametrize("scale", [1e-3, 0.05, 1.0, 10.0])
def test_random_rays_lose_nothing(scale):
    rng = np.random.default_rng(int(scale * 1000) + 17)
    total = 0
    for _ in range(100):
        t = random_triangle(rng, scale)
        o, d = rays_at(rng, t, 500)
        for which in (0, -1):
            miss, acc = lost(t, o, d, which=which)
            assert miss == 0
        total += acc
    assert total > 4000


def deformed_icosphere_leaves():
    out = []
    for leaf in icosphere_leaves():
        # the deformation of scene_update_common, on stored rows: rebuild vertices, deform, store again
        t = np.zeros(len(leaf), dtype=ptss.TRIANGLE_DTYPE)
        t["vertex0"], t["vertex1"], t["vertex2"] = leaf[:, 0:3], leaf[:, 0:3] + leaf[:, 3:6], leaf[:, 0:3] + leaf[:, 6:9]
        out.append(stored(deform(t)))
    return out


def test_deformed_leaves_with_shared_edges_lose_nothing():
    rng = np.random.default_rng(3)
    total = 0
    for leaf in deformed_icosphere_leaves()[::4]:
        o, d = [], []
        for t in leaf:
            for a, b in (rays_at(rng, t, 60, spread=0.05), grazing_rays(rng, t, 6, DETS)):
                o.append(a)
                d.append(b)
        for which in (0, -1):
            miss, acc = lost(leaf, np.concatenate(o), np.concatenate(d), which=which)
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
        miss, _ = lost(t, o, d, limit=np.where(acc, dist, np.float32(1.0)))
        assert miss == 0


def test_origins_near_the_eligibility_bound():
    rng = np.random.default_rng(9)
    far = 2.0 ** 39
    total = 0
    for _ in range(60):
        v0 = rng.uniform(-far, far, 3)
        t = np.concatenate([v0, rng.normal(0, far / 64, 3), rng.normal(0, far / 64, 3)]).astype(np.float32)
        o, d = rays_at(rng, t, 300, dist=(far / 8, far / 2))
        o = np.clip(o, -far * 1.2, far * 1.2)
        assert np.all(np.sum(o.astype(np.float64) ** 2, axis=1) < 2.0 ** 80)
        miss, acc = lost(t, o, d)
        assert miss == 0
        total += acc
        o, d = grazing_rays(rng, t, 20, DETS[:4], reach=(far / 8, far / 2))
        keep = np.sum(o.astype(np.float64) ** 2, axis=1) < 2.0 ** 80
        assert lost(t, o[keep], d[keep])[0] == 0
    assert total > 100


def test_a_leaf_with_a_zero_area_triangle_and_a_needle():
    """Nmin = 0 (no cone: cos alpha 0, every direction may graze) and a needle whose normal is tiny beside its sides."""
    rng = np.random.default_rng(21)
    good = [random_triangle(rng, 1.0) for _ in range(6)]
    v0 = np.array([0.5, -1.0, 2.0], dtype=np.float32)
    flat = np.concatenate([v0, [1.0, 0.5, 0.25], [2.0, 1.0, 0.5]]).astype(np.float32)          # e2 = 2 e1: no area
    needle = np.concatenate([v0, [3.0, 0.0, 0.0], [3.0, 1e-6, 0.0]]).astype(np.float32)
    with_flat = np.stack(good + [flat, needle])
    only_needle = np.stack(good + [needle])
    b = ptss.probe_mesh_refit(with_flat)
    assert b[0][9] == 0.0 and b[0][7] == 0.0 and b[0][8] == 1.0
    check_bound(b[0], with_flat)
    check_bound(ptss.probe_mesh_refit(only_needle)[0], only_needle)
    total = 0
    for leaf in (with_flat, only_needle):
        o, d = [], []
        for t in leaf:
            for a, c in (rays_at(rng, t, 300), grazing_rays(rng, t, 20, DETS)):
                o.append(a)
                d.append(c)
        miss, acc = lost(leaf, np.concatenate(o), np.concatenate(d))
        assert miss == 0
        total += acc
    assert total > 500


def test_an_under_inflated_refit_bound_is_caught():
    rng = np.random.default_rng(11)
    caught = 0
    for _ in range(120):
        t = random_triangle(rng, 1.0)
        o, d = grazing_rays(rng, t, 100, DETS)
        caught += lost(t, o, d, margin=0.0)[0]
        assert lost(t, o, d, margin=1.0)[0] == 0
    assert caught > 0


def test_argument_errors_return_before_any_device_call():
    L = ptss.device_lib()
    scene = ptss.Scene("cornell")
    tri = np.zeros(4, dtype=ptss.TRIANGLE_DTYPE)
    n = C.c_ulonglong()
    assert L.ptss_set_scene(None, C.byref(scene.desc)) == -1
    assert L.ptss_update_triangles(None, tri.ctypes.data, 0, 4, None) == -1
    assert L.ptss_update_rejected(None, C.byref(n)) == -1
    assert L.ptss_reseed(None, 1) == -1
    assert L.ptss_read_triangle_bounds(None, None, 0) == -1
    assert L.ptss_read_triangle_positions(None, None, 0) == -1
    assert ptss.host_lib().ptss_probe_mesh_refit(None, 4, None) == -1
