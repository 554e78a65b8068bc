"""Rays from surface points and the gutter fill on the GPU (ptss_generate_rays_surface / ptss_dilate_linear).

1. The device equals the host build byte for byte — rays, streams, surfels and the rejected count — on a plain, a classed, a mesh and the
many-sphere image (two of them store their primitives in another order), both modes, both sides, n around a wave and a workgroup,
without an index, with duplicates, with a permutation and with one of every kind of rejected entry. 2. Live meshes: after
ptss_update_triangles and again after ptss_resort_triangles the rays are those of the new records. 3. Independent of the probe: a short
ray back along the normal finds the point's own primitive. 4. The whole chain in closed form on one triangle under a uniform sky.
5. The gutter fill in both kernel forms. 6. Refusals."""
import ctypes as C

import numpy as np
import pytest

import ptss
from linear_common import model_fixed
from scene_update_common import WHITE, TableScene, deform, m530, p300, preset_triangles, seventy_spheres, triangles_of
from surface_common import (DILATE_GPU_SIZES, NS, TRIANGLE, bad_points, dilate_films, first_difference, good_points, host_states, make_points,
                            model_dilate, same_bytes, words)

pytestmark = pytest.mark.gpu
MODES = ("normal", "cosine")
SCENES = {
    "plain": p300,                                                                          # 300 triangles in the caller's order
    "classed": lambda: ptss.Scene("mixed"),                                                 # 16 triangles stored by edge class, 22 spheres
    "mesh": m530,                                                                           # 530 triangles in a kd order, beyond ldsVec4
    "many_spheres": lambda: seventy_spheres(preset_triangles("mixed"), preset="mixed"),     # 70 spheres in a spatial order
}


def image_kind(scene):
    L = ptss.probe_pack_scene(scene)[0]
    if L["accelSpheres"]:
        return "many_spheres"
    if L["triClassed"]:
        return "classed"
    return "mesh" if L["numLeaves"] > 0 else "plain"


class Context:
    def __init__(self, name):
        self.name, self.scene = name, SCENES[name]()
        assert image_kind(self.scene) == name
        self.tri, self.sph = ptss.scene_records(self.scene)
        self.r = ptss.Renderer(self.scene, 16, 16, max_iterations=2)
        self.launches, self.rejected = self.r.surface_launches()[0], self.r.surface_rejected()

    def check(self, what, points, rng, params, tri=None, **kw):
        """One device call against the probe over the caller's records: everything it writes, what it counts."""
        tri = self.tri if tri is None else tri
        want = ptss.probe_surface_rays(tri, self.sph, points, rng, params, **kw)
        got = self.r.generate_rays_surface(points, rng, params, **kw)
        assert same_bytes(got[0], want[0]), (self.name, what, "rays", first_difference(got[0], want[0]))
        assert same_bytes(got[1], want[1]), (self.name, what, "streams", first_difference(got[1], want[1]))
        if want[2] is not None:
            assert same_bytes(got[2], want[2]), (self.name, what, "surfels", first_difference(got[2], want[2]))
        self.launches += 1 if len(rng) else 0
        self.rejected += want[3]
        assert self.r.surface_launches()[0] == self.launches and self.r.surface_rejected() == self.rejected, (self.name, what)
        return want


@pytest.fixture(scope="module", params=list(SCENES))
def ctx(request):
    c = Context(request.param)
    yield c
    c.r.close()


# ---- 1. the device equals the host build ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_device_equals_the_host_build(ctx, mode):
    T, S = len(ctx.tri), len(ctx.sph)
    params = ptss.surface_params(mode, max_distance=float("inf") if mode == "cosine" else 0.75)
    good = good_points(T, S, 1100, seed=len(ctx.name))
    names, bad = bad_points(T, S)
    points = np.concatenate([good[:600], bad, good[600:]])   # the rejected kinds lie inside the range the largest batches walk
    bad_at = np.arange(600, 600 + len(bad))
    assert {int(f) for f in good["flags"]} == {0, 1} and (good["surface"] < TRIANGLE).any() and (good["surface"] >= TRIANGLE).any()
    g = np.random.default_rng(7)
    states = host_states(max(NS))
    rejected_before = ctx.rejected
    for n in NS:
        s0 = states[:n]
        marked = dict(rays=np.full((n, 8), 7.5, np.float32), surfels=np.full((n, 12), -3.25, np.float32))
        ctx.check((n, "range"), points, s0, params, first_point=(37 if n < 1025 else 5), **marked)
        ctx.check((n, "range, no surfels"), points, s0, params, first_point=len(points) - n)
        ctx.check((n, "duplicates"), points, s0, params, index=g.integers(0, 64, n).astype(np.uint32), **marked)
        perm = g.permutation(len(points))[:n].astype(np.uint32)
        ctx.check((n, "permutation"), points, s0, params, index=perm, **marked)
        mixed = perm.copy()
        slots = g.permutation(n)[:min(n, len(bad) + 3)]
        beyond = [len(points), 2 ** 31, 2 ** 32 - 1]
        mixed[slots] = np.concatenate([beyond, bad_at])[:len(slots)]
        want = ctx.check((n, "rejected entries"), points, s0, params, index=mixed, **marked)
        assert want[3] >= len(slots)
        for i in slots:   # a rejected entry writes no row and leaves its stream
            assert (words(want[0])[i] == words(marked["rays"])[i]).all() and (words(want[1])[i] == s0[i]).all()
    assert ctx.rejected > rejected_before
    # n = 0 launches nothing
    ctx.check("empty", points, states[:0], params)


# ---- 2. live meshes -------------------------------------------------------------------------------------------------------------------
def test_rays_follow_update_and_resort():
    """The mesh image after ptss_update_triangles with new vertices and normals, and again after ptss_resort_triangles has moved the rows:
    the device's rays equal the probe fed the NEW records (and differ from the old ones')."""
    c = Context("mesh")
    try:
        T, S = len(c.tri), len(c.sph)
        points = good_points(T, S, 700, seed=4)
        s0 = host_states(700)
        params = ptss.surface_params("cosine")
        old = c.check("before", points, s0, params, surfels=True)
        moved = deform(c.tri)
        c.r.update_triangles(moved)
        assert c.r.update_rejected() == 0
        new = c.check("updated", points, s0, params, tri=moved, surfels=True)
        assert not same_bytes(new[0], old[0])
        before = c.r.triangle_positions(T)
        c.r.resort_triangles()
        c.r.synchronize()
        after = c.r.triangle_positions(T)
        assert (before != after).any() and sorted(after.tolist()) == list(range(T))   # the rows have moved
        c.check("resorted", points, s0, params, tri=moved, surfels=True)
        c.check("resorted, normal mode", points, s0, ptss.surface_params("normal"), tri=moved, surfels=True)
    finally:
        c.r.close()


# ---- 3. independent of the probe ------------------------------------------------------------------------------------------------------
def test_a_short_ray_back_along_the_normal_finds_the_points_own_primitive():
    """The scene is scene_update_common.m530: an icosphere of 320 triangles above a floor grid of 210 (the nearest two surfaces are 0.3
    apart) and the Cornell preset's two spheres — no coincident surfaces. For interior points (a, b >= 0.1, a + b <= 0.9) ptss_intersect
    from the ray's origin along -n with tmax = 1e-3 reports the point's own primitive."""
    c = Context("mesh")
    try:
        points = good_points(len(c.tri), len(c.sph), 900, seed=12, interior=True)
        rays, _, surfels = c.r.generate_rays_surface(points, np.zeros((len(points), 6), np.uint32), ptss.surface_params("normal"), surfels=True)
        back = ptss.make_rays(rays["origin"], -surfels["normal"], 1e-3)
        hits = c.r.intersect(back)
        assert (points["surface"] >= TRIANGLE).sum() > 300 and (points["surface"] < TRIANGLE).sum() > 100
        assert np.array_equal(hits["kind"], surfels["kind"]) and np.array_equal(hits["primitive"], surfels["primitive"])
    finally:
        c.r.close()


# ---- 4. the whole chain in closed form ------------------------------------------------------------------------------------------------
SKY = (0.25, 0.5, 0.125)


def sky_scene():
    """One upward Lambert triangle, no spheres, no lights, defaultColor = SKY: every cosine ray misses and every radiance is SKY."""
    t = triangles_of([(-1, 0, -2)], [(1, 0, -2)], [(-1, 0, -4)], WHITE, normals=np.float32([[[0, 1, 0]] * 3]))
    s = TableScene(t, spheres=[], point_lights=[], keep_area_lights=False)
    s.desc.defaultColor.x, s.desc.defaultColor.y, s.desc.defaultColor.z = SKY
    return s


def test_the_bake_chain_in_closed_form():
    scene = sky_scene()
    tri = ptss.scene_records(scene)[0]
    assert tri["normal0"][0][1] == 1 and np.cross(tri["vertex1"][0] - tri["vertex0"][0], tri["vertex2"][0] - tri["vertex0"][0])[1] != 0
    r = ptss.Renderer(scene, 16, 16, max_iterations=4)
    try:
        width, rounds = 9, 3
        points, texels, height = ptss.surface_atlas(tri, 3.0, width, 1, 8)   # longest edge 2.83 at 3 texels a unit: side 8 (clamped), 36 texels
        assert len(points) == 36 and height == 8
        P, params, cosine = width * height, ptss.linear_params(), ptss.surface_params("cosine")
        q = [model_fixed(np.float32(c), params)[0] for c in SKY]
        want = np.zeros(P, dtype=ptss.LINEAR_DTYPE)
        want["r"][texels], want["g"][texels], want["b"][texels], want["samples"][texels] = rounds * q[0], rounds * q[1], rounds * q[2], rounds

        def bake(order, schedule):
            film, rng = np.zeros(P, dtype=ptss.LINEAR_DTYPE), r.seed_path_rng(len(order), 0x5EED)
            for _ in range(rounds):
                rays, rng, _ = r.generate_rays_surface(points, rng, cosine, index=order.astype(np.uint32))
                results, rng = r.trace_paths(rays, rng, 4, schedule=schedule)
                assert same_bytes(results["radiance"], np.broadcast_to(np.float32(SKY), (len(order), 3)))
                film = r.accumulate_paths_linear(results, film, index=texels[order], params=params)
            return film

        film = bake(np.arange(len(points)), None)
        assert same_bytes(film, want), first_difference(film, want)
        assert r.surface_rejected() == 0 and r.film_rejected() == 0
        # the refill schedule and a permuted index give the same bytes
        assert same_bytes(bake(np.arange(len(points)), "refill"), want)
        assert same_bytes(bake(np.random.default_rng(3).permutation(len(points)), None), want)
        # one gutter fill: each empty neighbour of the block gets the integer sum the model predicts
        filled = r.dilate_linear(film, width, height)
        model = model_dilate(want, width, height)
        assert same_bytes(filled, model), first_difference(filled, model)
        grown = (want["samples"] == 0) & (filled["samples"] > 0)
        assert grown.sum() >= 8 and (filled["r"][grown] == filled["samples"][grown].astype(np.uint64) // rounds * np.uint64(rounds * q[0])).all()
        # ... and its resolve shows the sky on them
        means = r.resolve_linear(filled, params=params, pixels=None, history=None)[0]
        assert np.abs(means["r"][grown] - SKY[0]).max() < 2e-6 and np.abs(means["g"][grown] - SKY[1]).max() < 2e-6
    finally:
        r.close()


# ---- 5. the gutter fill ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


@pytest.mark.parametrize("width,height", DILATE_GPU_SIZES)
def test_the_dilate_equals_the_probe_in_both_forms(small, width, height):
    launches = small.surface_launches()[1]
    for name, film in dilate_films(width, height).items():
        want = ptss.probe_dilate_linear(film, width, height)
        for form in (0, 1, 2):
            small.debug_dilate_linear_form(form)
            try:
                got = small.dilate_linear(film, width, height)
                again = small.dilate_linear(got, width, height)
            finally:
                small.debug_dilate_linear_form(0)
            assert same_bytes(got, want), (name, form, first_difference(got, want))
            assert same_bytes(again, ptss.probe_dilate_linear(want, width, height)), (name, form, "second pass")
            launches += 2
            assert small.surface_launches()[1] == launches


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_count_nothing(small):
    L, H = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    before = (small.surface_launches(), small.surface_rejected())
    buf = C.c_void_p()
    assert H.hipMalloc(C.byref(buf), 4096) == 0
    try:
        d = buf.value
        ok = ptss.surface_params()
        gen = lambda params=ok, points=d, num=8, first=0, index=None, n=8, rng=d + 1024, rays=d + 2048, surfels=None, ctx=small._ctx: \
            L.ptss_generate_rays_surface(ctx, C.byref(params) if params is not None else None, points, num, first, index, n, rng, rays, surfels, None)
        bad = []
        for change in (dict(structSize=20), dict(mode=2), dict(reserved=7), dict(maxDistance=0.0), dict(maxDistance=-2.0), dict(maxDistance=float("nan"))):
            p = ptss.surface_params()
            for k, v in change.items():
                setattr(p, k, v)
            bad.append(p)
        for p in bad:
            assert gen(params=p) == EINVAL
        assert gen(ctx=None) == EINVAL and gen(params=None) == EINVAL
        assert gen(points=None) == EINVAL and gen(rng=None) == EINVAL and gen(rays=None) == EINVAL
        assert gen(points=d + 8) == EINVAL and gen(rays=d + 2048 + 8) == EINVAL and gen(surfels=d + 3072 + 4) == EINVAL
        assert gen(rng=d + 1024 + 2) == EINVAL and gen(index=d + 1) == EINVAL
        assert gen(n=2 ** 31) == ERANGE and gen(num=2 ** 31) == ERANGE
        assert gen(first=1) == ERANGE and gen(first=9, n=0) == 0 and gen(num=8, first=4, n=5) == ERANGE
        assert gen(n=0, points=None, rng=None, rays=None) == 0   # n = 0 returns OK
        dil = lambda film=d, w=4, h=4, out=d + 2048, ctx=small._ctx: L.ptss_dilate_linear(ctx, film, w, h, out, None)
        assert dil(ctx=None) == EINVAL and dil(film=None) == EINVAL and dil(out=None) == EINVAL and dil(out=d) == EINVAL
        assert dil(film=d + 8) == EINVAL and dil(out=d + 2048 + 4) == EINVAL
        assert dil(w=0) == ERANGE and dil(h=-3) == ERANGE and dil(w=1 << 16, h=1 << 15) == ERANGE
        assert L.ptss_debug_dilate_linear_form(small._ctx, 3) == EINVAL and L.ptss_debug_dilate_linear_form(small._ctx, -1) == EINVAL
        assert L.ptss_surface_launches(small._ctx, None) == EINVAL and L.ptss_surface_rejected(small._ctx, None) == EINVAL
    finally:
        H.hipFree(buf)
    assert (small.surface_launches(), small.surface_rejected()) == before
    # the wrapper's own checks
    with pytest.raises(ValueError):
        small.dilate_linear(np.zeros(5, dtype=ptss.LINEAR_DTYPE), 2, 2)
    with pytest.raises(ValueError):
        small.generate_rays_surface(make_points([(0, 0.5, 0.5, 0)]), np.zeros((2, 6), np.uint32), index=np.zeros(3, np.uint32))
