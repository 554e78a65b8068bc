"""Light maps read back on the GPU (ptss_lookup_lightmap).

1. The device equals the host build byte for byte — rows and the four counts — on a plain, a classed (triangles plus spheres) and a mesh
image: hits of a 16 x 16 camera's centre rays, surfels of the atlas' points and one of every kind of rejected hit and block row inside
the range; n around a quad, a wave and a workgroup in both kernel forms; both filters, every flag combination, all three values of
ptss_debug_lightmap_form (form 1's bytes are form 2's); dev_info given (added to) and NULL; maps before and after ptss_dilate_linear and
with samples == 1 rows beside ordinary ones. 2. Live meshes: after ptss_update_triangles and ptss_resort_triangles the hits of the new
pose look up the same blocks. 3. Independent of the probe: §3.38's closed-form chain, baked and looked up from a camera. 4. The whole view
loop on `mixed` against a shadow loop of the probes. 5. Refusals."""
import ctypes as C

import numpy as np
import pytest

import ptss
import ptss_types
from lightmap_common import FILTERED, FILTERS, FLAGS, NO_BLOCK, NS, REJECTED, hits_with_bad_rows, modulate_weight, random_map
from linear_common import model_fixed
from scene_update_common import WHITE, TableScene, deform, m530, p300, triangles_of
from surface_common import first_difference, same_bytes

pytestmark = pytest.mark.gpu
SCENES = {"p300": p300, "mixed": lambda: ptss.Scene("mixed"), "m530": m530}
ATLAS_WIDTH = 128


def lm_params(width, height, filter="bilinear", flags=(False, False), **kw):
    return ptss.lightmap_params(width, height, filter, modulate=flags[0], emission=flags[1], **kw)


def camera_hits(r, width, height, camera=None):
    """ptss_intersect of the centre rays of a pinhole film: ((N,) RAY_DTYPE, (N,) HIT_DTYPE)."""
    film = ptss.film_camera("pinhole", width, height, camera, jitter=0)
    rays = r.generate_rays(film, np.zeros((width * height, 6), np.uint32))[0]
    return rays, r.intersect(rays)


class Context:
    def __init__(self, name):
        self.name, self.scene = name, SCENES[name]()
        self.tri, self.sph = ptss.scene_records(self.scene)
        self.mat = ptss.scene_materials(self.scene)
        self.r = ptss.Renderer(self.scene, 16, 16, max_iterations=2)
        self.bt, self.bs, self.points, self.texels, self.height = ptss.surface_atlas_blocks(self.tri, self.sph, 2.0, ATLAS_WIDTH, 1, 16)
        seen = camera_hits(self.r, 16, 16)[1]
        pick = np.linspace(0, len(self.points) - 1, max(NS) - len(seen) + 40).astype(np.int64)
        surfels = self.r.generate_rays_surface(self.points[pick], np.zeros((len(pick), 6), np.uint32), ptss.surface_params("normal"), surfels=True)[2]
        order = np.random.default_rng(len(name)).permutation(len(seen) + len(surfels))
        self.good = np.concatenate([seen, surfels])[order]
        self.good[0] = surfels[0]   # entry 0 stays a good hit


@pytest.fixture(scope="module", params=list(SCENES))
def ctx(request):
    c = Context(request.param)
    yield c
    c.r.close()


# ---- 1. the device equals the host build ---------------------------------------------------------------------------------------------
def test_the_device_equals_the_host_build(ctx):
    import torch
    r, W, H = ctx.r, ATLAS_WIDTH, ctx.height
    hits, blocks = hits_with_bad_rows(ctx.good, ctx.bt, lm_params(W, H), len(ctx.mat))
    hits = hits[:max(NS)]
    assert (hits["kind"] == 2).any() and (hits["kind"] == 1).any()   # every scene here has spheres
    raw = random_map(W, H, ctx.texels, seed=len(ctx.name))
    maps = {"raw": raw, "filled": r.dilate_linear(raw, W, H), "with samples == 1": random_map(W, H, ctx.texels, seed=3, big=True, ones=0.5)}
    assert (maps["filled"]["samples"] > 0).sum() > (raw["samples"] > 0).sum()
    dev = lambda a, word: torch.from_numpy(np.ascontiguousarray(a).view(word).reshape(len(a), -1).copy()).cuda()
    d_hits, d_bt = dev(hits, np.float32), dev(blocks, np.int32)
    d_bs = dev(ctx.bs, np.int32) if len(ctx.bs) else None
    launches = r.lightmap_launches()
    film = ptss.linear_params()
    for name, map_ in maps.items():
        d_map = dev(map_, np.int64)
        for filter in FILTERS:
            for flags in FLAGS:
                params = lm_params(W, H, filter, flags)
                want, _ = ptss.probe_lookup_lightmap(ctx.mat, hits, map_, params, blocks, ctx.bs, film=film)
                d_info = torch.full((4,), 7, dtype=torch.int32, device="cuda")
                total = np.full(4, 7, dtype=np.int64)
                by_form = {}
                for n in (NS if name == "raw" else NS[-1:]):
                    counts = ptss.probe_lookup_lightmap(ctx.mat, hits[:n], map_, params, blocks, ctx.bs, film=film)[1].astype(np.int64)
                    assert counts.sum() == n
                    for form in (0, 1, 2):
                        r.debug_lightmap_form(form)
                        try:
                            out = r.lookup_lightmap(d_hits[:n], d_map, params, d_bt, d_bs, film=film, info=d_info)
                            got = out.cpu().numpy().view(np.uint64)
                        finally:
                            r.debug_lightmap_form(0)
                        case = (ctx.name, name, filter, flags, n, form)
                        assert same_bytes(got, want[:n]), (case, first_difference(got, want[:n]))
                        total += counts
                        launches += 1
                        assert np.array_equal(d_info.cpu().numpy().astype(np.int64), total), (case, "counts are added")
                        by_form[form] = got.tobytes()
                    assert by_form[1] == by_form[2]
                    # dev_info NULL: the same rows
                    out = r.lookup_lightmap(d_hits[:n], d_map, params, d_bt, d_bs, film=film)
                    launches += 1
                    assert same_bytes(out.cpu().numpy().view(np.uint64), want[:n])
                if name == "raw" and filter == "bilinear":
                    full = ptss.probe_lookup_lightmap(ctx.mat, hits, map_, params, blocks, ctx.bs, film=film)[1]
                    assert full[FILTERED] > 300 and full[REJECTED] >= 23 and full[NO_BLOCK] >= 5, full
    assert r.lightmap_launches() == launches
    # the array path of the wrapper: the same rows, the counts returned
    params = lm_params(W, H, "bilinear", (True, True))
    got, info = r.lookup_lightmap(hits[:257], raw, params, blocks, ctx.bs)
    want, counts = ptss.probe_lookup_lightmap(ctx.mat, hits[:257], raw, params, blocks, ctx.bs)
    assert same_bytes(got, want) and np.array_equal(info, counts)
    assert r.lookup_lightmap(hits[:5], raw, params, blocks, ctx.bs, info=False)[1] is None
    # n = 0 launches nothing
    before = r.lightmap_launches()
    assert len(r.lookup_lightmap(hits[:0], raw, params, blocks, ctx.bs)[0]) == 0 and r.lightmap_launches() == before


# ---- 2. live meshes -------------------------------------------------------------------------------------------------------------------
def test_lookups_follow_update_and_resort():
    """Hits carry the caller's indices: after ptss_update_triangles the hits of the new pose look up their blocks, and after
    ptss_resort_triangles has moved the rows the same rays give the same hits' primitives and the same looked-up rows."""
    c = Context("m530")
    try:
        r, W, H = c.r, ATLAS_WIDTH, c.height
        film_map = random_map(W, H, c.texels, seed=8)
        params = lm_params(W, H, "bilinear", (True, True))
        rays, before = camera_hits(r, 32, 24)

        def check(hits):
            got, info = r.lookup_lightmap(hits, film_map, params, c.bt, c.bs)
            want, counts = ptss.probe_lookup_lightmap(c.mat, hits, film_map, params, c.bt, c.bs)
            assert same_bytes(got, want), first_difference(got, want)
            assert np.array_equal(info, counts) and info[FILTERED] > 100
            return got

        check(before)
        r.update_triangles(deform(c.tri))
        assert r.update_rejected() == 0
        moved = r.intersect(rays)
        assert not same_bytes(moved, before)
        rows = check(moved)
        T = len(c.tri)
        order = r.triangle_positions(T)
        r.resort_triangles()
        r.synchronize()
        assert (order != r.triangle_positions(T)).any()
        resorted = r.intersect(rays)
        assert np.array_equal(resorted["kind"], moved["kind"]) and np.array_equal(resorted["primitive"], moved["primitive"])
        assert same_bytes(check(resorted), rows)
    finally:
        c.r.close()


# ---- 3. independent of the probe ------------------------------------------------------------------------------------------------------
SKY = (0.25, 0.5, 0.125)


def sky_scene(albedo):
    """§3.38's closed-form scene — one upward Lambert triangle, no spheres, no lights, defaultColor = SKY — with the triangle's material
    given the diffuse colour `albedo` and no emission."""
    t = triangles_of([(-1, 0, -2)], [(1, 0, -2)], [(-1, 0, -4)], WHITE, normals=np.float32([[[0, 1, 0]] * 3]))
    s = TableScene(t, spheres=[], point_lights=[], keep_area_lights=False)
    mats = ptss.scene_materials(s)
    mats["diffuseColor"][WHITE], mats["emmitance"][WHITE] = albedo, 0
    s._materials = (ptss_types.Material * len(mats)).from_buffer_copy(mats.tobytes())
    s.desc.materials = s._materials
    s.desc.defaultColor.x, s.desc.defaultColor.y, s.desc.defaultColor.z = SKY
    return s


def looking_down():
    """A camera two units above the triangle, looking along -y (the default camera looks along -z: a quarter turn about x)."""
    cam = ptss.default_camera()
    cam.position.x, cam.position.y, cam.position.z = -0.3, 2.0, -2.7
    h = float(np.sqrt(0.5))
    cam.rotation.x, cam.rotation.y, cam.rotation.z, cam.rotation.w = -h, 0.0, 0.0, h
    return cam


@pytest.mark.parametrize("albedo", [(0.5, 0.5, 0.5), (1.0, 0.25, 0.0)])
def test_the_chain_in_closed_form_from_a_camera(albedo):
    """Every cosine ray of the bake misses, so every baked texel's mean is the sky's fixed point m, whatever the filter reads. From a
    camera above: every pixel that hits the triangle shows (m q + 32768) >> 16 with q the albedo in 1/65536 — (m + 1) >> 1 at an albedo
    of 0.5 —, every other pixel is zero, and the four counts add up to n."""
    scene = sky_scene(albedo)
    tri, sph = ptss.scene_records(scene)
    r = ptss.Renderer(scene, 16, 16, max_iterations=4)
    try:
        W, rounds = 9, 3
        bt, bs, points, texels, H = ptss.surface_atlas_blocks(tri, sph, 3.0, W, 1, 8)
        assert len(points) == 36 and H == 8 and len(bs) == 0
        film, cosine = ptss.linear_params(), ptss.surface_params("cosine")
        baked, rng = np.zeros(W * H, dtype=ptss.LINEAR_DTYPE), r.seed_path_rng(len(points), 0x5EED)
        for _ in range(rounds):
            rays, rng, _ = r.generate_rays_surface(points, rng, cosine)
            results, rng = r.trace_paths(rays, rng, 4)
            baked = r.accumulate_paths_linear(results, baked, index=texels, params=film)
        m = [model_fixed(np.float32(c), film)[0] for c in SKY]
        assert (baked["samples"][texels] == rounds).all() and (baked["r"][texels] == rounds * m[0]).all()
        _, hits = camera_hits(r, 24, 16, looking_down())
        on = hits["kind"] == 2
        assert 40 < on.sum() < len(hits) - 40 and (hits["kind"][~on] == 0).all()
        want = [(m[c] * modulate_weight(albedo[c]) + 32768) >> 16 for c in range(3)]
        if albedo[0] == 0.5:
            assert want == [(v + 1) >> 1 for v in m]
        for map_ in (baked, r.dilate_linear(baked, W, H)):
            for filter in FILTERS:
                got, info = r.lookup_lightmap(hits, map_, lm_params(W, H, filter, (True, False)), bt, None, film=film)
                assert info.sum() == len(hits) and info[FILTERED] == on.sum() and info[NO_BLOCK] == (~on).sum()
                for c, name in enumerate("rgb"):
                    assert (got[name][on] == want[c]).all(), (filter, name)
                assert (got["samples"][on] == 1).all() and not np.ascontiguousarray(got[~on]).view(np.uint64).any()
                plain, _ = r.lookup_lightmap(hits, map_, lm_params(W, H, filter), bt, None, film=film)
                assert (plain["r"][on] == m[0]).all() and (plain["g"][on] == m[1]).all() and (plain["b"][on] == m[2]).all()
    finally:
        r.close()


# ---- 4. the whole view loop -----------------------------------------------------------------------------------------------------------
def test_the_view_loop_equals_the_shadow_loop_of_the_probes():
    """`mixed` at 32 x 24: bake through the atlas with sphere blocks, fill, intersect, look up, meter, resolve on the device; the probes
    stand in for every step but the trace and the intersection (whose results both loops share)."""
    scene = ptss.Scene("mixed")
    tri, sph = ptss.scene_records(scene)
    mat = ptss.scene_materials(scene)
    r = ptss.Renderer(scene, 32, 24, max_iterations=3, seed=0xBA4E)
    try:
        W = 64
        bt, bs, points, texels, H = ptss.surface_atlas_blocks(tri, sph, 1.5, W, 1, 16)
        film, cosine = ptss.linear_params(), ptss.surface_params("cosine")
        dev, host = np.zeros(W * H, dtype=ptss.LINEAR_DTYPE), np.zeros(W * H, dtype=ptss.LINEAR_DTYPE)
        rng = r.seed_path_rng(len(points), 0xBA4E)
        for _ in range(2):
            rays, after, _ = r.generate_rays_surface(points, rng, cosine)
            shadow_rays, shadow_after, _, rejected = ptss.probe_surface_rays(tri, sph, points, rng, cosine)
            assert rejected == 0 and same_bytes(rays, shadow_rays) and same_bytes(after, shadow_after)
            results, rng = r.trace_paths(rays, after, 3)
            dev = r.accumulate_paths_linear(results, dev, index=texels, params=film)
            host = ptss.probe_accumulate_linear(results, host, index=texels, params=film)[0]
        for _ in range(2):
            dev, host = r.dilate_linear(dev, W, H), ptss.probe_dilate_linear(host, W, H)
        assert same_bytes(dev, host) and (host["samples"][texels] == 2).all()
        _, hits = camera_hits(r, 32, 24)
        assert {0, 1, 2} >= set(hits["kind"].tolist()) and (hits["kind"] == 1).any() and (hits["kind"] == 2).any()
        for filter in FILTERS:
            params = lm_params(W, H, filter, (True, True))
            view, info = r.lookup_lightmap(hits, dev, params, bt, bs, film=film)
            shadow, counts = ptss.probe_lookup_lightmap(mat, hits, host, params, bt, bs, film=film)
            assert same_bytes(view, shadow), first_difference(view, shadow)
            assert np.array_equal(info, counts) and info[REJECTED] == 0 and info[FILTERED] == (hits["kind"] != 0).sum()
            lit = view["samples"] == 1
            assert view["r"][lit & (hits["kind"] == 1)].any() and view["r"][lit & (hits["kind"] == 2)].any()   # both kinds carry baked light
            histogram = r.meter_linear(view)
            assert np.array_equal(histogram, ptss.probe_meter_linear(shadow))
            assert same_bytes(r.meter_exposure(histogram, params=film), ptss.probe_meter_exposure(histogram, params=film))
            got = r.resolve_linear(view, params=film)
            want = ptss.probe_resolve_linear(shadow, params=film)
            for a, b in zip(got, want):
                assert same_bytes(a, b)
    finally:
        r.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    buf = C.c_void_p()
    assert Hip.hipMalloc(C.byref(buf), 1 << 16) == 0
    try:
        before = r.lightmap_launches()
        d = buf.value
        ok, film = ptss.lightmap_params(8, 8, num_triangle_blocks=4, num_sphere_blocks=4), ptss.linear_params()
        look = lambda params=ok, film=film, bt=d, bs=d + 1024, map_=d + 2048, hits=d + 8192, n=8, out=d + 16384, info=d + 32768, ctx=r._ctx: \
            L.ptss_lookup_lightmap(ctx, C.byref(params) if params is not None else None, C.byref(film) if film is not None else None, bt, bs, map_, hits,
                                   n, out, info, None)
        assert look(ctx=None) == EINVAL and look(params=None) == EINVAL and look(film=None) == EINVAL
        assert look(map_=None) == EINVAL and look(hits=None) == EINVAL and look(out=None) == EINVAL
        assert look(bt=None) == EINVAL and look(bs=None) == EINVAL   # a table may be NULL only with a count of 0
        for change in (dict(structSize=36), dict(filter=2), dict(filter=-1), dict(flags=4), dict(flags=8 | 1), dict(reserved=1)):
            p = ptss.lightmap_params(8, 8, num_triangle_blocks=4, num_sphere_blocks=4)
            for k, v in change.items():
                setattr(p, k, v)
            assert look(params=p) == EINVAL, change
        bad_film = ptss.linear_params()
        bad_film.structSize = 4
        assert look(film=bad_film) == EINVAL
        for name in ("bt", "bs", "map_", "hits", "out"):
            base = dict(bt=d, bs=d + 1024, map_=d + 2048, hits=d + 8192, out=d + 16384)[name]
            assert look(**{name: base + 8}) == EINVAL, name
        assert look(info=d + 32768 + 2) == EINVAL
        assert look(out=d + 2048) == EINVAL and look(out=d + 2048 + 32 * 63) == EINVAL and look(out=d + 2048 - 32 * 7) == EINVAL   # overlaps the map
        assert look(n=1 << 31) == ERANGE
        for change in (dict(atlasWidth=0), dict(atlasHeight=0), dict(atlasWidth=-8), dict(atlasWidth=1 << 16, atlasHeight=1 << 15), dict(firstTriangle=-1),
                       dict(numTriangleBlocks=-1), dict(firstSphere=-1), dict(numSphereBlocks=-1)):
            p = ptss.lightmap_params(8, 8, num_triangle_blocks=4, num_sphere_blocks=4)
            for k, v in change.items():
                setattr(p, k, v)
            assert look(params=p) == ERANGE, change
        assert look(n=0, map_=None, hits=None, out=None) == 0   # n = 0 returns OK
        assert L.ptss_debug_lightmap_form(r._ctx, 3) == EINVAL and L.ptss_debug_lightmap_form(r._ctx, -1) == EINVAL
        assert L.ptss_lightmap_launches(r._ctx, None) == EINVAL
        assert r.lightmap_launches() == before
        # the wrapper's own checks
        with pytest.raises(ValueError):
            r.lookup_lightmap(np.zeros(2, dtype=ptss.HIT_DTYPE), np.zeros(5, dtype=ptss.LINEAR_DTYPE), ptss.lightmap_params(2, 2))
        assert r.lightmap_launches() == before
    finally:
        Hip.hipFree(buf)
        r.close()
