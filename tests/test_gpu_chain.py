"""Ray queries that follow mirrors and glass on the GPU (ptss_intersect_chain, ptss_lookup_lightmap_chain).

1. The device equals the composition — a Python loop of Renderer.intersect and ptss_probe_specular_link (the host build of
csrc/ptspecular.h) — byte for byte: hits, throughput, steps, direction, pathLength; maxSteps 0, 1, 2 and 8, three cameras, six scenes,
with and without cfg.everySphereLoop, the first link's tmax +inf and a finite one that cuts some first hits off. 2. maxSteps = 0 is
ptss_intersect. 3. On a camera's centre rays the chain is ptss_render_features_specular's. 4. The refill schedule equals one lane per
ray for every grid, on shuffled rays, with the image in LDS and in place. 5. A live mesh after ptss_update_triangles and
ptss_resort_triangles. 6. No trace in frame state, in ptss_launched_kernels or in the path queries' refill queue; the launch counters.
7. The refusals. 8. The tinted lookup: the device equals the host probe on the view of `mixed`, a throughput of ones is the plain lookup,
and a pixel seen in a flagged mirror is the directly looked-up row times the mirror's factor."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from lightmap_common import FILTERED, modulate_weight
from scene_update_common import deform
from surface_common import first_difference, same_bytes
from test_gpu_denoise import far_camera, moved_camera
from test_gpu_kernel_coverage import compare
from test_gpu_specular_features import SCENES

pytestmark = pytest.mark.gpu

W, H = 37, 23   # 851 rays = 14 waves, the last one partly filled
N = W * H
STEPS = (0, 1, 2, 8)
F32 = np.float32
_RAYS = {}


def camera_rays(name, cam):
    """The centre rays of a W x H frame, computed once per camera."""
    if name not in _RAYS:
        _RAYS[name] = ptss.camera_rays(cam, W, H)
    return _RAYS[name].copy()


CAMERAS = (("default", ptss.default_camera), ("moved", moved_camera), ("far", far_camera))


def composed(r, desc, rays, max_steps):
    """The chain as a composition: ptss_intersect of the live rays, ptss_probe_specular_link of their hits, at most max_steps + 1 times.
    -> (hits, chain, what happened: a dict of counts)."""
    n = len(rays)
    cur = np.ascontiguousarray(rays, dtype=F32).copy()
    hits_out = np.zeros(n, dtype=ptss.HIT_DTYPE)
    chain = np.zeros(n, dtype=ptss.CHAIN_DTYPE)
    through = np.ones((n, 3), dtype=F32)
    length = np.full(n, np.inf, dtype=F32)
    steps = np.zeros(n, dtype=np.uint32)
    live = np.ones(n, dtype=bool)
    classes = np.array([ptss.SPECULAR_CLASSES.index(ptss.specular_class(desc.materials[k])) for k in range(desc.numMaterials)])
    iors = np.array([desc.materials[k].indexOfRefraction for k in range(desc.numMaterials)], dtype=np.float64)
    seen = dict(tir_stopped=0, tir_reflected=0, refracted=0, mirrored=0, cut_off=0)
    for k in range(max_steps + 1):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        hits = r.intersect(cur[idx])
        hit = hits["kind"] != 0
        at, hh = idx[hit], hits[hit]
        length[idx[~hit]] = np.inf
        length[at] = hh["distance"] if k == 0 else length[at] + hh["distance"]   # float32, in chain order
        ended = np.ones(len(idx), dtype=bool)
        if k < max_steps and len(at):
            nxt, follows, factors = ptss.probe_specular_link(cur[at], hh, desc)
            cls, ior = classes[hh["materialIdx"]], iors[hh["materialIdx"]]
            cos = -(cur[at, 4:7].astype(np.float64) * hh["normal"]).sum(1)
            eta = np.where(cos > 0, 1.0 / ior, ior)
            tir = (cls == 1) & (eta * eta * (1 - cos * cos) > 1.001)
            seen["tir_stopped"] += int((tir & ~follows).sum())
            seen["tir_reflected"] += int((tir & follows).sum())
            seen["refracted"] += int(((cls == 1) & ~tir & follows).sum())
            seen["mirrored"] += int(((cls == 2) & follows).sum())
            ended[np.nonzero(hit)[0][follows]] = False
        done = idx[ended]
        hits_out[done] = hits[ended]
        chain["direction"][done], chain["pathLength"][done] = cur[done, 4:7], length[done]
        chain["throughput"][done], chain["steps"][done] = through[done], steps[done]
        live[:] = False
        if not ended.all():
            go = at[follows]
            through[go] = through[go] * factors[follows]   # float32, component by component, in chain order
            cur[go] = nxt[follows]
            steps[go] += 1
            live[go] = True
    return hits_out, chain, seen


def assert_same(got, want, what):
    (hits, chain), (want_hits, want_chain) = got, want
    assert same_bytes(hits, want_hits), (what, "hits", first_difference(hits, want_hits))
    for field in ("throughput", "steps", "direction", "pathLength"):
        assert chain[field].tobytes() == want_chain[field].tobytes(), (what, field, int((chain[field] != want_chain[field]).sum()))


# ---- 1., 2. the device equals the composition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every_sphere_loop", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_the_device_equals_the_composition(name, every_sphere_loop):
    scene = SCENES[name]()
    r = ptss.Renderer(scene, W, H, max_iterations=2, every_sphere_loop=every_sphere_loop)
    total, deepest, launches = {}, 0, 0
    for cam_name, make in CAMERAS:
        rays = camera_rays(cam_name, make())
        first = r.intersect(rays)
        finite = first["distance"][first["kind"] != 0]
        cut = rays.copy()
        if len(finite):
            cut[:, 3] = np.median(finite)   # a tmax that cuts about half of the first hits off
        for what, batch in (("inf", rays), ("finite tmax", cut)):
            plain = r.intersect(batch)
            for max_steps in STEPS:
                got = r.intersect_chain(batch, max_steps)
                launches += 1
                want_hits, want_chain, seen = composed(r, scene.desc, batch, max_steps)
                assert_same(got, (want_hits, want_chain), (name, cam_name, what, max_steps))
                assert got[1]["steps"].max(initial=0) <= max_steps
                if max_steps == 0:   # ptss_intersect's bytes
                    assert same_bytes(got[0], plain) and not got[1]["steps"].any() and (got[1]["throughput"] == 1).all()
                    assert got[1]["direction"].tobytes() == batch[:, 4:7].tobytes()
                miss = got[0]["kind"] == 0
                assert np.isposinf(got[1]["pathLength"][miss]).all() and np.isfinite(got[1]["pathLength"][~miss]).all()
                if cam_name != "far":
                    for k, v in seen.items():
                        total[k] = total.get(k, 0) + v
                    deepest = max(deepest, int(got[1]["steps"].max(initial=0)))
            if what == "finite tmax" and len(finite) and cam_name != "far":
                lost = (first["kind"] != 0) & (plain["kind"] == 0)
                assert lost.any() and (plain["kind"] != 0).any(), (name, cam_name)
                total["cut_off"] = total.get("cut_off", 0) + int(lost.sum())
    print(f"{name}: {total}, deepest chain {deepest}")
    # the cases are there for a reason: each reaches the branches it was chosen for
    assert total["cut_off"] > 0
    if name in ("default", "mixed"):
        assert total["refracted"] > 0 and total["mirrored"] > 0 and deepest >= 3
    if name == "cornell":
        assert total["refracted"] > 0 and total["mirrored"] > 0
    if name == "tir":
        assert total["tir_stopped"] > 0 and total["tir_reflected"] > 0 and total["refracted"] > 0 and total["mirrored"] > 0
    if name == "mirror_mesh":
        assert total["mirrored"] > 0
    assert r.chain_launches() == (launches, 0)
    # without dev_chain: the same hits; n = 0 launches nothing
    hits_only, none = r.intersect_chain(rays, 8, chain=False)
    assert none is None and same_bytes(hits_only, r.intersect_chain(rays, 8)[0])
    assert len(r.intersect_chain(rays[:0], 8)[0]) == 0 and r.chain_launches() == (launches + 2, 0)
    r.close()


# ---- 3. a camera's centre rays: the chain of ptss_render_features_specular ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "tir", "mirror_mesh"])
def test_centre_rays_give_the_specular_features(name):
    scene = SCENES[name]()
    r = ptss.Renderer(scene, W, H, max_iterations=2)
    for cam_name, make in CAMERAS[:2]:
        cam = make()
        r.set_camera(cam)
        rays = camera_rays(cam_name, cam)
        for max_steps in STEPS:
            feat, steps = r.features_specular(max_steps, steps=True)
            hits, chain = r.intersect_chain(rays, max_steps)
            assert np.array_equal(hits["materialIdx"], feat["materialIdx"]), (name, cam_name, max_steps)
            assert hits["normal"].tobytes() == feat["normal"].tobytes() and chain["pathLength"].tobytes() == feat["depth"].tobytes()
            assert np.array_equal(chain["steps"], steps)
        assert steps.any()
    r.close()


# ---- 4. the refill schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "in_place_484", "mirror_mesh", "tir"])
def test_refill_equals_lane_per_ray(name):
    torch = pytest.importorskip("torch")
    scene = SCENES[name]()
    r = ptss.Renderer(scene, W, H, max_iterations=2)
    rays = camera_rays("moved", moved_camera())
    rays = rays[np.random.default_rng(5).permutation(N)]   # neighbours in a wave no longer look the same way
    rays[::7, 3] = 2.5                                    # ... and some are cut short
    refills = 0
    for max_steps in (0, 3, 8):
        want = r.intersect_chain(rays, max_steps, schedule=None)   # options NULL: the default
        assert_same(r.intersect_chain(rays, max_steps, "lane"), want, (name, max_steps, "lane"))
        if max_steps and name != "in_place_484":   # chains of different lengths side by side (in "tir" the camera is inside the glass: every ray has one)
            assert want[1]["steps"].any() and (name == "tir" or (want[1]["steps"] == 0).any())
            assert len(set(want[1]["steps"].tolist())) > 1
        for cap in (1, 2, 0):   # one workgroup over 851 rays: every wave but the first four lives on refills
            assert_same(r.intersect_chain(rays, max_steps, "refill", cap), want, (name, max_steps, cap))
            refills += 1
        hits_only, none = r.intersect_chain(rays, max_steps, "refill", 1, chain=False)
        refills += 1
        assert none is None and same_bytes(hits_only, want[0])
    # device tensors, the current stream: the same bytes, nothing waited for in between
    d_rays = torch.from_numpy(rays).cuda()
    outs = [r.intersect_chain(d_rays, 8, "refill", cap) for cap in (1, 3, 0)] + [r.intersect_chain(d_rays, 8, "lane")]
    refills += 3
    for hits, chain in outs:
        assert hits.cpu().numpy().tobytes() == want[0].tobytes() and chain.cpu().numpy().tobytes() == want[1].tobytes()
    lane, refill = r.chain_launches()
    assert refill == refills and lane == 3 * 2 + 1
    r.close()


# ---- 5. a live scene ----------------------------------------------------------------------------------------------------------------------
def test_a_live_mesh_after_update_and_resort():
    scene = SCENES["mirror_mesh"]()
    r = ptss.Renderer(scene, W, H, max_iterations=2)
    assert r.triangle_leaves() > 0
    rays = camera_rays("default", ptss.default_camera())
    old = r.intersect_chain(rays, 4)
    assert old[1]["steps"].any()
    first = 16   # the icosphere's triangles follow the box's sixteen
    r.update_triangles(deform(ptss.scene_records(scene)[0][first:]), first=first)
    assert r.update_rejected() == 0
    moved = r.intersect_chain(rays, 4)
    assert not same_bytes(moved[0], old[0]) and moved[1]["steps"].any()
    assert_same(moved, composed(r, scene.desc, rays, 4)[:2], "moved")
    r.resort_triangles()
    r.synchronize()
    assert r.resort_launches() == 1
    for schedule, cap in (("lane", 0), ("refill", 1), ("refill", 0)):
        got = r.intersect_chain(rays, 4, schedule, cap)
        assert_same(got, composed(r, scene.desc, rays, 4)[:2], ("resorted", schedule, cap))
        assert np.array_equal(got[0]["primitive"], moved[0]["primitive"]) and got[1]["steps"].tobytes() == moved[1]["steps"].tobytes()
    r.close()


# ---- 6. no trace in frame state -----------------------------------------------------------------------------------------------------------
def test_frames_and_the_path_queue_are_untouched():
    torch = pytest.importorskip("torch")
    scene = ptss.Scene("mixed")
    w, h, bounces = 40, 24, 4
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces)
    rays = camera_rays("moved", moved_camera())
    d_rays = torch.from_numpy(rays).cuda()
    rng = r.seed_path_rng(N, 7)
    paths = r.trace_paths(rays, rng, 4, schedule="refill", max_workgroups=1)   # the path queries' queue exists and has counted
    stats = r.path_refill_stats()
    r.intersect_chain(rays, 3)   # before the first frame
    side = torch.cuda.Stream()
    for tick in range(8):
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        r.intersect_chain(d_rays, tick % 9, "refill" if tick & 1 else "lane", tick % 3)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):   # and on a second stream
            r.intersect_chain(d_rays, 8, "lane")
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    torch.cuda.synchronize()
    compare(r, o, "eight frames with a chain query after each", w, h, 1)
    assert r.chain_launches() == (1 + 4 + 8, 4)
    assert r.path_refill_stats() == stats and sum(r.path_launches()) == 0 and sum(r.specular_feature_launches()) == 0
    again = r.trace_paths(rays, rng, 4, schedule="refill", max_workgroups=1)
    assert same_bytes(again[0], paths[0]) and same_bytes(again[1], paths[1])
    r.close()
    o.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    buf = C.c_void_p()
    assert Hip.hipMalloc(C.byref(buf), 1 << 16) == 0
    try:
        d = buf.value
        n = 8   # rays 256 B, hits 384 B, chain 256 B
        refill = ptss.chain_options("refill", 1)

        def call(ctx=r._ctx, rays=d, n=n, max_steps=2, options=refill, hits=d + 1024, chain=d + 2048):
            return L.ptss_intersect_chain(ctx, rays, n, max_steps, C.byref(options) if options is not None else None, hits, chain, None)

        assert call(ctx=None) == EINVAL and call(rays=None) == EINVAL and call(hits=None) == EINVAL
        for field, value in (("structSize", 0), ("structSize", 20), ("schedule", 2), ("schedule", -1), ("reserved", 1), ("reserved", -1),
                             ("maxWorkgroups", -1)):
            bad = ptss.chain_options("refill", 1)
            setattr(bad, field, value)
            assert call(options=bad) == EINVAL, (field, value)
        for k in (4, 8):
            assert call(rays=d + k) == EINVAL and call(hits=d + 1024 + k) == EINVAL and call(chain=d + 2048 + k) == EINVAL, k
        assert call(hits=d) == EINVAL and call(hits=d + 240) == EINVAL and call(hits=d - 368) == EINVAL      # the hits overlap the rays
        assert call(chain=d + 16) == EINVAL and call(chain=d - 240) == EINVAL                                # the chain overlaps the rays
        assert call(chain=d + 1024) == EINVAL and call(chain=d + 1024 + 368) == EINVAL and call(chain=d + 1024 - 240) == EINVAL   # ... the hits
        for bad in (-1, 9, 2 ** 31 - 1, -2 ** 31):
            assert call(max_steps=bad) == ERANGE and call(max_steps=bad, options=None) == ERANGE, bad
        assert call(n=1 << 31) == ERANGE and call(n=(1 << 40)) == ERANGE
        assert L.ptss_chain_launches(r._ctx, None) == EINVAL and L.ptss_default_chain_options(None) == EINVAL
        assert r.chain_launches() == (0, 0)
        assert call(n=0, rays=None, hits=None, chain=None) == 0 and r.chain_launches() == (0, 0)   # n = 0 returns OK
        # the tinted lookup: ptss_lookup_lightmap's refusals, and the chain rows'
        ok, film = ptss.lightmap_params(8, 8, num_triangle_blocks=4, num_sphere_blocks=4), ptss.linear_params()

        def look(params=ok, film=film, bt=d, bs=d + 1024, map_=d + 2048, hits=d + 8192, chain=d + 12288, n=8, out=d + 16384, info=d + 32768, ctx=r._ctx):
            return L.ptss_lookup_lightmap_chain(ctx, C.byref(params) if params is not None else None, C.byref(film) if film is not None else None, bt,
                                                bs, map_, hits, chain, n, out, info, None)

        assert look(ctx=None) == EINVAL and look(params=None) == EINVAL and look(film=None) == EINVAL
        assert look(map_=None) == EINVAL and look(hits=None) == EINVAL and look(out=None) == EINVAL and look(chain=None) == EINVAL
        assert look(bt=None) == EINVAL and look(bs=None) == EINVAL
        for change in (dict(structSize=36), dict(filter=2), dict(flags=4), dict(reserved=1)):
            p = ptss.lightmap_params(8, 8, num_triangle_blocks=4, num_sphere_blocks=4)
            for k, v in change.items():
                setattr(p, k, v)
            assert look(params=p) == EINVAL, change
        for name, base in (("bt", d), ("bs", d + 1024), ("map_", d + 2048), ("hits", d + 8192), ("chain", d + 12288), ("out", d + 16384)):
            assert look(**{name: base + 8}) == EINVAL, name
        assert look(info=d + 32768 + 2) == EINVAL
        assert look(out=d + 2048) == EINVAL and look(out=d + 12288) == EINVAL and look(out=d + 12288 - 32 * 7) == EINVAL and look(out=d + 8192 + 48 * 7) == EINVAL
        assert look(n=1 << 31) == ERANGE
        for change in (dict(atlasWidth=0), dict(atlasWidth=1 << 16, atlasHeight=1 << 15), dict(numTriangleBlocks=-1), dict(firstSphere=-1)):
            p = ptss.lightmap_params(8, 8, num_triangle_blocks=4, num_sphere_blocks=4)
            for k, v in change.items():
                setattr(p, k, v)
            assert look(params=p) == ERANGE, change
        assert look(n=0, map_=None, hits=None, chain=None, out=None) == 0
        assert L.ptss_lightmap_chain_launches(r._ctx, None) == EINVAL
        assert r.lightmap_chain_launches() == 0 and r.lightmap_launches() == 0
    finally:
        Hip.hipFree(buf)
        r.close()


# ---- 8. the tinted lookup -----------------------------------------------------------------------------------------------------------------
def test_the_tinted_lookup_on_the_view_of_mixed():
    scene = ptss.Scene("mixed")
    tri, sph = ptss.scene_records(scene)
    mat = ptss.scene_materials(scene)
    w, h = 32, 24
    r = ptss.Renderer(scene, w, h, max_iterations=3, seed=0xBA4E)
    try:
        Wa = 64
        bt, bs, points, texels, Ha = ptss.surface_atlas_blocks(tri, sph, 1.5, Wa, 1, 16)
        film, cosine = ptss.linear_params(), ptss.surface_params("cosine")
        baked = np.zeros(Wa * Ha, dtype=ptss.LINEAR_DTYPE)
        rng = r.seed_path_rng(len(points), 0xBA4E)
        for _ in range(2):   # a small bake
            rays, rng, _ = r.generate_rays_surface(points, rng, cosine)
            results, rng = r.trace_paths(rays, rng, 3)
            baked = r.accumulate_paths_linear(results, baked, index=texels, params=film)
        baked = r.dilate_linear(baked, Wa, Ha)
        view_rays = r.generate_rays(ptss.film_camera("pinhole", w, h, None, jitter=0), np.zeros((w * h, 6), np.uint32))[0]
        first = r.intersect(view_rays)
        hits, chain = r.intersect_chain(view_rays, 4)
        assert chain["steps"].any() and (chain["steps"] == 0).any()
        for filter in ("nearest", "bilinear"):
            params = ptss.lightmap_params(Wa, Ha, filter, modulate=True, emission=True)
            got, info = r.lookup_lightmap(hits, baked, params, bt, bs, film=film, chain=chain)
            want, counts = ptss.probe_lookup_lightmap_chain(mat, hits, chain, baked, params, bt, bs, film=film)
            assert same_bytes(got, want), first_difference(got, want)
            assert np.array_equal(info, counts) and info[FILTERED] == (hits["kind"] != 0).sum()
            plain, plain_info = r.lookup_lightmap(hits, baked, params, bt, bs, film=film)
            assert np.array_equal(info, plain_info)   # the verdicts are the plain lookup's
            ones = chain.copy()
            ones["throughput"] = 1.0
            same, _ = r.lookup_lightmap(hits, baked, params, bt, bs, film=film, chain=ones)
            assert same_bytes(same, plain)
            # a pixel seen in a flagged mirror of known specAvg and specularColor: the directly looked-up row times that factor
            m = first["materialIdx"]
            flagged = (first["kind"] != 0) & (chain["steps"] == 1) & (mat["flags"][m] == 1) & (mat["refrAvg"][m] == 0) & (mat["diffAvg"][m] == 0)
            lit = flagged & (plain["samples"] == 1) & (plain["r"] > 16)
            assert lit.any(), "no pixel of the view looks into the mirror once and sees baked light"
            for i in np.nonzero(lit)[0]:
                factor = mat["specularColor"][m[i]].astype(F32) * F32(mat["specAvg"][m[i]])
                assert chain["throughput"][i].tobytes() == factor.tobytes()
                for c, ch in enumerate("rgb"):
                    assert int(got[ch][i]) == (int(plain[ch][i]) * modulate_weight(factor[c]) + 32768) >> 16, (i, ch)
            assert (got["r"][lit] < plain["r"][lit]).all()
        assert r.lightmap_chain_launches() == 4 and r.lightmap_launches() == 2
    finally:
        r.close()
