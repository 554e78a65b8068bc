"""The film of a path query on the GPU (ptss_generate_rays / ptss_accumulate_paths / ptss_ray_features).

1. The frame identity, the main pin: a pinhole film of the frame's size, fed ptss_seed_path_rng(seed, 0, skip 0) and run generate ->
   trace -> accumulate three times, leaves after every round the oracle's accumulator, display pixels and stream states of that
   frame, and a live context's own — bit for bit, for eight scenes, maxIterations 1, 2, 4, 8, the image staged in LDS and read in place.
2. The device's rays equal the host build of csrc/ptcamera.h byte for byte. 3. Accumulation equals the host probe.
4. ptss_ray_features against ptss_intersect + a material lookup and against ptss_render_features. 5. No trace in frame state; shards.
6. Refusals. 7. An equirect film through the denoiser.
The identity's cases keep the loop guard silent in every frame used, which tests/test_film_cpu.py checks."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from film_common import BATCHES, FILM_SIZES, ROUNDS, adversarial_radiance, films, frames_of, results_of, seeded_states, words
from path_query_common import H, ITERATIONS, N, SCENES, W, camera_of, eye_rays, make_scene, satisfies_identity_condition
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


def same_words(a, b):
    """Equal 32-bit words, a NaN standing for any NaN."""
    a, b = words(a), words(b)
    if a.shape != b.shape:
        return False
    fa, fb = a.view(np.float32), b.view(np.float32)
    return bool(((a == b) | (np.isnan(fa) & np.isnan(fb))).all())


# ---- 1. the frame identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
@pytest.mark.parametrize("name", list(SCENES))
def test_frame_identity(name, placement):
    _, every, _, seed = SCENES[name]
    scene, cam = make_scene(name, placement), camera_of(name)
    r = ptss.Renderer(scene, W, H, max_iterations=8, seed=seed, every_sphere_loop=every)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    for iterations in ITERATIONS:
        what = (name, placement, iterations)
        f = frames_of(name, iterations)
        rng = r.seed_path_rng(N, seed, 0, skip=0)
        film = np.zeros(N, dtype=ptss.FILM_DTYPE)
        r.set_max_iterations(iterations)
        r.reseed(seed)   # the context's streams as created, and a reset: the next frame is a first frame
        for k in range(ROUNDS):
            assert satisfies_identity_condition(f.live_counts[k], iterations), what
            rays, rng = r.generate_rays(film_cam, rng)
            if k == 0:
                assert np.array_equal(words(rays), words(eye_rays(cam, seed))), what   # the frame's own eye rays
            res, rng = r.trace_paths(rays, rng, iterations)
            film, pixels, history = r.accumulate_paths(res, film, pixels=True, history=True)
            assert np.array_equal(words(film)[:, :3], f.accum[k]), (what, k)
            assert (film["samples"] == k + 1).all(), (what, k)
            assert np.array_equal(pixels, f.pixels[k]), (what, k)
            assert np.array_equal(words(rng), f.states[k]), (what, k)
            assert (history["weight"] == k + 1).all()
            # ... and a live context's own frame
            r.generate_frame()
            assert np.array_equal(r.live_counts(), f.live_counts[k]), (what, k)
            assert np.array_equal(words(film)[:, :3], r.accumulator()) and np.array_equal(pixels, r.pixels()), (what, k)
            for p in (0, N // 2 + 7, N - 1):
                assert np.array_equal(r.rng_state(p), words(rng)[p]), (what, k, p)
    assert r.film_launches() == (len(ITERATIONS) * ROUNDS, len(ITERATIONS) * ROUNDS, 0) and r.film_rejected() == 0
    r.close()


# ---- 2. the device's rays are the host probe's ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


@pytest.mark.parametrize("width,height", FILM_SIZES)
def test_rays_equal_the_host_probe(small, width, height):
    r, P, seed = small, width * height, 0xF11
    for film in films(width, height):
        what = (width, height, film.kind, film.jitter)
        s0 = seeded_states(seed, P)
        rays, after = r.generate_rays(film, s0)   # the whole film
        want_rays, want_after, _ = ptss.probe_film_rays(film, s0)
        assert np.array_equal(words(rays), words(want_rays)) and np.array_equal(words(after), words(want_after)), what
        if not film.jitter:
            assert np.array_equal(words(after), s0), what
    if (width, height) != (64, 48):
        return
    g = np.random.default_rng(4)
    marked = np.full((P, 8), 7.5, dtype=np.float32)
    before = r.film_rejected()
    dropped = 0
    for film in films(width, height):
        what = (film.kind, film.jitter)
        for n in BATCHES:   # parts of the film that end inside a wave, from a first pixel > 0
            s0 = seeded_states(seed + n, n)
            rays, after = r.generate_rays(film, s0, first_pixel=P - n - 5)
            want_rays, want_after, _ = ptss.probe_film_rays(film, s0, first_pixel=P - n - 5)
            assert np.array_equal(words(rays), words(want_rays)) and np.array_equal(words(after), words(want_after)), (what, n)
        s0 = seeded_states(seed, P)
        perm = g.permutation(P).astype(np.uint32)   # a permuted index ...
        rays, after = r.generate_rays(film, s0, index=perm)
        want_rays, want_after, _ = ptss.probe_film_rays(film, s0, index=perm)
        assert np.array_equal(words(rays), words(want_rays)) and np.array_equal(words(after), words(want_after)), what
        wild = perm.copy()   # ... and one with entries beyond the film: not written, counted
        out = g.choice(P, 333, replace=False)
        wild[out] = g.choice([P, P + 1, 2 ** 31, 2 ** 32 - 1], 333)
        rays, after = r.generate_rays(film, s0, index=wild, rays=marked)
        want_rays, want_after, rejected = ptss.probe_film_rays(film, s0, index=wild, rays=marked)
        assert rejected == 333
        dropped += 333
        assert np.array_equal(words(rays), words(want_rays)) and np.array_equal(words(after), words(want_after)), what
        assert (words(rays)[out] == words(marked)[out]).all() and np.array_equal(words(after)[out], s0[out]), what
        assert r.film_rejected() == before + dropped, what


# ---- 3. accumulation is the host probe's -------------------------------------------------------------------------------------------------
def test_accumulate_equals_the_host_probe(small):
    r, g = small, np.random.default_rng(9)
    rad = adversarial_radiance()
    M, P = len(rad), W * H
    more = np.concatenate([rad, g.uniform(0, 1.2, (P - M, 3)).astype(np.float32) ** 3])   # one row per film pixel
    res = results_of(more)
    start = np.zeros(P, dtype=ptss.FILM_DTYPE)
    px0, hs0 = np.full((P, 4), 9, np.uint8), np.full((P, 4), -2.0, np.float32)
    before = r.film_rejected()

    def check(what, n, **kw):
        nonlocal before
        for pixels, history in ((px0, hs0), (px0, None), (None, hs0), (None, None)):   # each combination of the two outputs
            film, px, hs = r.accumulate_paths(res[:n], start, pixels=pixels, history=history, **kw)
            want, want_px, want_hs, rejected = ptss.probe_accumulate(res[:n], start, pixels=pixels, history=history, **kw)
            assert np.array_equal(words(film), words(want)), what
            assert (px is None) == (pixels is None) and (hs is None) == (history is None)
            assert px is None or np.array_equal(px, want_px), what
            assert hs is None or same_words(hs, want_hs), what
            before += rejected
            assert r.film_rejected() == before, what
        return film, px, hs

    film, _, _ = check("identity map", P)
    assert (film["samples"] == 1).all()
    for n in BATCHES:   # a part of the film: the rest stays untouched
        film, px, hs = r.accumulate_paths(res[:n], start, first_pixel=1000, pixels=px0, history=hs0)
        want, want_px, want_hs, _ = ptss.probe_accumulate(res[:n], start, first_pixel=1000, pixels=px0, history=hs0)
        assert np.array_equal(words(film), words(want)) and np.array_equal(px, want_px) and same_words(hs, want_hs), n
        rest = np.ones(P, bool)
        rest[1000:1000 + n] = False
        assert (film["samples"][rest] == 0).all() and (px[rest] == 9).all() and (words(hs)[rest].view(np.float32) == -2.0).all(), n
    check("permuted index", P, index=g.permutation(P).astype(np.uint32))
    film, _, _ = check("300 rays onto one pixel", 300, index=np.full(300, 1234, np.uint32))
    assert film["samples"][1234] == 300 and film["samples"].sum() == 300
    few = g.integers(0, 40, P).astype(np.uint32) * 77
    film, px, hs = check("many to few", P, index=few)
    untouched = np.ones(P, bool)
    untouched[few] = False
    assert (film["samples"][untouched] == 0).all() and (px is None or (px[untouched] == 9).all())
    wild = g.integers(0, P, P).astype(np.uint32)
    wild[::7] = P + g.integers(0, 5, len(wild[::7]))
    check("entries beyond the film", P, index=wild)
    # a film carried over several calls, with and without an index
    film, want = start, start
    for k in range(4):
        index = None if k % 2 == 0 else g.integers(0, P, P).astype(np.uint32)
        rows = results_of(g.permutation(more))
        film, px, hs = r.accumulate_paths(rows, film, index=index, pixels=True, history=True)
        want, want_px, want_hs, _ = ptss.probe_accumulate(rows, want, index=index, pixels=True, history=True)
        assert np.array_equal(words(film), words(want)) and np.array_equal(px, want_px) and same_words(hs, want_hs), k
    assert film["samples"].sum() == 4 * P


# ---- 4. features of arbitrary rays ---------------------------------------------------------------------------------------------------------
def arbitrary_rays(n, seed=5):
    """n rays around and through the closed box of the "mixed" preset: from inside and outside, four fifths towards its inside, a fifth
    anywhere (from outside, most of those miss); some with zero and non-finite components."""
    g = np.random.default_rng(seed)
    o = g.uniform([-9, -8, -14], [9, 8, 4], size=(n, 3))   # the box is [-5, 5]^2 x [-10, 0]: most origins lie outside it
    target = g.uniform([-4.5, -4.5, -9.5], [4.5, 4.5, -0.5], size=(n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::5] = g.normal(size=(len(d[::5]), 3))   # not normalised, anywhere
    rays = ptss.make_rays(o, d, np.float32(0.25))   # tmax is ignored: a feature is the hit at any distance
    rays[7, 4:7] = 0
    rays[8, 4] = 0
    rays[9, 5:7] = 0
    rays[10, 0] = np.nan
    rays[11, 4] = np.inf
    rays[12, 5] = -np.inf
    rays[13, 2] = np.inf
    rays[14, 6] = np.nan
    return rays


@pytest.mark.parametrize("placement", ["lds", "in_place"])
@pytest.mark.parametrize("name", ["mixed", "point_light", "mesh", "many_spheres", "every_sphere_loop"])
def test_ray_features(name, placement):
    _, every, _, seed = SCENES[name]
    scene, cam = make_scene(name, placement), camera_of(name)
    scene.desc.defaultColor.x, scene.desc.defaultColor.y, scene.desc.defaultColor.z = 0.25, 0.5, 0.125
    r = ptss.Renderer(scene, W, H, max_iterations=2, seed=seed, every_sphere_loop=every)
    r.set_camera(cam)
    rays = arbitrary_rays(4096)
    feat = r.ray_features(rays)
    at_inf = rays.copy()
    at_inf[:, 3] = INF
    hits = r.intersect(at_inf)
    miss = hits["kind"] == 0
    assert miss.sum() > 50 and (hits["kind"] == 1).sum() > 50 and (hits["kind"] == 2).sum() > 500, name
    assert same_words(feat["normal"], hits["normal"]) and same_words(feat["depth"].reshape(-1, 1), hits["distance"].reshape(-1, 1)), name
    assert np.array_equal(feat["materialIdx"], hits["materialIdx"]), name
    albedo = np.array([[m.diffuseColor.x, m.diffuseColor.y, m.diffuseColor.z] for m in
                       (scene.desc.materials[int(k)] for k in np.where(miss, 0, hits["materialIdx"]))], dtype=np.float32)
    albedo[miss] = (0.25, 0.5, 0.125)
    assert np.array_equal(words(feat["albedo"]), words(albedo)), name
    assert (feat["materialIdx"][miss] == -1).all() and (feat["depth"][miss] == INF).all() and (feat["normal"][miss] == 0).all()
    # of the jitter = 0 pinhole rays of the context's camera it is ptss_render_features, byte for byte
    centre, _ = r.generate_rays(ptss.film_camera("pinhole", W, H, cam, jitter=0), np.zeros((N, 6), np.uint32))
    assert np.array_equal(words(r.ray_features(centre)), words(r.features())), name
    assert r.film_launches() == (1, 0, 2)
    r.close()


# ---- 5. no trace in frame state; sharded contexts ----------------------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    twin = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)   # frames only
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    film_cam = ptss.film_camera("thinlens", 80, 30, cam, lens_radius=0.1, focus_distance=5.0)   # a film of its own shape
    P = 80 * 30
    s0 = r.seed_path_rng(P, 99)
    want_rays, want_rng, _ = ptss.probe_film_rays(film_cam, s0)
    want_feat = r.ray_features(want_rays)   # before the first frame
    res = results_of(np.random.default_rng(1).uniform(0, 1, (P, 3)).astype(np.float32))
    want_film, want_px, _, _ = ptss.probe_accumulate(res, np.zeros(P, ptss.FILM_DTYPE), pixels=True)
    side = torch.cuda.Stream()
    d_res = torch.from_numpy(words(res).view(np.float32).copy()).cuda()
    for tick in range(20):
        r.generate_frame()
        twin.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        rays, rng = r.generate_rays(film_cam, s0)   # on the context's stream
        film, px, _ = r.accumulate_paths(res, np.zeros(P, ptss.FILM_DTYPE), pixels=True)
        assert np.array_equal(words(rays), words(want_rays)) and np.array_equal(words(rng), words(want_rng)), tick
        assert np.array_equal(words(film), words(want_film)) and np.array_equal(px, want_px), tick
        assert same_words(r.ray_features(rays), want_feat), tick
        with torch.cuda.stream(side):   # and on a second one
            d_rng = torch.from_numpy(words(s0).view(np.int32).copy()).cuda()
            d_rays = r.generate_rays(film_cam, d_rng)
            d_feat = r.ray_features(d_rays)
            d_film = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
            d_px = torch.zeros((P, 4), dtype=torch.uint8, device="cuda")
            r.accumulate_paths(d_res, d_film, pixels=d_px)
        side.synchronize()
        assert np.array_equal(d_rays.cpu().numpy().view(np.uint32), words(want_rays)), tick
        assert np.array_equal(d_rng.cpu().numpy().view(np.uint32), words(want_rng)), tick
        assert same_words(d_feat.cpu().numpy(), want_feat), tick
        assert np.array_equal(d_film.cpu().numpy().view(np.uint32), words(want_film)) and np.array_equal(d_px.cpu().numpy(), want_px), tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "twenty frames with the three film calls after each", W, H, 1)
    assert r.launched_kernels() == twin.launched_kernels()   # what the frames alone set
    assert r.film_launches() == (40, 40, 41) and twin.film_launches() == (0, 0, 0) and r.film_rejected() == 0
    twin.close()
    o.close()
    r.close()


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_a_sharded_context_answers_as_the_unsharded_one(name):
    _, every, _, seed = SCENES[name]
    scene, cam = make_scene(name), camera_of(name)
    film_cam = ptss.film_camera("pinhole", W, H, cam)
    f = frames_of(name, 4)
    rays = arbitrary_rays(1000)
    whole = None
    for rank in (None, 0, 1):
        tile = {} if rank is None else dict(tile_rank=rank, tile_world=2, band_rows=8)
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, every_sphere_loop=every, **tile)
        eye, rng = r.generate_rays(film_cam, r.seed_path_rng(N, seed))   # all of the film, whatever rows the shard owns
        res, rng = r.trace_paths(eye, rng, 4)
        film, pixels, _ = r.accumulate_paths(res, np.zeros(N, ptss.FILM_DTYPE), pixels=True)
        assert np.array_equal(words(film)[:, :3], f.accum[0]) and np.array_equal(pixels, f.pixels[0]) and np.array_equal(words(rng), f.states[0]), (name, rank)
        feat = r.ray_features(rays)
        if whole is None:
            whole = feat
        assert same_words(feat, whole), (name, rank)
        assert r.film_launches() == (1, 1, 1)
        r.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n, P = 300, 20 * 15
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("f_rays", n * 32), ("f_rng", n * 24), ("f_res", n * 16), ("f_film", P * 16), ("f_pix", P * 4), ("f_hist", P * 16), ("f_feat", n * 32),
             ("f_index", n * 4))
    d_rays, d_rng, d_res, d_film, d_pix, d_hist, d_feat, d_index = (r._device_buffer(name, size + 16) for name, size in sizes)
    for (_, size), dev in zip(sizes, (d_rays, d_rng, d_res, d_film, d_pix, d_hist, d_feat, d_index)):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    good = ptss.film_camera("thinlens", 20, 15, lens_radius=0.1, focus_distance=3.0)
    gen = lambda ctx, film, first, index, count, rng, rays: L.ptss_generate_rays(ctx, C.byref(film) if film is not None else None, first, index, count, rng, rays, None)
    acc = lambda ctx, res, index, first, count, film, pixels, px, hs: L.ptss_accumulate_paths(ctx, res, index, first, count, film, pixels, px, hs, None)
    feat = lambda ctx, rays, out, count: L.ptss_ray_features(ctx, rays, out, count, None)
    assert gen(r._ctx, good, 0, None, n, d_rng, d_rays) == 0
    assert acc(r._ctx, d_res, None, 0, n, d_film, P, d_pix, d_hist) == 0
    assert feat(r._ctx, d_rays, d_feat, n) == 0
    r.synchronize()
    counters, kernels = r.film_launches(), r.launched_kernels()
    assert counters == (1, 1, 1) and r.film_rejected() == 0

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, (d_rays, d_rng, d_res, d_film, d_pix, d_hist, d_feat, d_index)):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    # ptss_generate_rays
    assert gen(None, good, 0, None, n, d_rng, d_rays) == EINVAL and gen(r._ctx, None, 0, None, n, d_rng, d_rays) == EINVAL
    assert gen(r._ctx, good, 0, None, n, None, d_rays) == EINVAL and gen(r._ctx, good, 0, None, n, d_rng, None) == EINVAL
    changes = [dict(structSize=64), dict(structSize=0), dict(kind=3), dict(kind=-1), dict(jitter=2), dict(jitter=-1), dict(width=0), dict(height=0),
               dict(width=-20), dict(lensRadius=-0.5), dict(lensRadius=float("inf")), dict(lensRadius=float("nan")), dict(focusDistance=0.0),
               dict(focusDistance=-1.0), dict(focusDistance=float("inf")), dict(focusDistance=float("nan"))]
    for change in changes:
        film = ptss.film_camera("thinlens", 20, 15, lens_radius=0.1, focus_distance=3.0)
        for k, v in change.items():
            setattr(film, k, v)
        assert gen(r._ctx, film, 0, None, n, d_rng, d_rays) == EINVAL, change
    for k in (4, 8, 12):
        assert gen(r._ctx, good, 0, None, n, d_rng, off(d_rays, k)) == EINVAL, k
    for k in (1, 2, 3):
        assert gen(r._ctx, good, 0, None, n, off(d_rng, k), d_rays) == EINVAL, k
        assert gen(r._ctx, good, 0, off(d_index, k), n, d_rng, d_rays) == EINVAL, k
    for count in (2 ** 31, 2 ** 40):
        assert gen(r._ctx, good, 0, d_index, count, d_rng, d_rays) == ERANGE, count
    assert gen(r._ctx, ptss.film_camera("pinhole", 2 ** 16, 2 ** 15), 0, None, n, d_rng, d_rays) == ERANGE   # width * height = 2^31
    for first, count in ((1, P), (P, 1), (P + 1, 0 + 1), (2 ** 63, 2), (P - n + 1, n)):
        assert gen(r._ctx, good, first, None, count, d_rng, d_rays) == ERANGE, (first, count)
    assert gen(r._ctx, good, 0, None, 0, None, None) == 0   # n = 0
    # ptss_accumulate_paths
    assert acc(None, d_res, None, 0, n, d_film, P, d_pix, d_hist) == EINVAL
    assert acc(r._ctx, None, None, 0, n, d_film, P, d_pix, d_hist) == EINVAL and acc(r._ctx, d_res, None, 0, n, None, P, d_pix, d_hist) == EINVAL
    for k in (4, 8, 12):
        assert acc(r._ctx, off(d_res, k), None, 0, n, d_film, P, d_pix, d_hist) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, off(d_film, k), P, d_pix, d_hist) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, d_film, P, d_pix, off(d_hist, k)) == EINVAL, k
    for k in (1, 2, 3):
        assert acc(r._ctx, d_res, off(d_index, k), 0, n, d_film, P, d_pix, d_hist) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, d_film, P, off(d_pix, k), d_hist) == EINVAL, k
    assert acc(r._ctx, d_res, d_index, 0, 2 ** 31, d_film, P, d_pix, d_hist) == ERANGE
    assert acc(r._ctx, d_res, d_index, 0, n, d_film, 2 ** 31, d_pix, d_hist) == ERANGE
    for first, count, pixels in ((1, n, n), (P - n + 1, n, P), (P, 1, P), (0, n, n - 1), (2 ** 63, 2, P)):
        assert acc(r._ctx, d_res, None, first, count, d_film, pixels, d_pix, d_hist) == ERANGE, (first, count, pixels)
    assert acc(r._ctx, None, None, 0, 0, None, P, None, None) == 0   # n = 0
    # ptss_ray_features
    assert feat(None, d_rays, d_feat, n) == EINVAL and feat(r._ctx, None, d_feat, n) == EINVAL and feat(r._ctx, d_rays, None, n) == EINVAL
    for k in (4, 8, 12):
        assert feat(r._ctx, off(d_rays, k), d_feat, n) == EINVAL and feat(r._ctx, d_rays, off(d_feat, k), n) == EINVAL, k
    assert feat(r._ctx, d_rays, d_feat, 2 ** 31) == ERANGE
    assert feat(r._ctx, None, None, 0) == 0   # n = 0
    out3, one = (C.c_ulonglong * 3)(), C.c_ulonglong()
    assert L.ptss_film_launches(None, out3) == EINVAL and L.ptss_film_launches(r._ctx, None) == EINVAL
    assert L.ptss_film_rejected(None, C.byref(one)) == EINVAL and L.ptss_film_rejected(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.film_launches() == counters and r.launched_kernels() == kernels and r.film_rejected() == 0
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 4-byte aligned streams, indices and pixels, NULL outputs, the last pixels of the film
    assert gen(r._ctx, good, P - 7, None, 7, off(d_rng, 4), d_rays) == 0
    assert acc(r._ctx, d_res, off(d_index, 4), 0, n - 1, d_film, P, off(d_pix, 4), None) == 0
    assert acc(r._ctx, d_res, None, P - 7, 7, d_film, P, None, None) == 0
    r.synchronize()
    assert r.film_launches() == (2, 3, 1) and r.launched_kernels() == kernels and r.film_rejected() == 0
    r.close()


# ---- 7. a panorama through the denoiser ----------------------------------------------------------------------------------------------------
def test_an_equirect_film_feeds_the_denoiser():
    name = "mixed"
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name), W, H, max_iterations=4, seed=seed)   # a context of the film's size: the denoiser's frame
    pano = ptss.film_camera("equirect", W, H, cam)
    rng = r.seed_path_rng(N, seed)
    film = np.zeros(N, dtype=ptss.FILM_DTYPE)
    for _ in range(2):
        rays, rng = r.generate_rays(pano, rng)
        res, rng = r.trace_paths(rays, rng, 4)
        film, pixels, history = r.accumulate_paths(res, film, pixels=True, history=True)
    centre, _ = r.generate_rays(ptss.film_camera("equirect", W, H, cam, jitter=0), rng)
    feat = r.ray_features(centre)
    assert (feat["materialIdx"] >= 0).mean() > 0.99   # a closed box: a panorama sees a surface (nearly) everywhere
    assert len(np.unique(pixels[:, :3], axis=0)) > 100 and (history["weight"] == 2).all()
    for levels in (0, 3):
        params = ptss.default_denoise_params(levels=levels)
        want, _ = ptss.probe_denoise_history(history, feat, W, H, params)
        got = r.denoise_history(history=history, features=feat, levels=levels)
        assert np.array_equal(got, want), levels
        if levels == 0:
            assert np.array_equal(got, pixels)   # unfiltered: the film's own display pixels
    r.close()
