"""Carrying the linear films across a camera move on the GPU (ptss_reproject_linear). Every test requires the device
to equal the host probe byte for byte — film rows, moment rows and the four counters.

1. Every size, film kind, camera pair, with and without moments, features of real scenes, films of real rounds. 2. Inputs no film
holds. 3. Motion rows. 4. The loop rounds -> carry -> rounds into the seeded film -> plan, denoise, meter, glare, resolve -> a second
move, against a shadow loop of the probes. 5. Frames interleaved with the calls, a second stream, two shards. 6. Refusals. 7. Quality:
one round into the seeded film against one round into an empty one."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from lindenoise_common import corner_holes, first_difference, same_bytes, words
from linear_common import linear_film
from linstats_common import random_word_moments, zero_moments
from meter_common import state_equal
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from splat_common import splat_film
from test_gpu_kernel_coverage import compare
from test_linreproject_cpu import CAMERA_REFUSED, REPROJECT_REFUSED
from test_lindenoise_cpu import FILM_REFUSED, changed

pytestmark = pytest.mark.gpu
FILMS = ("linear", "splat")
SIZES = ((1, 1), (31, 7), (32, 8), (33, 9), (65, 17), (70, 37))
SIZE_PAIRS = [(s, s) for s in SIZES] + [((33, 9), (70, 37)), ((70, 37), (33, 9))]   # (now, previous)
# (now kind, previous kind, scene, move)
PAIRS = [("pinhole", "pinhole", "mixed", "df"), ("pinhole", "pinhole", "mesh", "wg"), ("thinlens", "thinlens", "cornell", "wg"),
         ("thinlens", "thinlens", "mixed", "df"), ("equirect", "equirect", "mesh", "df"), ("equirect", "equirect", "cornell", "wg"),
         ("equirect", "equirect", "mixed", "dfg"), ("pinhole", "equirect", "cornell", "df"), ("pinhole", "equirect", "mixed", "wg"),
         ("pinhole", "equirect", "mesh", "df"), ("equirect", "pinhole", "mixed", "wg"), ("equirect", "pinhole", "cornell", "df"),
         ("equirect", "pinhole", "mesh", "wg")]
ITERATIONS = 3
# Every pose A stands one 'w' step in front of the scene's camera (§3.19's reason: the presets' own camera position lies on a surface
# for a camera that steps sideways from it, and a first hit at distance 0 reprojects nowhere).
START = "w"


def moved(cam, keys):
    out = ptss.Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(ptss.Camera))
    for k in keys:
        assert ptss.move_camera(out, k)
    return out


def film_cameras(kind, w, h, cam):
    """(the jittered camera the rounds sample through, the centre-ray camera of the features) of one pose."""
    lens = dict(lens_radius=0.05, focus_distance=4.0)
    return ptss.film_camera(kind, w, h, cam, jitter=1, **lens), ptss.film_camera(kind, w, h, cam, jitter=0, **lens)


def centre_features(r, centre_cam, seed):
    P = centre_cam.width * centre_cam.height
    return r.ray_features(r.generate_rays(centre_cam, r.seed_path_rng(P, seed, 0, skip=0))[0])


def rounds(r, film_cam, seed, n, splat, params, film=None, moments=None, rng=None, shadow=None):
    """n rounds with stats through film_cam into (film, moments) (new ones where None) -> (film, moments, rng). shadow: (film, moments) of a
    shadow loop of the probes, advanced alongside and compared."""
    w, h = film_cam.width, film_cam.height
    P = w * h
    film = film if film is not None else (splat_film(P) if splat else linear_film(P))
    moments = moments if moments is not None else zero_moments(P)
    rng = rng if rng is not None else r.seed_path_rng(P, seed, 0, skip=0)
    flt = ptss.splat_filter("tent", 1.5)
    for _ in range(n):
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, ITERATIONS)
        if splat:
            film = r.splat_paths(res, pos, film, w, h, filter=flt, params=params, homed_first_pixel=0)
            moments = r.accumulate_paths_linear_stats(res, None, moments, params=params)[1]
            if shadow is not None:
                shadow[0] = ptss.probe_splat_paths(res, pos, shadow[0], w, h, filter=flt, params=params, homed_first_pixel=0)[0]
                shadow[1] = ptss.probe_accumulate_linear_stats(res, None, shadow[1], params=params)[1]
        else:
            film, moments = r.accumulate_paths_linear_stats(res, film, moments, params=params)
            if shadow is not None:
                shadow[0], shadow[1], _ = ptss.probe_accumulate_linear_stats(res, shadow[0], shadow[1], params=params)
        if shadow is not None:
            assert same_bytes(film, shadow[0]) and same_bytes(moments, shadow[1])
    return film, moments, rng


def punched(film, moments, w, h):
    """Empty pixels at the corners of the 32 x 8 tiles."""
    film, moments = film.copy(), moments.copy()
    if w * h >= 16:
        holes = corner_holes(w, h)
        words(film)[holes] = 0
        words(moments)[holes] = 0
    return film, moments


def check(r, now, fn, prev, fp, film, moments, params, reproject, what, motion=None, launches=None):
    got = r.reproject_linear(now, fn, prev, fp, film, moments, params, reproject, motion_now=motion)
    want = ptss.probe_reproject_linear(now, fn, prev, fp, film, moments, params, reproject, motion_now=motion)
    assert same_bytes(got[0], want[0]), (what, "film", first_difference(got[0], want[0]))
    if moments is not None:
        assert same_bytes(got[1], want[1]), (what, "moments", first_difference(got[1], want[1]))
    else:
        assert got[1] is None and want[1] is None
    assert got[2] == want[2], (what, got[2], want[2])
    assert int(got[2]["seeded"]) + int(got[2]["offFilm"]) + int(got[2]["noTap"]) == now.width * now.height, what
    if launches is not None:
        launches[0] += 1
        assert r.reproject_linear_launches() == launches[0], what
    return got


_RENDERERS = {}


@pytest.fixture(scope="module")
def renderer_of():
    def get(name):
        if name not in _RENDERERS:
            r = ptss.Renderer(make_scene(name), W, H, max_iterations=ITERATIONS, seed=SCENES[name][3])
            r.set_camera(camera_of(name))
            _RENDERERS[name] = r
        return _RENDERERS[name]
    yield get
    for r in _RENDERERS.values():
        r.close()
    _RENDERERS.clear()


# ---- 1. every size, kind, camera pair ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind_now,kind_prev,name,keys", PAIRS, ids=lambda v: str(v))
def test_the_seeded_film_equals_the_probe(renderer_of, kind_now, kind_prev, name, keys):
    """Tile edges (32 x 8), films of one pixel, films of different sizes; empty pixels at the tile corners; the features of a real scene
    from two poses; films and moments of real rounds; pixels seeded, off the film, disoccluded."""
    r = renderer_of(name)
    seed = SCENES[name][3]
    cam_a = moved(camera_of(name), START)
    cam_b = moved(cam_a, keys)
    params, reproject = ptss.linear_params(), ptss.reproject_linear_params()
    launches = [r.reproject_linear_launches()]
    seeded = empty = total = 0
    for k, ((wn, hn), (wp, hp)) in enumerate(SIZE_PAIRS):
        film_a, centre_a = film_cameras(kind_prev, wp, hp, cam_a)
        _, centre_b = film_cameras(kind_now, wn, hn, cam_b)
        fp, fn = centre_features(r, centre_a, seed), centre_features(r, centre_b, seed)
        for kind in FILMS:
            film, moments, _ = rounds(r, film_a, seed, 2 + k % 3, kind == "splat", params)
            film, moments = punched(film, moments, wp, hp)
            what = (kind_now, kind_prev, name, keys, (wn, hn), (wp, hp), kind)
            a = check(r, centre_b, fn, centre_a, fp, film, moments, params, reproject, what, launches=launches)
            b = check(r, centre_b, fn, centre_a, fp, film, None, params, reproject, what, launches=launches)
            assert same_bytes(a[0], b[0])
            seeded += int(a[2]["seeded"])
            empty += int(a[2]["noTap"]) + int(a[2]["offFilm"])
            total += wn * hn
    print(kind_now, kind_prev, name, keys, "seeded", seeded, "empty", empty)
    # the case is about seeded pixels and about empty ones. The narrowest pair is an equirect film looking at a pinhole one: a quarter of
    # its longitudes and about a third of its latitudes, 9 % of the sphere, less what the move hides: 3 % is asked of every pair
    assert seeded > 0.03 * total and empty > 0


# ---- 2. inputs no film holds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_broken_features_random_bytes_and_a_camera_far_away(renderer_of, kind):
    r = renderer_of("mixed")
    seed = SCENES["mixed"][3]
    g = np.random.default_rng(17)
    params = ptss.linear_params()
    for kn, kp, (wn, hn), (wp, hp) in (("pinhole", "pinhole", (70, 37), (70, 37)), ("equirect", "thinlens", (65, 17), (33, 9)), ("thinlens", "equirect", (33, 9), (65, 17))):
        cam_a = moved(camera_of("mixed"), START)
        cam_b = moved(cam_a, "df")
        _, centre_a = film_cameras(kp, wp, hp, cam_a)
        _, centre_b = film_cameras(kn, wn, hn, cam_b)
        fp, fn = centre_features(r, centre_a, seed).copy(), centre_features(r, centre_b, seed).copy()
        Pp = wp * hp
        junk_film = (g.integers(0, 2 ** 63, (Pp, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, (Pp, 4), dtype=np.uint64))
        junk_film[::3, 3] = g.integers(0, 9, len(junk_film[::3])) << (16 if kind == "splat" else 0)   # a third with counts a film holds
        junk_film[::3, :3] >>= np.uint64(30)
        junk_film = junk_film.view(ptss.SPLAT_DTYPE if kind == "splat" else ptss.LINEAR_DTYPE).reshape(-1)
        junk_moments = random_word_moments(Pp, g)
        what = (kind, kn, kp)
        check(r, centre_b, fn, centre_a, fp, junk_film, junk_moments, params, ptss.reproject_linear_params(max_history=(1 << 23) - 1), what + ("random bytes",))
        check(r, centre_b, fn, centre_a, fp, junk_film, junk_moments, ptss.linear_params(0, 2.0 ** 40), ptss.reproject_linear_params(cos_normal=-1.0, depth_tolerance=3e38, min_coverage=0.0), what + ("everything counts",))
        broken_n, broken_p = fn.copy(), fp.copy()
        broken_n["depth"][::7], broken_n["normal"][::11], broken_n["depth"][3::13], broken_n["depth"][5::17] = np.nan, np.nan, 1e30, np.inf
        broken_p["depth"][::5], broken_p["normal"][::9] = np.nan, np.inf
        check(r, centre_b, broken_n, centre_a, broken_p, junk_film, junk_moments, params, ptss.reproject_linear_params(), what + ("NaN and inf features",))
        far_a, far_b = camera_of("mixed"), camera_of("mixed")
        far_a.position.z, far_b.position.z, far_b.position.x = 4e15, 4e15, 3e8
        _, centre_fa = film_cameras(kp, wp, hp, far_a)
        _, centre_fb = film_cameras(kn, wn, hn, far_b)
        check(r, centre_fb, centre_features(r, centre_fb, seed), centre_fa, centre_features(r, centre_fa, seed), junk_film, junk_moments, params,
              ptss.reproject_linear_params(), what + ("beyond 1e15",))


# ---- 3. motion rows ------------------------------------------------------------------------------------------------------------------------------
def test_motion_rows_of_a_moved_mesh_and_of_an_unmoved_pose():
    from test_gpu_motion import grid_512, nudged, table_of
    w, h = 70, 37
    scene = grid_512()
    pose_a = table_of(scene.desc)
    r = ptss.Renderer(scene, w, h, max_iterations=2)
    cam_a = ptss.default_camera()
    cam_b = moved(cam_a, "df")
    params, reproject = ptss.linear_params(), ptss.reproject_linear_params()
    film_a, centre_a = film_cameras("pinhole", w, h, cam_a)
    _, centre_b = film_cameras("pinhole", w, h, cam_b)
    r.set_camera(cam_a)
    fp = r.features()
    assert same_bytes(fp, centre_features(r, centre_a, 5))   # the context's own pinhole at its own size: the same rows
    for kind in FILMS:
        film, moments, _ = rounds(r, film_a, 5, 3, kind == "splat", params)
        r.set_camera(cam_b)
        fn, still = r.features_motion(None)
        a = check(r, centre_b, fn, centre_a, fp, film, moments, params, reproject, (kind, "unmoved, rows"), motion=still)
        b = check(r, centre_b, fn, centre_a, fp, film, moments, params, reproject, (kind, "unmoved, NULL"))
        assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1]) and a[2] == b[2]
        r.update_triangles(nudged(pose_a, 0.05))
        fn2, mot = r.features_motion(pose_a)
        assert (mot["prevPoint"] != still["prevPoint"]).any()
        c = check(r, centre_b, fn2, centre_a, fp, film, moments, params, reproject, (kind, "moved mesh"), motion=mot)
        d = check(r, centre_b, fn2, centre_a, fp, film, moments, params, reproject, (kind, "moved mesh, NULL"))
        assert not same_bytes(c[0], d[0])   # the rows matter
        r.update_triangles(pose_a)
        r.set_camera(cam_a)
    r.close()


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement,kind", [("lds", "linear"), ("in_place", "linear"), ("lds", "splat"), ("in_place", "splat")])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement, kind):
    name = "mixed"
    splat = kind == "splat"
    seed = SCENES[name][3]
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=ITERATIONS, seed=seed)
    params, meter = ptss.linear_params(exposure=1.25), ptss.meter_params(rate=0.5)
    glare = ptss.glare_params(levels=5, mode="add", threshold=0.25, strength=0.25)
    denoise, plan = ptss.denoise_linear_params(levels=3), ptss.linear_plan_params()
    reproject = ptss.reproject_linear_params(max_history=4)
    cam = moved(camera_of(name), START)
    film_cam, centre = film_cameras("pinhole", W, H, cam)
    features = centre_features(r, centre, seed)
    shadow = [splat_film(N) if splat else linear_film(N), zero_moments(N)]
    film, moments, rng = rounds(r, film_cam, seed, 3, splat, params, shadow=shadow)
    state = want_state = None
    # two moves, chained: the second carries a film the first one seeded. Three rounds stand behind the first move (below the cap of
    # 4: K = 3), five behind the second (K = 4); two rounds follow each
    for move, most in (("df", 3 + 2), ("wg", 4 + 2)):
        what = (placement, kind, move)
        cam = moved(cam, move)
        film_next, centre_next = film_cameras("pinhole", W, H, cam)
        features_next = centre_features(r, centre_next, seed)
        film, moments, info = check(r, centre_next, features_next, centre, features, film, moments, params, reproject, what)
        want = ptss.probe_reproject_linear(centre_next, features_next, centre, features, shadow[0], shadow[1], params, reproject)
        assert same_bytes(film, want[0]) and same_bytes(moments, want[1])
        shadow = [want[0], want[1]]
        assert 0 < int(info["seeded"]) < N and int(info["noVariance"]) < int(info["seeded"])
        film_cam, centre, features = film_next, centre_next, features_next
        film, moments, rng = rounds(r, film_cam, seed, 2, splat, params, film, moments, rng, shadow=shadow)
        if not splat:   # the history plus the new rounds; a disoccluded pixel holds the new rounds alone
            assert int(film["samples"].max()) == most and int(film["samples"].min()) == 2
        cdf, index, plan_info = r.plan_samples_linear(moments, N, params, plan)
        want_plan = ptss.probe_plan_samples_linear(shadow[1], N, params, plan)
        assert np.array_equal(cdf, want_plan[0]) and np.array_equal(index, want_plan[1]) and plan_info == want_plan[2], what
        clean = r.denoise_linear(film, W, H, moments, features, params, denoise)
        want_clean = ptss.probe_denoise_linear(shadow[0], W, H, shadow[1], features, params, denoise)
        assert same_bytes(clean, want_clean), (what, first_difference(clean, want_clean))
        hist = r.meter_linear(clean)
        want_hist = ptss.probe_meter_linear(want_clean)
        state = r.meter_exposure(hist, state, params, meter)
        want_state = ptss.probe_meter_exposure(want_hist, want_state, params, meter)
        assert np.array_equal(hist, want_hist) and state_equal(state, want_state), what
        pyr = r.glare_build(clean, W, H, params, glare)
        want_pyr = ptss.probe_glare_build(want_clean, W, H, params, glare)
        assert same_bytes(pyr, want_pyr), what
        linear, pixels, history = r.resolve_linear(clean, params=params, metered=state, glare=(W, H, glare, pyr))
        wanted = ptss.probe_resolve_glare(want_clean, W, H, want_pyr, params=params, glare=glare, state=want_state)
        assert same_bytes(linear, wanted[0]) and np.array_equal(pixels, wanted[1]) and same_bytes(history, wanted[2]), what
        # the seeded film itself through its own kind's resolve
        own = (r.resolve_splat if splat else r.resolve_linear)(film, params=params)
        own_want = (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(shadow[0], params=params)
        assert same_bytes(own[0], own_want[0]) and np.array_equal(own[1], own_want[1]), what
    assert r.reproject_linear_launches() == 2
    assert 0 < int(pixels[:, :3].max()) and int(pixels[:, :3].min()) < 255
    r.close()


# ---- 5. frames, a second stream, two shards -----------------------------------------------------------------------------------------------------
def carry_case(r, seed, kind, keys="df", w=70, h=37):
    cam_a = moved(camera_of("mixed"), START)
    cam_b = moved(cam_a, keys)
    film_a, centre_a = film_cameras("pinhole", w, h, cam_a)
    _, centre_b = film_cameras("pinhole", w, h, cam_b)
    fp, fn = centre_features(r, centre_a, seed), centre_features(r, centre_b, seed)
    film, moments, _ = rounds(r, film_a, seed, 3, kind == "splat", ptss.linear_params())
    return centre_b, fn, centre_a, fp, film, moments


def test_frames_interleaved_with_the_calls_and_a_second_stream():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    params, reproject = ptss.linear_params(), ptss.reproject_linear_params()
    helper = ptss.Renderer(make_scene(name), W, H, max_iterations=ITERATIONS, seed=seed)   # (builds the cases; r traces nothing but its frames)
    cases = {kind: carry_case(helper, seed, kind) for kind in FILMS}
    helper.close()
    want = {kind: ptss.probe_reproject_linear(c[0], c[1], c[2], c[3], c[4], c[5], params, reproject) for kind, c in cases.items()}
    side = torch.cuda.Stream()
    i64 = lambda a: torch.from_numpy(words(a).view(np.int64).copy()).cuda()
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1, 8).copy()).cuda()
    dev = {kind: (f32(c[1]), f32(c[3]), i64(c[4]), i64(c[5])) for kind, c in cases.items()}
    torch.cuda.synchronize()
    P = 70 * 37
    for tick in range(4):
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        for kind, c in cases.items():
            got = r.reproject_linear(c[0], c[1], c[2], c[3], c[4], c[5], params, reproject)
            assert same_bytes(got[0], want[kind][0]) and same_bytes(got[1], want[kind][1]) and got[2] == want[kind][2], (tick, kind)
            with torch.cuda.stream(side):
                d_out = torch.full((P, 4), -1, dtype=torch.int64, device="cuda")
                d_mom = torch.full((P, 4), -1, dtype=torch.int64, device="cuda")
                d_info = torch.zeros(4, dtype=torch.int64, device="cuda")
                r.reproject_linear(c[0], dev[kind][0], c[2], dev[kind][1], dev[kind][2], dev[kind][3], params, reproject, film_kind=kind, out=d_out,
                                   moments_out=d_mom, info=d_info)
            side.synchronize()
            assert same_bytes(d_out.cpu().numpy(), want[kind][0]) and same_bytes(d_mom.cpu().numpy(), want[kind][1]), (tick, kind)
            assert d_info.cpu().numpy().view(np.uint64).tolist() == [int(v) for v in want[kind][2]], (tick, kind)
        assert r.launched_kernels() == before, tick   # the kernel owns no bit
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "four frames with the carry after each", W, H, 1)
    assert r.reproject_linear_launches() == 16
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.glare_launches() == (0, 0, 0) and r.denoise_linear_launches() == (0, 0)
    o.close()
    r.close()


def test_two_shards_serve_the_whole_film():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    params, reproject = ptss.linear_params(), ptss.reproject_linear_params()
    helper = ptss.Renderer(scene, W, H, max_iterations=ITERATIONS, seed=seed)
    c = carry_case(helper, seed, "linear", "wg")
    helper.close()
    want = ptss.probe_reproject_linear(c[0], c[1], c[2], c[3], c[4], c[5], params, reproject)
    for rank in (0, 1):
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8)
        got = r.reproject_linear(c[0], c[1], c[2], c[3], c[4], c[5], params, reproject)
        assert same_bytes(got[0], want[0]) and same_bytes(got[1], want[1]) and got[2] == want[2], rank
        assert r.reproject_linear_launches() == 1
        r.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    w, h = 20, 15
    P = w * h
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    names = ("lr_fn", "lr_mo", "lr_fp", "lr_film", "lr_mom", "lr_out", "lr_mout", "lr_info")
    sizes = [P * 32, P * 16, P * 32, P * 32, P * 32, P * 32, P * 32, 32]
    bufs = [r._device_buffer(n, s + 16) for n, s in zip(names, sizes)]
    d_fn, d_mo, d_fp, d_film, d_mom, d_out, d_mout, d_info = bufs
    cam = ptss.film_camera("pinhole", w, h, ptss.default_camera(), jitter=0)
    feat = np.zeros(P, dtype=ptss.FEATURE_DTYPE)
    feat["normal"], feat["depth"], feat["materialIdx"] = (0.0, 0.0, 1.0), 4.0, 0
    film = linear_film(P)
    film["r"], film["samples"] = 5 << 20, 5
    for s, dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, s + 16), "hipMemset")
    for dev, host in ((d_fn, feat), (d_fp, feat), (d_film, film)):
        ptss._hip_check(Hip.hipMemcpy(dev, host.ctypes.data, host.nbytes, 1), "hipMemcpy")
    params, good = ptss.linear_params(), ptss.reproject_linear_params()
    ref = lambda s: C.byref(s) if s is not None else None
    off = lambda p, k: C.c_void_p(p.value + k)

    def run(ctx, now=cam, fn=d_fn, mo=None, prev=cam, fp=d_fp, f=d_film, kind=0, mom=d_mom, p=params, q=good, out=d_out, mout=d_mout, info=d_info):
        return L.ptss_reproject_linear(ctx, ref(now), fn, mo, ref(prev), fp, f, kind, mom, ref(p), ref(q), out, mout, info, None)

    assert run(r._ctx) == 0 and run(r._ctx, kind=1) == 0 and run(r._ctx, mom=None, mout=None, info=None) == 0
    r.synchronize()
    counter, kernels = r.reproject_linear_launches(), r.launched_kernels()
    assert counter == 3

    def snapshot():
        out = []
        for s, dev in zip(sizes, bufs):
            host = np.empty(s + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    assert before[7][:32].view(np.uint64).tolist() == [2 * P, 0, 0, 2 * P]   # the two calls that count: every pixel seeded, the zero moments carry no variance
    EINVAL = -1
    assert run(None) == EINVAL
    for name in ("now", "fn", "prev", "fp", "f", "p", "q", "out"):
        assert run(r._ctx, **{name: None}) == EINVAL, name
    assert run(r._ctx, mom=None) == EINVAL and run(r._ctx, mout=None) == EINVAL
    for kind in (2, -1, 77):
        assert run(r._ctx, kind=kind) == EINVAL, kind
    for k in (4, 8):
        for name, dev in (("fn", d_fn), ("mo", d_mo), ("fp", d_fp), ("f", d_film), ("mom", d_mom), ("out", d_out), ("mout", d_mout)):
            assert run(r._ctx, **{name: off(dev, k)}) == EINVAL, (name, k)
    assert run(r._ctx, info=off(d_info, 4)) == EINVAL
    assert run(r._ctx, out=d_film) == EINVAL and run(r._ctx, out=d_mom) == EINVAL and run(r._ctx, mout=d_film) == EINVAL
    assert run(r._ctx, mout=d_mom) == EINVAL and run(r._ctx, mout=d_out) == EINVAL and run(r._ctx, out=off(d_film, 32 * P - 16)) == EINVAL
    for change in REPROJECT_REFUSED:
        assert run(r._ctx, q=changed(ptss.reproject_linear_params, **change)) == EINVAL, change
    for change in FILM_REFUSED:
        assert run(r._ctx, p=changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change)) == EINVAL, change
    for change in CAMERA_REFUSED:
        bad = changed(lambda: ptss.film_camera("pinhole", w, h, ptss.default_camera(), jitter=0), **change)
        assert run(r._ctx, now=bad) == EINVAL and run(r._ctx, prev=bad) == EINVAL, change
    n = C.c_ulonglong(0)
    assert L.ptss_reproject_linear_launches(None, C.byref(n)) == EINVAL and L.ptss_reproject_linear_launches(r._ctx, None) == EINVAL
    r.synchronize()
    assert r.reproject_linear_launches() == counter and r.launched_kernels() == kernels
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    r.close()


def test_a_film_of_one_row_of_tiles_and_a_narrow_tall_one():
    """16 x 4 pixels is less than one workgroup; 1 x 2^22 pixels, the tallest film the call takes, is 2^19 tile rows: more than a grid has
    in y. One row of workgroups serves both."""
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    for w, h in ((16, 4), (1, 1 << 22)):
        cam_a = ptss.default_camera()
        _, centre_a = film_cameras("equirect", w, h, cam_a)
        _, centre_b = film_cameras("equirect", w, h, moved(cam_a, "dfg"))
        fp, fn = centre_features(r, centre_a, 3), centre_features(r, centre_b, 3)
        film = linear_film(w * h)
        film["r"], film["g"], film["b"], film["samples"] = 3 << 20, np.arange(w * h) << 8, 1 << 18, 1 + np.arange(w * h) % 5
        check(r, centre_b, fn, centre_a, fp, film, None, ptss.linear_params(), ptss.reproject_linear_params(), (w, h))
    r.close()


# ---- 7. quality ----------------------------------------------------------------------------------------------------------------------------------
def relative_mse(film, truth, params):
    """The relative MSE of a film's linear means against the truth's, §3.34's denominator: mean over pixels and channels of
    (c - t)^2 / (t^2 + 0.01)."""
    def means(f):
        wd = words(f).astype(np.float64)
        return wd[:, :3] / np.maximum(wd[:, 3:4] % 2.0 ** 32, 1.0) * 2.0 ** -params.scaleLog2
    c, t = means(film), means(truth)
    return float(((c - t) ** 2 / (t ** 2 + 0.01)).mean())


def test_one_round_into_the_seeded_film_beats_one_round_into_an_empty_film():
    """cornell at 64 x 48: 64 rounds at pose A (one 'w' step in front of the default camera, §3.19's reason), a 'df' move, then one
    round at B into the seeded film against the same round into an empty film; truth = 256 rounds at B. The figures are printed; the
    measured ones stand in DESIGN.md §3.35."""
    name = "cornell"
    seed = SCENES[name][3]
    r = ptss.Renderer(make_scene(name), W, H, max_iterations=ITERATIONS, seed=seed)
    params, reproject = ptss.linear_params(), ptss.reproject_linear_params()
    cam_a = moved(ptss.default_camera(), "w")
    cam_b = moved(cam_a, "df")
    film_a, centre_a = film_cameras("pinhole", W, H, cam_a)
    film_b, centre_b = film_cameras("pinhole", W, H, cam_b)
    fp, fn = centre_features(r, centre_a, seed), centre_features(r, centre_b, seed)
    history, history_m, _ = rounds(r, film_a, seed, 64, False, params)
    truth, _, _ = rounds(r, film_b, seed + 1, 256, False, params)
    seeded, seeded_m, info = r.reproject_linear(centre_b, fn, centre_a, fp, history, history_m, params, reproject)
    assert int(info["seeded"]) > N // 2
    a, a_m, _ = rounds(r, film_b, seed + 2, 1, False, params, seeded, seeded_m)
    b, b_m, _ = rounds(r, film_b, seed + 2, 1, False, params)
    mse_seeded, mse_empty = relative_mse(a, truth, params), relative_mse(b, truth, params)
    denoise = ptss.denoise_linear_params()
    dn_seeded = relative_mse(r.denoise_linear(a, W, H, a_m, fn, params, denoise), truth, params)
    dn_empty = relative_mse(r.denoise_linear(b, W, H, b_m, fn, params, denoise), truth, params)
    print(f"relative MSE: seeded {mse_seeded:.4f}, empty {mse_empty:.4f}, ratio {mse_seeded / mse_empty:.3f}; denoised: seeded {dn_seeded:.4f}, "
          f"empty {dn_empty:.4f}; info {info}")
    assert mse_seeded < mse_empty
    r.close()
