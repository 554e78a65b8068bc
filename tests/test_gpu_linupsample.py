"""Upsampling the two linear films on the GPU (ptss_upsample_linear). Every test requires the device to equal the host
probe byte for byte — the large film and the three counters — in all three forms (0 the shipped table, 1 every tap from global memory,
2 the lo pixels of a tile divided once and staged in LDS), and ptss_upsample_linear_launches to move by one per call that launched.

1. Every size, factor, film kind and form, with and without the wrap. 2. Inputs no film holds. 3. The loop generate -> trace ->
accumulate with stats -> denoise -> features of both sizes -> upsample -> meter -> glare build -> glare resolve against a shadow loop
of the probes, on a pinhole and an equirect film. 4. Frames interleaved with the calls, a second stream, two shards, dev_info NULL.
5. Refusals.

The kernel's tile is 32 x 8 hi pixels. SIZES holds, for every factor f, lo films whose large film is a single pixel and less than a
tile — a workgroup whose staged rectangle is all ring around one or a few lo pixels —, one tile exactly (f = 3: 30 x 6, the nearest
below; 32 is no multiple of 3), one tile and one pixel column and row over (f = 2, 4: one lo pixel over), and several tiles."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from linear_common import linear_film
from linstats_common import zero_moments
from linupsample_common import (BAD_SIDES, BIG_PARAMS, COARSE_PARAMS, DEFAULT_PARAMS, FACTORS, FILM_REFUSED, TILE_X, TILE_Y, UP_REFUSED, case, changed,
                                features_of, first_difference, same_bytes, words, wrapped_sums_film)
from meter_common import state_equal
from path_query_common import SCENES, camera_of, make_scene
from splat_common import splat_film
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu
FILMS = ("linear", "splat")
FORMS = (0, 1, 2)
SIZES = {1: ((1, 1), (3, 2), (TILE_X, TILE_Y), (TILE_X + 1, TILE_Y + 1), (17, 9), (33, 17)),
         2: ((1, 1), (3, 2), (TILE_X // 2, TILE_Y // 2), (TILE_X // 2 + 1, TILE_Y // 2 + 1), (17, 9), (33, 9)),
         3: ((1, 1), (3, 2), (10, 2), (11, 3), (17, 9), (33, 9)),
         4: ((1, 1), (3, 2), (TILE_X // 4, TILE_Y // 4), (TILE_X // 4 + 1, TILE_Y // 4 + 1), (17, 9), (33, 9))}
INFO = ("filtered", "fallback", "empty")


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


class Checker:
    """Device against probe for one context, keeping the counter the calls move. The probe of a case is taken once and shared by the forms."""

    def __init__(self, r):
        self.r, self.launches, self.cache = r, r.upsample_linear_launches(), {}

    def run(self, key, film, w, h, flo, fhi, params, up, forms=FORMS):
        want = self.cache.get(key)
        if want is None:
            want = self.cache[key] = ptss.probe_upsample_linear(film, w, h, flo, fhi, params, up)
        for form in forms:
            what = (key, w, h, up.factor, up.flags, form)
            self.r.debug_upsample_linear_form(form)
            try:
                got, info = self.r.upsample_linear(film, w, h, flo, fhi, params, up)
            finally:
                self.r.debug_upsample_linear_form(0)
            assert same_bytes(got, want[0]), (what, first_difference(got, want[0]))
            assert info.tobytes() == want[1].tobytes(), (what, info, want[1])
            self.launches += 1
            assert self.r.upsample_linear_launches() == self.launches, what
        return want


# ---- 1. every size, factor, film kind and form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
@pytest.mark.parametrize("f", FACTORS)
def test_the_film_and_the_counters_equal_the_probe_in_every_form(small, f, kind):
    c = Checker(small)
    params = DEFAULT_PARAMS
    filtered = 0
    for w, h in SIZES[f]:
        for wrap in (False, True):
            film, flo, fhi, up = case(w, h, f, params, seed=1, splat=kind == "splat", wrap=wrap)
            _, info = c.run((w, h, wrap), film, w, h, flo, fhi, params, up)
            assert sum(int(info[k]) for k in INFO) == f * f * w * h
            if w * h >= 100:   # the cases filter: most hi pixels have counted taps, some have none, some are empty
                assert 2 * int(info["filtered"]) >= f * f * w * h and int(info["fallback"]) >= 1 and int(info["empty"]) >= 1, (w, h, info)
            filtered += int(info["filtered"])
    assert filtered > 0


def test_a_large_film_higher_than_a_launch_grid_has_rows(small):
    """1 x 2^17 by 4: 524,288 hi rows, 65,536 tile rows — more than the second dimension of a launch grid holds and past ptss_upsample's
    limit of 524,280 rows: the tiles are indexed along one dimension."""
    w, h, f = 1, 1 << 17, 4
    g = np.random.default_rng(11)
    n = g.integers(0, 4, w * h).astype(np.uint64)
    film = np.zeros(w * h, dtype=ptss.LINEAR_DTYPE)
    for ch in "rgb":
        film[ch] = g.integers(0, 1 << 30, w * h).astype(np.uint64) * n
    film["samples"] = n

    def flat(rows):
        ft = np.zeros(rows, dtype=ptss.FEATURE_DTYPE)
        ft["normal"][:, 2], ft["depth"] = 1.0, (2.0 + np.arange(rows) * (8.0 / rows)).astype(np.float32)
        return ft

    flo, fhi = flat(h), np.repeat(flat(f * h), f)   # one column: a hi row's four pixels share its depth
    c = Checker(small)
    _, info = c.run("high", film, w, h, flo, fhi, DEFAULT_PARAMS, ptss.upsample_linear_params(f, 0.1, 4.0, wrap_x=True), forms=(1, 2))
    assert sum(int(info[k]) for k in INFO) == f * f * w * h and 2 * int(info["filtered"]) > f * f * w * h and int(info["empty"]) > 0


# ---- 2. inputs no film holds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_words_that_wrap_means_at_two_to_the_forty_and_features_of_nan(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    w, h = 33, 9
    for f in FACTORS:
        wrap = f % 2 == 0
        up = ptss.upsample_linear_params(f, 0.1, 4.0, wrap_x=wrap)
        flo, fhi = features_of(w, h, bad=True), features_of(w * f, h * f, bad=True)
        c.run(("sums that wrap", f), wrapped_sums_film(w * h, splat, seed=f), w, h, flo, fhi, DEFAULT_PARAMS, up)
        film, flo2, fhi2, _ = case(w, h, f, BIG_PARAMS, seed=2, splat=splat, wrap=wrap, bad=True, big=True)
        assert int(words(film)[:, :3].max()) >= 1 << 40
        c.run(("means at 2^40, NaN and 1e30 in the features", f), film, w, h, flo2, fhi2, BIG_PARAMS, up)
        coarse, clo, chi, _ = case(w, h, f, COARSE_PARAMS, seed=3, splat=splat, wrap=wrap)
        c.run(("another scale", f), coarse, w, h, clo, chi, COARSE_PARAMS, ptss.upsample_linear_params(f, 10.0, 0.25, wrap_x=wrap))


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("film_kind,kind", [("pinhole", "linear"), ("equirect", "linear"), ("equirect", "splat")])
def test_the_loop_equals_a_shadow_loop_of_the_probes(film_kind, kind):
    name, iterations, w, h, f = "mixed", 4, 32, 24, 2
    P, splat = w * h, kind == "splat"
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name), w, h, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera(film_kind, w, h, cam, jitter=1)
    params, meter, flt = ptss.linear_params(exposure=1.25), ptss.meter_params(rate=0.5), ptss.splat_filter("tent", 1.5)
    glare = ptss.glare_params(levels=5, mode="add", threshold=0.25, strength=0.25)
    denoise = ptss.denoise_linear_params(levels=3)
    up = ptss.upsample_linear_params(f, wrap_x=film_kind == "equirect")
    # the centre rays of the same film camera at both sizes
    centre = lambda s: r.ray_features(r.generate_rays(ptss.film_camera(film_kind, s * w, s * h, cam, jitter=0), r.seed_path_rng(s * s * P, seed, 0, skip=0))[0])
    flo, fhi = centre(1), centre(f)
    rng = r.seed_path_rng(P, seed, 0, skip=0)
    film = shadow = splat_film(P) if splat else linear_film(P)
    moments = shadow_m = zero_moments(P)
    state = want_state = None
    totals = np.zeros(1, ptss.UPSAMPLE_LINEAR_INFO_DTYPE)[0]
    for k in range(3):
        what = (film_kind, kind, k)
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        if splat:
            film = r.splat_paths(res, pos, film, w, h, filter=flt, params=params, homed_first_pixel=0)
            shadow = ptss.probe_splat_paths(res, pos, shadow, w, h, filter=flt, params=params, homed_first_pixel=0)[0]
            moments = r.accumulate_paths_linear_stats(res, None, moments, params=params)[1]
            shadow_m = ptss.probe_accumulate_linear_stats(res, None, shadow_m, params=params)[1]
        else:
            film, moments = r.accumulate_paths_linear_stats(res, film, moments, params=params)
            shadow, shadow_m, _ = ptss.probe_accumulate_linear_stats(res, shadow, shadow_m, params=params)
        assert same_bytes(film, shadow) and same_bytes(moments, shadow_m), what
        clean = r.denoise_linear(film, w, h, moments, flo, params, denoise)
        want_clean = ptss.probe_denoise_linear(shadow, w, h, shadow_m, flo, params, denoise)
        assert same_bytes(clean, want_clean), what
        large, totals = r.upsample_linear(clean, w, h, flo, fhi, params, up, info=totals)
        want_large, info = ptss.probe_upsample_linear(want_clean, w, h, flo, fhi, params, up)
        assert same_bytes(large, want_large), (what, first_difference(large, want_large))
        assert len(large) == f * f * P and int(info["filtered"]) > P   # (a quarter at the least: the nearest lo pixel mostly has the hi pixel's material)
        hist = r.meter_linear(large)
        want_hist = ptss.probe_meter_linear(want_large)
        state = r.meter_exposure(hist, state, params, meter)
        want_state = ptss.probe_meter_exposure(want_hist, want_state, params, meter)
        assert np.array_equal(hist, want_hist) and state_equal(state, want_state), what
        pyr = r.glare_build(large, f * w, f * h, params, glare)
        want_pyr = ptss.probe_glare_build(want_large, f * w, f * h, params, glare)
        assert same_bytes(pyr, want_pyr), what
        linear, pixels, history = r.resolve_linear(large, params=params, metered=state, glare=(f * w, f * h, glare, pyr))
        want = ptss.probe_resolve_glare(want_large, f * w, f * h, want_pyr, params=params, glare=glare, state=want_state)
        assert same_bytes(linear, want[0]) and np.array_equal(pixels, want[1]) and same_bytes(history, want[2]), what
    assert sum(int(totals[n]) for n in INFO) == 3 * f * f * P   # the counters are added to
    assert r.upsample_linear_launches() == 3 and len(pixels) == f * f * P
    assert 0 < int(pixels[:, :3].max()) and int(pixels[:, :3].min()) < 255
    r.close()


# ---- 4. frames, a second stream, two shards, dev_info NULL ----------------------------------------------------------------------------------------
def test_frames_interleaved_with_the_calls_a_second_stream_and_no_info():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    W, H = 64, 48
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    w, h, f = 33, 17, 3
    params = DEFAULT_PARAMS
    cases = {splat: case(w, h, f, params, seed=5, splat=splat, wrap=splat) for splat in (False, True)}
    want = {splat: ptss.probe_upsample_linear(film, w, h, flo, fhi, params, up) for splat, (film, flo, fhi, up) in cases.items()}
    side = torch.cuda.Stream()
    rows = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.float32).reshape(-1, 8).copy()).cuda()
    dev = {splat: [torch.from_numpy(words(film).view(np.int64).copy()).cuda(), rows(flo), rows(fhi)] for splat, (film, flo, fhi, up) in cases.items()}
    torch.cuda.synchronize()
    calls = 0
    for tick in range(4):   # four frames with the calls after each, on the context's stream and on a second one
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        for splat, (film, flo, fhi, up) in cases.items():
            got, info = r.upsample_linear(film, w, h, flo, fhi, params, up)
            assert same_bytes(got, want[splat][0]) and info.tobytes() == want[splat][1].tobytes(), tick
            got, info = r.upsample_linear(film, w, h, flo, fhi, params, up, info=False)   # dev_info NULL
            assert same_bytes(got, want[splat][0]) and info is None, tick
            with torch.cuda.stream(side):
                d_out = torch.full((f * f * w * h, 4), -1, dtype=torch.int64, device="cuda")
                d_info = torch.zeros(3, dtype=torch.int64, device="cuda")
                r.upsample_linear(dev[splat][0], w, h, dev[splat][1], dev[splat][2], params, up, film_kind="splat" if splat else "linear", out=d_out,
                                  info=d_info)
            side.synchronize()
            assert same_bytes(d_out.cpu().numpy(), want[splat][0]) and d_info.cpu().numpy().tobytes() == want[splat][1].tobytes(), tick
            calls += 3
        assert r.launched_kernels() == before, tick   # the kernels own no bit
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "four frames with the upsample after each", W, H, 1)
    assert r.upsample_linear_launches() == calls
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.glare_launches() == (0, 0, 0) and r.film_launches() == (0, 0, 0)
    o.close()
    r.close()


def test_two_shards_serve_the_whole_film():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    w, h, f = 33, 17, 2
    params = DEFAULT_PARAMS
    film, flo, fhi, up = case(w, h, f, params, seed=6)
    want = ptss.probe_upsample_linear(film, w, h, flo, fhi, params, up)
    for rank in (0, 1):
        r = ptss.Renderer(scene, 64, 48, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8)
        got, info = r.upsample_linear(film, w, h, flo, fhi, params, up)   # all of the film, whatever rows the shard owns
        assert same_bytes(got, want[0]) and info.tobytes() == want[1].tobytes(), rank
        assert r.upsample_linear_launches() == 1
        r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    w, h, f = 20, 15, 2
    P, Q = w * h, f * f * w * h
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("lu_film", P * 32), ("lu_flo", P * 32), ("lu_fhi", Q * 32), ("lu_out", Q * 32 + P * 32), ("lu_info", 24))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_film, d_flo, d_fhi, d_out, d_info = bufs
    params, good = ptss.linear_params(), ptss.upsample_linear_params(f)
    film, flo, fhi, _ = case(w, h, f, params)
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    for dev, host in ((d_film, film), (d_flo, flo), (d_fhi, fhi)):
        ptss._hip_check(Hip.hipMemcpy(dev, host.ctypes.data, host.nbytes, 1), "hipMemcpy")
    ref = lambda s: C.byref(s) if s is not None else None
    off = lambda p, k: C.c_void_p(p.value + k)

    def run(ctx, film=d_film, kind=0, width=w, height=h, lo=d_flo, hi=d_fhi, p=params, u=good, out=d_out, info=d_info):
        return L.ptss_upsample_linear(ctx, film, kind, width, height, lo, hi, ref(p), ref(u), out, info, None)

    assert run(r._ctx) == 0 and run(r._ctx, kind=1) == 0 and run(r._ctx, info=None) == 0
    r.synchronize()
    counter, kernels = r.upsample_linear_launches(), r.launched_kernels()
    assert counter == 3

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    assert int(before[4][:24].view(np.uint64).sum()) == 2 * Q
    assert run(None) == EINVAL
    for name in ("film", "lo", "hi", "p", "u", "out"):
        assert run(r._ctx, **{name: None}) == EINVAL, name
    for kind in (2, -1, 77):
        assert run(r._ctx, kind=kind) == EINVAL, kind
    for k in (4, 8, 12):
        for name, dev in (("film", d_film), ("lo", d_flo), ("hi", d_fhi), ("out", d_out)):
            assert run(r._ctx, width=w - 1, **{name: off(dev, k)}) == EINVAL, (name, k)
    for k in (4, 12):
        assert run(r._ctx, info=off(d_info, k)) == EINVAL, k
    # an output range that overlaps the input film: the film itself, a film that starts inside the output, one that ends inside it
    assert run(r._ctx, out=d_film) == EINVAL
    assert run(r._ctx, film=off(d_out, 32)) == EINVAL and run(r._ctx, film=off(d_out, Q * 32 - 16)) == EINVAL
    for change in UP_REFUSED:
        assert run(r._ctx, u=changed(lambda: ptss.upsample_linear_params(f), **change)) == EINVAL, change
    for change in FILM_REFUSED:
        assert run(r._ctx, p=changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change)) == EINVAL, change
    for width, height, factor in BAD_SIDES:
        assert run(r._ctx, width=width, height=height, u=ptss.upsample_linear_params(factor)) == ERANGE, (width, height, factor)
    one = C.c_ulonglong(0)
    assert L.ptss_upsample_linear_launches(None, C.byref(one)) == EINVAL and L.ptss_upsample_linear_launches(r._ctx, None) == EINVAL
    assert L.ptss_debug_upsample_linear_form(None, 0) == EINVAL and L.ptss_debug_upsample_linear_form(r._ctx, 3) == EINVAL
    assert L.ptss_debug_upsample_linear_form(r._ctx, -1) == EINVAL
    r.synchronize()
    assert r.upsample_linear_launches() == counter and r.launched_kernels() == kernels
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.glare_launches() == (0, 0, 0) and r.film_launches() == (0, 0, 0)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 16-byte steps of every pointer, 8-byte steps of the info, a film right behind the output, the ends of the factor range
    assert run(r._ctx, film=off(d_film, 16), lo=off(d_flo, 16), hi=off(d_fhi, 16), out=off(d_out, 16), info=off(d_info, 8), width=w - 1) == 0
    assert run(r._ctx, film=off(d_out, Q * 32)) == 0
    assert run(r._ctx, u=ptss.upsample_linear_params(1)) == 0 and run(r._ctx, width=w // 2, height=h // 2, u=ptss.upsample_linear_params(4)) == 0
    r.synchronize()
    assert r.upsample_linear_launches() == counter + 4 and r.launched_kernels() == kernels
    r.close()
