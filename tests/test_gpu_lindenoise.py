"""The denoiser of the two linear films on the GPU (ptss_denoise_linear). Every test requires the device to equal the
host probe byte for byte — the output film and, through a read-back of the workspace, the float plane in front of the last pass — in
both kernel forms (taps from global memory; tile and halo staged in LDS, at the spacings where that kernel exists), and
ptss_denoise_linear_launches to count one kernel for prepare and one per pass.

1. Every size and level count on both films, in each form. 2. Inputs no film holds. 3. The loop generate -> trace -> accumulate with
stats -> denoise -> meter -> glare build -> resolve against a shadow loop of the probes. 4. levels = 0 on the device. 5. Frames
interleaved with the calls, a second stream, two shards. 6. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from glare_common import film_of
from lindenoise_common import case, first_difference, same_bytes, words
from linear_common import linear_film, params_of
from linstats_common import moments_of_rows, random_word_moments, zero_moments
from meter_common import state_equal
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from splat_common import splat_film
from test_gpu_kernel_coverage import compare
from test_lindenoise_cpu import BAD_SIDES, DENOISE_REFUSED, FILM_REFUSED, changed

pytestmark = pytest.mark.gpu
FILMS = ("linear", "splat")
SIZES = ((1, 1), (31, 7), (32, 8), (33, 9), (65, 17), (70, 37))
LEVELS = tuple(range(7))
FORMS = {"table": 0, "global": 1, "staged": 2, "staged at spacings 1 and 4": 4 + 5, "staged at spacing 2": 4 + 2}


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


class Checker:
    """Device against probe for one context, keeping the two counters the calls move. The probe of a case is taken once per level count
    and shared by the forms."""

    def __init__(self, r):
        self.r, self.launches, self.cache = r, list(r.denoise_linear_launches()), {}

    def probe(self, key, film, w, h, moments, features, params, levels, sigmas):
        k = (key, w, h, levels, sigmas)
        if k not in self.cache:
            d = ptss.denoise_linear_params(levels, *sigmas)
            self.cache[k] = ptss.probe_denoise_linear(film, w, h, moments, features, params, d, plane=True)
        return self.cache[k]

    def run(self, key, film, w, h, moments, features, params, levels, form=0, sigmas=(3.0, 0.1, 4.0)):
        what = (key, w, h, levels, form)
        self.r.debug_denoise_linear_form(form)
        try:
            got, ws = self.r.denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params(levels, *sigmas), workspace=True)
        finally:
            self.r.debug_denoise_linear_form(0)
        want = self.probe(key, film, w, h, moments, features, params, levels, sigmas)[0]
        assert same_bytes(got, want), (what, first_difference(got, want))
        if levels >= 1:   # the plane in front of the last pass: what the probe computes last with one level less
            P = w * h
            at = ((levels - 1) & 1) * 16 * P
            plane = ws[at:at + 16 * P].view(np.float32).reshape(-1, 4)
            want_plane = self.probe(key, film, w, h, moments, features, params, levels - 1, sigmas)[1]
            bad = np.nonzero((plane.view(np.uint32) != want_plane.view(np.uint32)).any(axis=1))[0]
            assert len(bad) == 0, (what, int(bad[0]), plane[bad[0]], want_plane[bad[0]], len(bad))
        self.launches[0] += 1
        self.launches[1] += 1 + levels
        assert list(self.r.denoise_linear_launches()) == self.launches, what
        return got


# ---- 1. every size, level count, film kind and form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_film_equals_the_probe_at_every_level_count_in_both_forms(small, size, kind):
    """Tile edges (32 x 8), the halo at the frame's border, tiles that are all halo, spacings larger than the frame; empty pixels at the
    tile corners, pixels of one sample, features with misses."""
    w, h = size
    c = Checker(small)
    params = params_of(20, 65536.0)
    film, moments, features = case(w, h, params, seed=1, splat=kind == "splat")
    for levels in LEVELS:
        for form in FORMS.values():
            c.run("case", film, w, h, moments, features, params, levels, form)


# ---- 2. inputs no film holds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_words_that_wrap_and_moments_of_random_bytes(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    params = params_of(20, 65536.0)
    g = np.random.default_rng(9)
    for w, h in ((65, 17), (70, 37)):
        film, moments, features = case(w, h, params, seed=2, splat=splat)
        P = w * h
        junk = random_word_moments(P, g)
        ones = moments_of_rows([[5, 25, 0, 1]] * P)
        high = film_of(w, h, splat, params, kind="high")   # sums no call of the library leaves
        pool = film_of(w, h, splat, params, seed=1)        # adversarial means up to 2^40, pixels without samples
        broken = features.copy()
        broken["depth"][::7] = np.nan
        broken["normal"][::11] = np.nan
        broken["depth"][3::13] = 1e30
        for form in (1, 2):
            for levels in (1, 3, 5):
                c.run("random moments", film, w, h, junk, features, params, levels, form)
                c.run("N = 1 everywhere", film, w, h, ones, features, params, levels, form)
                c.run("N = 0 everywhere", film, w, h, zero_moments(P), features, params, levels, form)
                c.run("a high film", high, w, h, junk, features, params, levels, form)
                c.run("the pool", pool, w, h, junk, features, params, levels, form, sigmas=(1e20, 1e20, 1e20))
                c.run("features of NaN", film, w, h, moments, broken, params, levels, form)
            coarse = params_of(6, 64.0)
            f2, m2, ft2 = case(w, h, coarse, seed=3, splat=splat)
            c.run("another scale", f2, w, h, m2, ft2, coarse, 4, form, sigmas=(0.5, 10.0, 0.25))


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement,kind", [("lds", "linear"), ("in_place", "linear"), ("lds", "splat"), ("in_place", "splat")])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement, kind):
    name, iterations = "mixed", 4
    splat = kind == "splat"
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    centre_cam = ptss.film_camera("pinhole", W, H, cam, jitter=0)
    params, meter, flt = ptss.linear_params(exposure=1.25), ptss.meter_params(rate=0.5), ptss.splat_filter("tent", 1.5)
    glare = ptss.glare_params(levels=6, mode="add", threshold=0.25, strength=0.25)
    denoise = ptss.denoise_linear_params(levels=4 if placement == "lds" else 5)
    features = r.ray_features(r.generate_rays(centre_cam, r.seed_path_rng(N, seed, 0, skip=0))[0])   # the pixel-centre rays
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = splat_film(N) if splat else linear_film(N)
    moments = shadow_m = zero_moments(N)
    state = want_state = None
    changed_pixels = 0
    for k in range(4):   # four rounds: generate, refill trace, accumulate with stats (and splat); denoise; meter, update; build, glare resolve
        what = (placement, kind, k)
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        if splat:   # the filtered film, with the moments kept by home pixel
            film = r.splat_paths(res, pos, film, W, H, filter=flt, params=params, homed_first_pixel=0)
            shadow = ptss.probe_splat_paths(res, pos, shadow, W, H, filter=flt, params=params, homed_first_pixel=0)[0]
            moments = r.accumulate_paths_linear_stats(res, None, moments, params=params)[1]
            shadow_m = ptss.probe_accumulate_linear_stats(res, None, shadow_m, params=params)[1]
        else:
            film, moments = r.accumulate_paths_linear_stats(res, film, moments, params=params)
            shadow, shadow_m, _ = ptss.probe_accumulate_linear_stats(res, shadow, shadow_m, params=params)
        assert same_bytes(film, shadow) and same_bytes(moments, shadow_m), what
        clean = r.denoise_linear(film, W, H, moments, features, params, denoise)
        want_clean = ptss.probe_denoise_linear(shadow, W, H, shadow_m, features, params, denoise)
        assert same_bytes(clean, want_clean), (what, first_difference(clean, want_clean))
        h = r.meter_linear(clean)
        want_h = ptss.probe_meter_linear(want_clean)
        state = r.meter_exposure(h, state, params, meter)
        want_state = ptss.probe_meter_exposure(want_h, want_state, params, meter)
        assert np.array_equal(h, want_h) and state_equal(state, want_state), what
        pyr = r.glare_build(clean, W, H, params, glare)
        want_pyr = ptss.probe_glare_build(want_clean, W, H, params, glare)
        assert same_bytes(pyr, want_pyr), what
        linear, pixels, history = r.resolve_linear(clean, params=params, metered=state, glare=(W, H, glare, pyr))
        want = ptss.probe_resolve_glare(want_clean, W, H, want_pyr, params=params, glare=glare, state=want_state)
        assert same_bytes(linear, want[0]) and np.array_equal(pixels, want[1]) and same_bytes(history, want[2]), what
        plain = r.denoise_linear(film, W, H, moments, features, params, ptss.denoise_linear_params(levels=0))
        changed_pixels += int((words(plain)[:, :3] != words(clean)[:, :3]).any(axis=1).sum())
    assert r.denoise_linear_launches() == (8, 4 * (1 + denoise.levels) + 4) and changed_pixels > N   # the filter did something
    assert 0 < int(pixels[:, :3].max()) and int(pixels[:, :3].min()) < 255
    r.close()


# ---- 4. levels = 0 on the device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_levels_zero_leaves_the_resolve_the_meter_and_the_glare_unchanged(small, kind):
    splat = kind == "splat"
    w, h = 65, 34
    params = params_of(20, 65536.0, exposure=0.75)
    film = film_of(w, h, splat, params, seed=4)
    out = small.denoise_linear(film, w, h, random_word_moments(w * h, np.random.default_rng(2)), case(w, h, params)[2], params,
                               ptss.denoise_linear_params(levels=0))
    a = (small.resolve_splat if splat else small.resolve_linear)(film, params=params)
    b = small.resolve_linear(out, params=params)
    assert a[1].tobytes() == b[1].tobytes()
    for ch in "rgb":
        assert a[0][ch].tobytes() == b[0][ch].tobytes() and a[2][ch].tobytes() == b[2][ch].tobytes(), ch
    assert np.array_equal((small.meter_splat if splat else small.meter_linear)(film), small.meter_linear(out))
    glare = ptss.glare_params(levels=5, threshold=0.125)
    assert same_bytes(small.glare_build(film, w, h, params, glare), small.glare_build(out, w, h, params, glare))


# ---- 5. frames, a second stream, two shards -----------------------------------------------------------------------------------------------------
def test_frames_interleaved_with_the_calls_and_a_second_stream():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    w, h = 70, 37
    P = w * h
    params, denoise = params_of(20, 65536.0), ptss.denoise_linear_params(levels=5)
    cases = {splat: case(w, h, params, seed=5, splat=splat) for splat in (False, True)}
    want = {splat: ptss.probe_denoise_linear(f, w, h, m, ft, params, denoise) for splat, (f, m, ft) in cases.items()}
    side = torch.cuda.Stream()
    dev = {splat: [torch.from_numpy(words(f).view(np.int64).copy()).cuda(), torch.from_numpy(words(m).view(np.int64).copy()).cuda(),
                   torch.from_numpy(np.ascontiguousarray(ft).view(np.float32).reshape(-1, 8).copy()).cuda()] for splat, (f, m, ft) in cases.items()}
    torch.cuda.synchronize()
    for tick in range(6):   # six frames with the calls after each, on the context's stream and on a second one
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        for splat, (f, m, ft) in cases.items():
            assert same_bytes(r.denoise_linear(f, w, h, m, ft, params, denoise), want[splat]), tick
            with torch.cuda.stream(side):
                d_out = torch.full((P, 4), -1, dtype=torch.int64, device="cuda")
                r.denoise_linear(dev[splat][0], w, h, dev[splat][1], dev[splat][2], params, denoise, film_kind="splat" if splat else "linear", out=d_out)
            side.synchronize()
            assert same_bytes(d_out.cpu().numpy(), want[splat]), tick
        assert r.launched_kernels() == before, tick   # the kernels own no bit
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "six frames with the denoiser after each", W, H, 1)
    assert r.denoise_linear_launches() == (24, 24 * 6)
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.glare_launches() == (0, 0, 0) and r.film_launches() == (0, 0, 0)
    o.close()
    r.close()


def test_two_shards_serve_the_whole_film():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    w, h = 70, 37
    params, denoise = params_of(20, 65536.0), ptss.denoise_linear_params(levels=3)
    film, moments, features = case(w, h, params, seed=6)
    want = ptss.probe_denoise_linear(film, w, h, moments, features, params, denoise)
    for rank in (0, 1):
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8)
        assert same_bytes(r.denoise_linear(film, w, h, moments, features, params, denoise), want), rank   # all of the film, whatever rows the shard owns
        assert r.denoise_linear_launches() == (1, 4)
        r.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    w, h = 20, 15
    P = w * h
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    ws_bytes = ptss.denoise_linear_workspace(w, h)
    sizes = (("ld_film", P * 32), ("ld_mom", P * 32), ("ld_feat", P * 32), ("ld_ws", ws_bytes + P * 32), ("ld_out", P * 32))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_film, d_mom, d_feat, d_ws, d_out = bufs
    params, good = ptss.linear_params(), ptss.denoise_linear_params(levels=3)
    film, moments, features = case(w, h, params)
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    for dev, host in ((d_film, film), (d_mom, moments), (d_feat, features)):
        ptss._hip_check(Hip.hipMemcpy(dev, host.ctypes.data, host.nbytes, 1), "hipMemcpy")
    ref = lambda s: C.byref(s) if s is not None else None
    off = lambda p, k: C.c_void_p(p.value + k)

    def run(ctx, f=d_film, kind=0, width=w, height=h, m=d_mom, ft=d_feat, p=params, d=good, workspace=d_ws, out=d_out):
        return L.ptss_denoise_linear(ctx, f, kind, width, height, m, ft, ref(p), ref(d), workspace, out, None)

    assert run(r._ctx) == 0 and run(r._ctx, kind=1) == 0
    r.synchronize()
    counters, kernels = r.denoise_linear_launches(), r.launched_kernels()
    assert counters == (2, 8)

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    assert run(None) == EINVAL
    for name in ("f", "m", "ft", "p", "d", "workspace", "out"):
        assert run(r._ctx, **{name: None}) == EINVAL, name
    for kind in (2, -1, 77):
        assert run(r._ctx, kind=kind) == EINVAL, kind
    for k in (4, 8, 12):
        for name, dev in (("f", d_film), ("m", d_mom), ("ft", d_feat), ("workspace", d_ws), ("out", d_out)):
            assert run(r._ctx, width=w - 1, **{name: off(dev, k)}) == EINVAL, (name, k)
    assert run(r._ctx, out=d_film) == EINVAL
    for k in (0, 16, ws_bytes - 16):   # dev_out or dev_film inside the workspace
        assert run(r._ctx, out=off(d_ws, k)) == EINVAL and run(r._ctx, f=off(d_ws, k)) == EINVAL, k
    for change in DENOISE_REFUSED:
        assert run(r._ctx, d=changed(lambda: ptss.denoise_linear_params(levels=3), **change)) == EINVAL, change
    for change in FILM_REFUSED:
        assert run(r._ctx, p=changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change)) == EINVAL, change
    for width, height in BAD_SIDES:
        assert run(r._ctx, width=width, height=height) == ERANGE, (width, height)
    out2 = (C.c_ulonglong * 2)()
    assert L.ptss_denoise_linear_launches(None, out2) == EINVAL and L.ptss_denoise_linear_launches(r._ctx, None) == EINVAL
    assert L.ptss_debug_denoise_linear_form(None, 0) == EINVAL and L.ptss_debug_denoise_linear_form(r._ctx, 3) == EINVAL and L.ptss_debug_denoise_linear_form(r._ctx, 12) == EINVAL
    assert L.ptss_debug_denoise_linear_form(r._ctx, -1) == EINVAL
    r.synchronize()
    assert r.denoise_linear_launches() == counters and r.launched_kernels() == kernels
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.glare_launches() == (0, 0, 0) and r.film_launches() == (0, 0, 0)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 16-byte steps of every pointer, an output right behind the workspace, the ends of the level range
    assert run(r._ctx, f=off(d_film, 16), m=off(d_mom, 16), ft=off(d_feat, 16), workspace=off(d_ws, 16), out=off(d_out, 16), width=w - 1) == 0
    assert run(r._ctx, out=off(d_ws, ws_bytes), d=ptss.denoise_linear_params(levels=6)) == 0
    assert run(r._ctx, d=ptss.denoise_linear_params(levels=0)) == 0
    r.synchronize()
    assert r.denoise_linear_launches() == (5, 8 + 4 + 7 + 1) and r.launched_kernels() == kernels
    r.close()
