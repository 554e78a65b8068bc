"""Glare for the two linear films on the GPU (ptss_glare_build, ptss_resolve_linear_glare / ptss_resolve_splat_glare).
Every test requires the device to equal the host probes byte for byte, and ptss_glare_launches to count what the design says a call
launches. The context is a 16 x 16 cornell.

1. The whole pyramid for every level count at the CPU test's sizes on both films, films whose words wrap, and two films sized by the
   header's constants so that the reduce's tile edges, the down and up kernels of the large levels and the single-workgroup tail all
   run. 2. The resolves with each combination of NULL outputs, sub-ranges, a state on the device and a state of garbage; strength 0
   against the plain resolves. 3. The loop generate -> trace -> accumulate (or splat) -> meter -> update -> build -> glare resolve
   against a shadow loop of the probes. 4. Frames interleaved with the calls stay the oracle's. 5. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from glare_common import (LEVELS, MODES, SIZES, STRENGTHS, default_params, every_kernel_sizes, film_of, first_difference, model_build_kernels,
                          model_means, model_tail_level, same_bytes, thresholds_for)
from linear_common import linear_film, params_of, same_words
from meter_common import new_state, state_equal
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from splat_common import splat_film
from test_glare_cpu import GLARE_REFUSED, changed
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu
FILMS = ("linear", "splat")


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


class Checker:
    """Device against probe for one context, keeping the three counters the calls move."""

    def __init__(self, r):
        self.r, self.launches = r, list(r.glare_launches())

    def counted(self, what):
        assert list(self.r.glare_launches()) == self.launches, (what, self.r.glare_launches(), self.launches)

    def build(self, what, film, w, h, params, glare):
        got = self.r.glare_build(film, w, h, params, glare)
        want = ptss.probe_glare_build(film, w, h, params, glare)
        assert same_bytes(got, want), (what, first_difference(got, want))
        self.launches[0] += 1
        self.launches[1] += model_build_kernels(w, h, glare.levels)
        self.counted(what)
        return got

    def resolve(self, what, film, w, h, pyramid, params, glare, state=None, **kw):
        call = self.r.resolve_splat if film.dtype == ptss.SPLAT_DTYPE else self.r.resolve_linear
        got = call(film, params=params, metered=state, glare=(w, h, glare, pyramid), **kw)
        want = ptss.probe_resolve_glare(film, w, h, pyramid, params=params, glare=glare, state=state, **kw)
        for a, b in zip(got, want):
            assert (a is None) == (b is None), what
            assert a is None or (np.array_equal(a, b) if a.dtype == np.uint8 else same_words(a, b)), what
        launched = any(kw.get(k, True) is not None for k in ("linear", "pixels", "history")) and kw.get("count", 1) != 0
        self.launches[2] += 1 if launched else 0
        self.counted(what)
        return got


# ---- 1. the pyramid --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_the_pyramid_equals_the_probe_at_every_size_and_level_count(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    params = default_params()
    for w, h in SIZES:
        film = film_of(w, h, splat, params)
        inside = thresholds_for(film, params)[1]
        for levels in LEVELS:
            c.build((w, h, levels), film, w, h, params, ptss.glare_params(levels=levels, threshold=inside if levels % 2 else 0.0))
    for w, h in ((3, 3), (37, 21)):   # sums no call of the library leaves: the words wrap on both sides alike
        c.build(("a high film", w, h), film_of(w, h, splat, params, kind="high"), w, h, params, ptss.glare_params(levels=4, threshold=1.5))
    c.build("above everything", film_of(37, 21, splat, params, kind="top"), 37, 21, params, ptss.glare_params(levels=3, threshold=2.0 ** 20))
    c.build("another scale", film_of(37, 21, splat, params_of(32, 256.0)), 37, 21, params_of(32, 256.0), ptss.glare_params(levels=5, threshold=0.01))


@pytest.mark.parametrize("kind", FILMS)
def test_films_on_which_every_kernel_runs(small, kind):
    """Sized by csrc/ptglare.h's kTile and kTailEntries: the tail starts at level 2 on the first film and at level 3 on the second, so the
    down and the up kernels of the large levels run once and twice, beside the tail; with two levels no tail runs at all."""
    splat = kind == "splat"
    c = Checker(small)
    params = default_params()
    (w2, h2), (w3, h3) = every_kernel_sizes()
    assert model_tail_level(w2, h2, 8) == 2 and model_tail_level(w3, h3, 8) == 3 and model_tail_level(w3, h3, 2) == 2
    assert (w2 // 2) % ptss.GLARE_TILE and (h2 // 2) % ptss.GLARE_TILE and w2 // 2 > 4 * ptss.GLARE_TILE   # level 1 ends inside a tile, past the fourth
    assert [model_build_kernels(w3, h3, L) for L in (1, 2, 3, 8)] == [1, 3, 5, 6] and model_build_kernels(w2, h2, 8) == 4
    film = film_of(w2, h2, splat, params)
    for levels in (1, 2, 3, 8):
        c.build((w2, h2, levels), film, w2, h2, params, ptss.glare_params(levels=levels, threshold=0.125))
    film = film_of(w3, h3, splat, params)
    for levels in (2, 3, 8):
        pyr = c.build((w3, h3, levels), film, w3, h3, params, ptss.glare_params(levels=levels))
    glare = ptss.glare_params(levels=8, mode="add", strength=0.5)
    c.resolve("the large film resolved", film, w3, h3, pyr, params, glare)


# ---- 2. the resolves ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_the_resolves_equal_the_probe(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    w, h = 37, 21
    P = w * h
    params = params_of(20, 65536.0, exposure=0.75)
    film = film_of(w, h, splat, params, seed=2)
    state = new_state()
    state["exposure"], state["updates"] = 2.5, 3
    for mode in MODES:
        for strength in STRENGTHS:
            glare = ptss.glare_params(levels=4, mode=mode, threshold=0.125, strength=strength)
            pyr = c.build((mode, strength), film, w, h, params, glare)
            c.resolve((mode, strength, "no state"), film, w, h, pyr, params, glare)
            c.resolve((mode, strength, "a state"), film, w, h, pyr, params, glare, state)
    before = dict(linear=np.full((P, 4), -3.0, np.float32), pixels=np.full((P, 4), 9, np.uint8), history=np.full((P, 4), -2.0, np.float32))
    for mask in range(8):   # each combination of NULL outputs; what is not asked for and what lies outside the range keeps its bytes
        kw = {k: (before[k] if mask & (1 << i) else None) for i, k in enumerate(("linear", "pixels", "history"))}
        c.resolve(("outputs", mask), film, w, h, pyr, params, glare, state if mask & 1 else None, **kw)
        outs = c.resolve(("a sub-range", mask), film, w, h, pyr, params, glare, None if mask & 1 else state, first_pixel=65, count=257, **kw)
        for out, was in zip(outs, (before["linear"], before["pixels"], before["history"])):
            if out is not None:
                rows = np.ascontiguousarray(out).view(was.dtype).reshape(-1, 4)
                assert np.array_equal(rows[:65], was[:65]) and np.array_equal(rows[65 + 257:], was[65 + 257:]) and not np.array_equal(rows[65:322], was[65:322])
    c.resolve("count = 0", film, w, h, pyr, params, glare, first_pixel=10, count=0)
    c.resolve("the last pixel", film, w, h, pyr, params, glare, first_pixel=P - 1, count=1)
    garbage = np.frombuffer(bytes(range(7, 55)), dtype=ptss.METER_STATE_DTYPE).copy()   # garbage in, garbage pixels out: no address depends on it
    for bits in (garbage, np.frombuffer(b"\xff" * 48, dtype=ptss.METER_STATE_DTYPE).copy()):
        linear, pixels, history = (small.resolve_splat if splat else small.resolve_linear)(film, params=params, metered=bits, glare=(w, h, glare, pyr))
        assert len(linear) == len(pixels) == len(history) == P
        c.launches[2] += 1
        c.counted("a state of garbage")
    junk = np.frombuffer(np.random.default_rng(5).bytes(len(pyr) * 32), dtype=ptss.GLARE_DTYPE).copy()   # and a pyramid of garbage
    c.resolve("a pyramid of garbage", film, w, h, junk, params, glare)


@pytest.mark.parametrize("kind", FILMS)
def test_a_state_on_the_device_and_strength_zero(small, kind):
    torch = pytest.importorskip("torch")
    splat = kind == "splat"
    w, h = 65, 34
    P = w * h
    params = params_of(20, 65536.0, exposure=1.5)
    film = film_of(w, h, splat, params, kind="top")   # means below 2^48: the plain resolve's bytes at strength 0
    film[::5] = film_of(w, h, splat, params, kind="pool", seed=1)[::5]
    beyond = [p for p, e in enumerate(model_means(film)) if max(e[:3]) >= 1 << 48]
    film[beyond] = film_of(w, h, splat, params, kind="top")[beyond]
    film[[0, 7, P - 1]] = (splat_film(1) if splat else linear_film(1))[0]   # pixels without samples
    before = small.glare_launches()
    d_film = torch.from_numpy(film.view(np.int64).reshape(-1, 4).copy()).cuda()
    state = new_state()
    state["exposure"], state["updates"] = 0.6, 1
    d_state = torch.from_numpy(state.view(np.int64).copy()).cuda()
    resolve, plain_probe = (small.resolve_splat, ptss.probe_resolve_splat) if splat else (small.resolve_linear, ptss.probe_resolve_linear)
    for k, glare in enumerate((ptss.glare_params(levels=5, strength=0.0), ptss.glare_params(levels=3, mode="add", strength=0.0),
                               ptss.glare_params(levels=6, mode="add", strength=0.3, threshold=0.5))):
        entries = ptss.glare_layout(w, h, glare.levels)[1]
        d_pyr = torch.full((entries, 4), -1, dtype=torch.int64, device="cuda")
        small.glare_build(d_film, w, h, params, glare, kind, d_pyr)
        pyr = d_pyr.cpu().numpy().view(np.uint64)
        assert same_bytes(pyr, ptss.probe_glare_build(film, w, h, params, glare)), glare.levels
        outs = [torch.zeros((P, 4), dtype=t, device="cuda") for t in (torch.float32, torch.uint8, torch.float32)]
        resolve(d_film, params=params, linear=outs[0], pixels=outs[1], history=outs[2], metered=d_state, glare=(w, h, glare, d_pyr))
        want = ptss.probe_resolve_glare(film, w, h, pyr, params=params, glare=glare, state=state)
        got = [o.cpu().numpy() for o in outs]
        assert same_words(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_words(got[2], want[2]), glare.levels
        if glare.strength == 0.0:   # the plain resolve at the state's exposure, on the device and on the host, N = 0 rows included
            at = ptss.linear_params(params.scaleLog2, params.clampMax, float(np.float32(0.6) * np.float32(1.5)))
            for a, b, d in zip(got, plain_probe(film, params=at), resolve(film, params=at)):
                assert a.tobytes() == b.tobytes() == d.tobytes(), (glare.levels, glare.mode)
    after = small.glare_launches()
    assert (after[0] - before[0], after[2] - before[2]) == (3, 3) and after[1] - before[1] == sum(model_build_kernels(w, h, L) for L in (5, 3, 6))


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement,kind", [("lds", "linear"), ("in_place", "linear"), ("lds", "splat"), ("in_place", "splat")])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement, kind):
    name, iterations = "mixed", 4
    splat = kind == "splat"
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params, meter, flt = ptss.linear_params(exposure=1.25), ptss.meter_params(rate=0.5), ptss.splat_filter("tent", 1.5)
    glare = ptss.glare_params(levels=6, mode="add" if placement == "lds" else "mix", threshold=0.25, strength=0.25)
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = splat_film(N) if splat else linear_film(N)
    state = want_state = None
    glow = 0
    for k in range(4):   # four rounds: generate, refill trace, accumulate or splat; meter, update; build, glare resolve
        what = (placement, kind, k)
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=flt, params=params, homed_first_pixel=0)
            shadow = ptss.probe_splat_paths(res, pos, shadow, W, H, filter=flt, params=params, homed_first_pixel=0)[0]   # the device's own results
        else:
            film = r.accumulate_paths_linear(res, film, params=params)
            shadow = ptss.probe_accumulate_linear(res, shadow, params=params)[0]
        assert film.tobytes() == shadow.tobytes(), what
        h = (r.meter_splat if splat else r.meter_linear)(film)
        want_h = (ptss.probe_meter_splat if splat else ptss.probe_meter_linear)(shadow)
        state = r.meter_exposure(h, state, params, meter)
        want_state = ptss.probe_meter_exposure(want_h, want_state, params, meter)
        assert np.array_equal(h, want_h) and state_equal(state, want_state), what
        pyr = r.glare_build(film, W, H, params, glare)
        want_pyr = ptss.probe_glare_build(shadow, W, H, params, glare)
        assert same_bytes(pyr, want_pyr), (what, first_difference(pyr, want_pyr))
        linear, pixels, history = (r.resolve_splat if splat else r.resolve_linear)(film, params=params, metered=state, glare=(W, H, glare, pyr))
        want = ptss.probe_resolve_glare(shadow, W, H, want_pyr, params=params, glare=glare, state=want_state)
        assert same_words(linear, want[0]) and np.array_equal(pixels, want[1]) and same_words(history, want[2]), what
        plain = (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(shadow, params=params)[0]
        glow += int((linear["r"] != plain["r"]).sum())
    assert r.glare_launches() == (4, 4 * model_build_kernels(W, H, 6), 4) and r.meter_launches() == (4, 4, 0) and glow > 0   # something bled
    assert pyr.view(np.uint64).any() and 0 < int(pixels[:, :3].max()) and int(pixels[:, :3].min()) < 255
    r.close()


# ---- 4. frames are untouched ---------------------------------------------------------------------------------------------------------------------
def test_frames_interleaved_with_the_calls_stay_the_oracles():
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    w, h = 65, 34
    params, glare = default_params(), ptss.glare_params(levels=7, mode="add", strength=0.4, threshold=0.25)
    films = {splat: film_of(w, h, splat, params, seed=3) for splat in (False, True)}
    want = {}
    for splat, film in films.items():
        pyr = ptss.probe_glare_build(film, w, h, params, glare)
        want[splat] = (pyr,) + ptss.probe_resolve_glare(film, w, h, pyr, params=params, glare=glare)
    for tick in range(10):   # ten frames with the calls after each
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        for splat, film in films.items():
            pyr = r.glare_build(film, w, h, params, glare)
            linear, px, hs = (r.resolve_splat if splat else r.resolve_linear)(film, params=params, glare=(w, h, glare, pyr))
            x = want[splat]
            assert same_bytes(pyr, x[0]) and same_words(linear, x[1]) and np.array_equal(px, x[2]) and same_words(hs, x[3]), tick
        assert r.launched_kernels() == before, tick   # the glare kernels own no bit
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "ten frames with the glare calls after each", W, H, 1)
    assert r.glare_launches() == (20, 20 * model_build_kernels(w, h, 7), 20)
    assert r.linear_launches() == (0, 0) and r.splat_stats()[:3] == (0, 0, 0) and r.meter_launches() == (0, 0, 0) and r.film_launches() == (0, 0, 0)
    o.close()
    r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    w, h = 20, 15
    Pf = w * h
    entries = ptss.glare_layout(w, h, 8)[1]
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("g_film", Pf * 32), ("g_pyr", entries * 32), ("g_state", 48), ("g_lin", Pf * 16), ("g_pix", Pf * 4), ("g_hist", Pf * 16))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_film, d_pyr, d_s, d_lin, d_pix, d_hist = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    film_params, good = ptss.linear_params(), ptss.glare_params(levels=4)
    host_film = film_of(w, h, False, film_params)
    ptss._hip_check(Hip.hipMemcpy(d_film, host_film.ctypes.data, host_film.nbytes, 1), "hipMemcpy")
    ref = lambda s: C.byref(s) if s is not None else None
    resolves = (L.ptss_resolve_linear_glare, L.ptss_resolve_splat_glare)

    def build(ctx, film, pyr, kind=0, width=w, height=h, params=film_params, glare=good):
        return L.ptss_glare_build(ctx, film, kind, width, height, ref(params), ref(glare), pyr, None)

    def rsv(call, ctx, film, first, count, pyr, s, lin, pix, hist, width=w, height=h, params=film_params, glare=good):
        return call(ctx, film, first, count, ref(params), width, height, ref(glare), pyr, s, lin, pix, hist, None)

    assert build(r._ctx, d_film, d_pyr) == 0 and build(r._ctx, d_film, d_pyr, 1) == 0
    for call in resolves:
        assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist) == 0
    r.synchronize()
    counters, kernels = r.glare_launches(), r.launched_kernels()
    assert counters == (2, 2 * model_build_kernels(w, h, 4), 2)

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    nan, inf = float("nan"), float("inf")
    bad_glares = [changed(lambda: ptss.glare_params(levels=4), **change) for change in GLARE_REFUSED]
    bad_films = []
    for change in (dict(structSize=16), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=inf), dict(scaleLog2=32, clampMax=257.0),
                   dict(exposure=-0.5), dict(exposure=nan), dict(reserved=1)):
        bad_films.append(changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change))
    bad_sides = ((0, h), (w, 0), (-1, h), (2 ** 22 + 1, 1), (1, 2 ** 22 + 1), (2 ** 22, 512), (46341, 46341))
    # ptss_glare_build
    assert build(None, d_film, d_pyr) == EINVAL and build(r._ctx, None, d_pyr) == EINVAL and build(r._ctx, d_film, None) == EINVAL
    assert build(r._ctx, d_film, d_pyr, params=None) == EINVAL and build(r._ctx, d_film, d_pyr, glare=None) == EINVAL
    for kind in (2, -1, 77):
        assert build(r._ctx, d_film, d_pyr, kind) == EINVAL, kind
    for k in (4, 8, 12):
        assert build(r._ctx, off(d_film, k), d_pyr, width=w - 1) == EINVAL and build(r._ctx, d_film, off(d_pyr, k)) == EINVAL, k
    for glare in bad_glares:
        assert build(r._ctx, d_film, d_pyr, glare=glare) == EINVAL
    assert build(r._ctx, d_film, d_pyr, params=ptss.linear_params(scale_log2=32, clamp_max=256.0), glare=ptss.glare_params(threshold=257.0)) == EINVAL
    for params in bad_films:
        assert build(r._ctx, d_film, d_pyr, params=params) == EINVAL
    for width, height in bad_sides:
        assert build(r._ctx, d_film, d_pyr, width=width, height=height) == ERANGE, (width, height)
    # the glare resolves: ptss_resolve_linear's refusals, the glare's, the state's and the film's extent
    for call in resolves:
        assert rsv(call, None, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist) == EINVAL and rsv(call, r._ctx, None, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist) == EINVAL
        assert rsv(call, r._ctx, d_film, 0, Pf, None, d_s, d_lin, d_pix, d_hist) == EINVAL
        assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist, params=None) == EINVAL
        assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist, glare=None) == EINVAL
        for k in (4, 8, 12):
            assert rsv(call, r._ctx, off(d_film, k), 0, Pf - 1, d_pyr, d_s, d_lin, d_pix, d_hist) == EINVAL, k
            assert rsv(call, r._ctx, d_film, 0, Pf, off(d_pyr, k), d_s, d_lin, d_pix, d_hist) == EINVAL, k
            assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, off(d_lin, k), d_pix, d_hist) == EINVAL, k
            assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, off(d_hist, k)) == EINVAL, k
        for k in (1, 2, 3):
            assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, off(d_pix, k), d_hist) == EINVAL, k
        for k in (1, 2, 4, 12):
            assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, off(d_s, k), d_lin, d_pix, d_hist) == EINVAL, k
        for first, count in ((0, Pf + 1), (Pf, 1), (1, Pf), (0, 2 ** 31), (2 ** 31, 1), (2 ** 63, 2 ** 63)):
            assert rsv(call, r._ctx, d_film, first, count, d_pyr, d_s, d_lin, d_pix, d_hist) == ERANGE, (first, count)
        for glare in bad_glares:
            assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist, glare=glare) == EINVAL
        for params in bad_films:
            assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, d_lin, d_pix, d_hist, params=params) == EINVAL
        for width, height in bad_sides:
            assert rsv(call, r._ctx, d_film, 0, 1, d_pyr, d_s, d_lin, d_pix, d_hist, width=width, height=height) == ERANGE, (width, height)
        assert rsv(call, r._ctx, None, 0, 0, None, None, None, None, None) == 0   # count = 0
        assert rsv(call, r._ctx, d_film, Pf, 0, d_pyr, None, d_lin, d_pix, d_hist) == 0
        assert rsv(call, r._ctx, d_film, 0, Pf, d_pyr, d_s, None, None, None) == 0   # nothing asked for: nothing launched
    out3 = (C.c_ulonglong * 3)()
    assert L.ptss_glare_launches(None, out3) == EINVAL and L.ptss_glare_launches(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.glare_launches() == counters and r.launched_kernels() == kernels
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.film_launches() == (0, 0, 0) and r.film_rejected() == 0
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 16-byte steps of the film and the pyramid, an 8-byte aligned state or none, 4-byte aligned pixels, the boundary parameters
    edge = ptss.glare_params(levels=8, mode="add", threshold=2.0 ** 20, strength=1.0)
    assert build(r._ctx, off(d_film, 16), off(d_pyr, 16), width=w - 1, height=h, glare=ptss.glare_params(levels=1)) == 0
    assert build(r._ctx, d_film, d_pyr, glare=edge) == 0
    assert rsv(L.ptss_resolve_linear_glare, r._ctx, off(d_film, 16), 0, Pf - 1, d_pyr, off(d_s, 8), off(d_lin, 16), off(d_pix, 4), None, glare=edge) == 0
    assert rsv(L.ptss_resolve_splat_glare, r._ctx, d_film, Pf - 1, 1, d_pyr, None, None, d_pix, None, glare=edge) == 0
    r.synchronize()
    assert r.glare_launches() == (4, counters[1] + 1 + model_build_kernels(w, h, 8), 4) and r.launched_kernels() == kernels
    r.close()
