"""The meter of the two linear films on the GPU (ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure and the metered resolves;
DESIGN.md §3.31). Every test requires the device to equal the host probes byte for byte. The context is a 16 x 16 cornell; the film is
the siblings' 64 x 48.

1. Histograms of both films: counts of 1, 63, 64, 65 and 257 pixels from a first pixel above 0, the whole film, every pixel in one bin, 64
   different bins in every 64 pixels, the adversarial and the largest rows, pixels without samples inside and between runs, two calls into
   one histogram, and one film of grid cap x block + 257 pixels, so that the stride loop and its tail both run.
2. The exposure kernel on every histogram of the CPU test, and a chain of updates whose state stays on the device.
3. The metered resolves against the plain ones given the state's exposure read back. 4. The loop generate -> trace -> accumulate ->
   meter -> update -> metered resolve against a shadow loop of the probes, the history through the denoiser. 5. No trace in frame state, a
   second stream, two shards into one histogram. 6. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from film_common import BATCHES, results_of
from linear_common import SCALES, high_film, linear_film, params_of, same_words
from meter_common import (BINS, adversarial_films, bin_film, exposure_histograms, largest_linear_rows, largest_splat_rows, new_state,
                          state_equal)
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from splat_common import high_film as high_splat_film
from splat_common import splat_film
from test_gpu_kernel_coverage import compare
from test_meter_cpu import METERS

pytestmark = pytest.mark.gpu
P = W * H
FILMS = ("linear", "splat")


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


class Checker:
    """Device against probe for one context, keeping the three counters the calls move."""

    def __init__(self, r):
        self.r, self.launches = r, list(r.meter_launches())

    def counted(self, what):
        assert list(self.r.meter_launches()) == self.launches, what

    def meter(self, what, film, splat, **kw):
        got = (self.r.meter_splat if splat else self.r.meter_linear)(film, **kw)
        want = (ptss.probe_meter_splat if splat else ptss.probe_meter_linear)(film, **kw)
        assert np.array_equal(got, want), what
        count = kw.get("count")
        self.launches[0] += 1 if len(film) - kw.get("first_pixel", 0) > 0 and count != 0 else 0
        self.counted(what)
        return got

    def exposure(self, what, h, state, params, meter):
        got = self.r.meter_exposure(h, state, params, meter)
        want = ptss.probe_meter_exposure(h, state, params, meter)
        assert state_equal(got, want), (what, got, want)
        self.launches[1] += 1
        self.counted(what)
        return got

    def resolve(self, what, film, splat, state, params, **kw):
        """The metered resolve against the probe of the plain one at exposure = state's * params', and against the plain call itself."""
        call = self.r.resolve_splat if splat else self.r.resolve_linear
        got = call(film, params=params, metered=state, **kw)
        at = ptss.linear_params(params.scaleLog2, params.clampMax, float(np.float32(state["exposure"][0]) * np.float32(params.exposure)))
        want = (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(film, params=at, **kw)
        plain = call(film, params=at, **kw)
        for a, b, c in zip(got, want, plain):
            assert (a is None) == (b is None) == (c is None), what
            assert a is None or (np.array_equal(a, b) if a.dtype == np.uint8 else same_words(a, b)), what
            assert a is None or a.tobytes() == c.tobytes(), what
        launched = any(kw.get(k, True) is not None for k in ("linear", "pixels", "history")) and len(film) > 0 and kw.get("count", 1) != 0
        self.launches[2] += 1 if launched else 0
        self.counted(what)
        return got


_ROWS = {}


def rows_film(splat, P_):
    """P_ pixels tiled from the adversarial and the largest rows of one film, every seventh pixel without samples."""
    if not _ROWS:   # built once
        films = adversarial_films()
        for s in (False, True):
            parts = [film for _, film, fs in films if fs == s]
            parts += [largest_splat_rows(), high_splat_film(3)] if s else list(largest_linear_rows())
            _ROWS[s] = np.concatenate(parts)
    rows = _ROWS[splat]
    film = np.tile(rows, -(-P_ // len(rows)))[:P_].copy()
    film["weight" if splat else "samples"][::7] = 0
    return film


# ---- 1. histograms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_histograms_equal_the_probe(small, kind):
    splat = kind == "splat"
    c, g = Checker(small), np.random.default_rng(3)
    film = rows_film(splat, P)
    whole = c.meter("the whole film", film, splat)
    assert 0 < int(whole.sum()) < P and np.count_nonzero(whole) > 20
    for n in BATCHES:   # 1, 63, 64, 65, 257 pixels from a first pixel > 0
        c.meter(("first pixel 1000", n), film, splat, first_pixel=1000, count=n)
        c.meter(("first pixel 1", n), film, splat, first_pixel=1, count=n, histogram=whole)
    c.meter("to the film's end", film, splat, first_pixel=P - 65)
    c.meter("count = 0", film, splat, first_pixel=10, count=0, histogram=whole)
    one = c.meter("every pixel in one bin", bin_film([137] * P, splat), splat)
    assert one[137] == P and one.sum() == P
    spread = bin_film([30 + 4 * (i % 64) + (i // 64) % 4 for i in range(P)], splat)   # 64 different bins in every 64 consecutive pixels
    h = c.meter("64 bins per wave", spread, splat)
    assert np.count_nonzero(h) == 256 and h.max() == P // 256
    # pixels without samples inside runs of one bin and between them, black pixels, and runs that cross wave and workgroup edges
    bins = np.repeat(g.integers(25, 322, 60), g.integers(1, 130, 60))[:P]
    bins = np.concatenate([bins, np.full(P - len(bins), 200)])
    bins[g.choice(P, 300, replace=False)] = -1
    bins[g.choice(P, 100, replace=False)] = 0
    bins[64:128] = -1   # a whole wave without a pixel to meter
    h = c.meter("runs with holes", bin_film(bins, splat), splat)
    assert h[0] == int((bins == 0).sum()) and h.sum() == int((bins >= 0).sum())
    # two calls into one histogram = one call over the union; a histogram that was in use, counts that wrap
    first = c.meter("first half", film, splat, count=1500)
    both = c.meter("second half into the same", film, splat, first_pixel=1500, histogram=first)
    assert np.array_equal(both, whole)
    c.meter("a histogram near 2^32", film, splat, histogram=np.full(BINS, 2 ** 32 - 3, np.uint32))


@pytest.mark.parametrize("kind", FILMS)
def test_a_film_larger_than_the_grid_strides_and_ends_in_a_tail(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    big = ptss.METER_GRID_CAP * ptss.METER_BLOCK + 257
    film = rows_film(splat, big)
    h = c.meter("grid cap x block + 257 pixels", film, splat)
    assert int(h.sum()) == int((film["weight" if splat else "samples"] != 0).sum())
    c.meter("from an odd first pixel", film, splat, first_pixel=12345, count=big - 12345 - 1)


# ---- 2. exposure ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_log2", [0, 20, 32])
def test_exposure_equals_the_probe(small, scale_log2):
    c = Checker(small)
    params = params_of(scale_log2, dict(SCALES[:3])[scale_log2])
    used = new_state()
    used["exposure"], used["target"], used["meanLog2"], used["updates"] = 3.5, 2.0, -1.25, 9
    for hname, h in exposure_histograms():
        for mname, kw in METERS.items():
            c.exposure((hname, mname), h, None, params, ptss.meter_params(**kw))
        c.exposure((hname, "a state in use"), h, used, params, ptss.meter_params(rate=0.3))
    dark = np.zeros(BINS, np.uint32)
    dark[1] = 10
    c.exposure("both clamps", dark, None, params, ptss.meter_params(min_exposure=0.5, max_exposure=4.0))
    c.exposure("a zero exposure", dark, used, params, ptss.meter_params(min_exposure=0.0, max_exposure=0.0))


@pytest.mark.parametrize("rate", [0.25, 0.0, 1.0])
def test_a_chain_of_updates_with_the_state_on_the_device(small, rate):
    torch = pytest.importorskip("torch")
    params, meter = ptss.linear_params(), ptss.meter_params(rate=rate)
    hists = [h for _, h in exposure_histograms()]
    chain = [hists[9], hists[2], hists[0], hists[3], hists[1]]
    before = small.meter_launches()
    d_state = torch.zeros(6, dtype=torch.int64, device="cuda")
    want = new_state()
    for k, h in enumerate(chain):   # five updates, the state never leaving the device
        d_h = torch.from_numpy(h.view(np.int32).copy()).cuda()
        small.meter_exposure(d_h, d_state, params, meter)
        want = ptss.probe_meter_exposure(h, want, params, meter)
        got = d_state.cpu().numpy().view(ptss.METER_STATE_DTYPE)
        assert state_equal(got, want), (rate, k, got, want)
    assert int(want["updates"][0]) == 5 and small.meter_launches() == (before[0], before[1] + 5, before[2])


# ---- 3. the metered resolves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_metered_resolves_equal_the_plain_ones_at_the_states_exposure(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    film = rows_film(splat, 700)
    before = dict(linear=np.full((700, 4), -3.0, np.float32), pixels=np.full((700, 4), 9, np.uint8), history=np.full((700, 4), -2.0, np.float32))
    params = ptss.linear_params()
    state = c.exposure("the film's own state", (ptss.probe_meter_splat if splat else ptss.probe_meter_linear)(film), None, params, ptss.meter_params())
    assert 0 < float(state["exposure"][0]) < 65536
    for compensation in (1.0, 0.37):
        params = ptss.linear_params(exposure=compensation)
        for mask in range(8):   # each combination of NULL outputs; what is not asked for and what lies outside the range keeps its bytes
            kw = {k: (before[k] if mask & (1 << i) else None) for i, k in enumerate(("linear", "pixels", "history"))}
            c.resolve(("outputs", mask, compensation), film, splat, state, params, **kw)
            linear, pixels, history = c.resolve(("a sub-range", mask, compensation), film, splat, state, params, first_pixel=65, count=257, **kw)
            for out, was in ((linear, before["linear"]), (pixels, before["pixels"]), (history, before["history"])):
                if out is not None:
                    rows = np.ascontiguousarray(out).view(was.dtype).reshape(-1, 4)
                    assert np.array_equal(rows[:65], was[:65]) and np.array_equal(rows[65 + 257:], was[65 + 257:]) and not np.array_equal(rows[65:322], was[65:322])
    c.resolve("count = 0", film, splat, state, params, first_pixel=10, count=0)
    for exposure in (0.0, 1.0, 2.0 ** -16, 40.0):   # states the caller made
        made = new_state()
        made["exposure"], made["updates"] = exposure, 1
        c.resolve(("a made state", exposure), film, splat, made, ptss.linear_params(exposure=1.5))
    garbage = np.frombuffer(bytes(range(7, 55)), dtype=ptss.METER_STATE_DTYPE).copy()   # garbage in, garbage pixels out: no address depends on it
    for bits in (garbage, np.frombuffer(b"\xff" * 48, dtype=ptss.METER_STATE_DTYPE).copy()):
        linear, pixels, history = (small.resolve_splat if splat else small.resolve_linear)(film, metered=bits)
        assert len(linear) == len(pixels) == len(history) == 700
        c.launches[2] += 1


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement):
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params, meter = ptss.linear_params(exposure=1.25), ptss.meter_params(rate=0.5)
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = linear_film(N)
    state = want_state = None
    exposures = []
    for k in range(4):   # four rounds: generate, refill trace, accumulate; zero, meter, update; metered resolve
        what = (placement, k)
        rays, rng = r.generate_rays(film_cam, rng)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        film = r.accumulate_paths_linear(res, film, params=params)
        shadow, _ = ptss.probe_accumulate_linear(res, shadow, params=params)   # the probe fed the device's own trace results
        assert film.tobytes() == shadow.tobytes(), what
        h = r.meter_linear(film)
        want_h = ptss.probe_meter_linear(shadow)
        assert np.array_equal(h, want_h) and int(h.sum()) == N, what
        state = r.meter_exposure(h, state, params, meter)
        want_state = ptss.probe_meter_exposure(want_h, want_state, params, meter)
        assert state_equal(state, want_state), what
        exposures.append(float(state["exposure"][0]))
        linear, pixels, history = r.resolve_linear(film, params=params, metered=state)
        at = ptss.linear_params(exposure=float(want_state["exposure"][0] * np.float32(1.25)))
        want_linear, want_pixels, want_history = ptss.probe_resolve_linear(shadow, params=at)
        assert same_words(linear, want_linear) and np.array_equal(pixels, want_pixels) and same_words(history, want_history), what
    assert r.meter_launches() == (4, 4, 4) and r.linear_launches() == (4, 0) and all(0 < e < 65536 for e in exposures) and len(set(exposures)) > 1
    assert 0 < int(pixels[:, :3].max()) and int(pixels[:, :3].min()) < 255
    film_cam.jitter = 0
    feat = r.ray_features(r.generate_rays(film_cam, rng)[0])
    dn = ptss.default_denoise_params(levels=2)
    want, _ = ptss.probe_denoise_history(want_history, feat, W, H, dn)
    assert np.array_equal(r.denoise_history(history=history, features=feat, levels=2), want)
    r.close()


# ---- 5. no trace in frame state; a second stream; two shards -------------------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    Pf = 80 * 30
    params, meter = ptss.linear_params(exposure=0.7), ptss.meter_params()
    films = {False: rows_film(False, Pf), True: rows_film(True, Pf)}
    want = {}
    for splat, film in films.items():
        h = (ptss.probe_meter_splat if splat else ptss.probe_meter_linear)(film)
        s = ptss.probe_meter_exposure(h, None, params, meter)
        at = ptss.linear_params(exposure=float(s["exposure"][0] * np.float32(0.7)))
        want[splat] = (h, s) + (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(film, params=at)
    side = torch.cuda.Stream()
    d_films = {splat: torch.from_numpy(film.view(np.int64).reshape(-1, 4).copy()).cuda() for splat, film in films.items()}
    for tick in range(20):   # twenty frames with the calls after each
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        for splat, film in films.items():   # on the context's stream
            h = (r.meter_splat if splat else r.meter_linear)(film)
            s = r.meter_exposure(h, None, params, meter)
            linear, px, hs = (r.resolve_splat if splat else r.resolve_linear)(film, params=params, metered=s)
            w = want[splat]
            assert np.array_equal(h, w[0]) and state_equal(s, w[1]) and same_words(linear, w[2]) and np.array_equal(px, w[3]) and same_words(hs, w[4]), tick
        with torch.cuda.stream(side):   # and on a second one, nothing leaving the device in between
            outs = {}
            for splat, d_film in d_films.items():
                d_h = torch.zeros(BINS, dtype=torch.int32, device="cuda")
                d_s = torch.zeros(6, dtype=torch.int64, device="cuda")
                d_linear = torch.zeros((Pf, 4), dtype=torch.float32, device="cuda")
                d_px = torch.zeros((Pf, 4), dtype=torch.uint8, device="cuda")
                d_hs = torch.zeros((Pf, 4), dtype=torch.float32, device="cuda")
                (r.meter_splat if splat else r.meter_linear)(d_film, histogram=d_h)
                r.meter_exposure(d_h, d_s, params, meter)
                (r.resolve_splat if splat else r.resolve_linear)(d_film, params=params, linear=d_linear, pixels=d_px, history=d_hs, metered=d_s)
                outs[splat] = (d_h, d_s, d_linear, d_px, d_hs)
        side.synchronize()
        for splat, (d_h, d_s, d_linear, d_px, d_hs) in outs.items():
            w = want[splat]
            assert np.array_equal(d_h.cpu().numpy().view(np.uint32), w[0]) and state_equal(d_s.cpu().numpy(), w[1]), tick
            assert same_words(d_linear.cpu().numpy(), w[2]) and np.array_equal(d_px.cpu().numpy(), w[3]) and same_words(d_hs.cpu().numpy(), w[4]), tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "twenty frames with the meter calls after each", W, H, 1)
    assert r.meter_launches() == (80, 80, 80) and r.linear_launches() == (0, 0) and r.splat_stats()[:3] == (0, 0, 0) and r.film_launches() == (0, 0, 0)
    o.close()
    r.close()


def test_two_shards_meter_into_one_histogram():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    film = rows_film(False, N)
    want = ptss.probe_meter_linear(film)
    want_state = ptss.probe_meter_exposure(want)
    h = None
    for rank in (0, 1):   # two shards, each metering its half of the film into the histogram the other one adds to
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8)
        h = r.meter_linear(film, first_pixel=rank * (N // 2), count=N // 2, histogram=h)
        whole = r.meter_linear(film)   # and all of the film, whatever rows the shard owns
        assert np.array_equal(whole, want), rank
        assert state_equal(r.meter_exposure(whole), want_state), rank
        assert r.meter_launches() == (2, 1, 0)
        r.close()
    assert np.array_equal(h, want)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    Pf = 20 * 15
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("m_film", Pf * 32), ("m_hist", BINS * 4), ("m_state", 48), ("m_lin", Pf * 16), ("m_pix", Pf * 4), ("m_hhist", Pf * 16))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_film, d_h, d_s, d_lin, d_pix, d_hist = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    host_film = rows_film(False, Pf)
    ptss._hip_check(Hip.hipMemcpy(d_film, host_film.ctypes.data, host_film.nbytes, 1), "hipMemcpy")
    good, film_params = ptss.meter_params(), ptss.linear_params()
    ref = lambda s: C.byref(s) if s is not None else None
    meters = (L.ptss_meter_linear, L.ptss_meter_splat)
    resolves = (L.ptss_resolve_linear_metered, L.ptss_resolve_splat_metered)
    exp = lambda ctx, h, s, params=film_params, meter=good: L.ptss_meter_exposure(ctx, h, ref(params), ref(meter), s, None)
    rsv = lambda call, ctx, film, first, count, s, lin, pix, hist, params=film_params: call(ctx, film, first, count, ref(params), s, lin, pix, hist, None)
    for call in meters:
        assert call(r._ctx, d_film, 0, Pf, d_h, None) == 0
    assert exp(r._ctx, d_h, d_s) == 0
    for call in resolves:
        assert rsv(call, r._ctx, d_film, 0, Pf, d_s, d_lin, d_pix, d_hist) == 0
    r.synchronize()
    counters, kernels = r.meter_launches(), r.launched_kernels()
    assert counters == (2, 1, 2)

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    ranges = ((0, 2 ** 31), (2 ** 31, 1), (2 ** 31 - 1, 1), (2 ** 30, 2 ** 30), (2 ** 63, 2 ** 63))
    for call in meters:
        assert call(None, d_film, 0, Pf, d_h, None) == EINVAL and call(r._ctx, None, 0, Pf, d_h, None) == EINVAL and call(r._ctx, d_film, 0, Pf, None, None) == EINVAL
        for k in (4, 8, 12):
            assert call(r._ctx, off(d_film, k), 0, Pf - 1, d_h, None) == EINVAL, k
        for k in (1, 2, 3):
            assert call(r._ctx, d_film, 0, Pf, off(d_h, k), None) == EINVAL, k
        for first, count in ranges:
            assert call(r._ctx, d_film, first, count, d_h, None) == ERANGE, (first, count)
        assert call(r._ctx, None, 0, 0, None, None) == 0   # count = 0
    # ptss_meter_exposure
    assert exp(None, d_h, d_s) == EINVAL and exp(r._ctx, None, d_s) == EINVAL and exp(r._ctx, d_h, None) == EINVAL
    assert exp(r._ctx, d_h, d_s, None) == EINVAL and exp(r._ctx, d_h, d_s, film_params, None) == EINVAL
    for k in (1, 2, 3):
        assert exp(r._ctx, off(d_h, k), d_s) == EINVAL, k
    for k in (1, 2, 4, 12):
        assert exp(r._ctx, d_h, off(d_s, k)) == EINVAL, k
    nan, inf = float("nan"), float("inf")
    for change in (dict(structSize=28), dict(structSize=0), dict(key=0.0), dict(key=-0.18), dict(key=nan), dict(key=inf), dict(lowPermille=1000),
                   dict(highPermille=1000), dict(lowPermille=500, highPermille=500), dict(rate=-0.01), dict(rate=1.01), dict(rate=nan),
                   dict(minExposure=-1.0), dict(minExposure=nan), dict(maxExposure=inf), dict(maxExposure=-1.0), dict(minExposure=2.0, maxExposure=1.0),
                   dict(reserved=1)):
        meter = ptss.meter_params()
        for k, v in change.items():
            setattr(meter, k, v)
        assert exp(r._ctx, d_h, d_s, film_params, meter) == EINVAL, change
    bad_films = []
    for change in (dict(structSize=16), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=inf), dict(scaleLog2=32, clampMax=257.0),
                   dict(exposure=-0.5), dict(exposure=nan), dict(reserved=1)):
        params = ptss.linear_params(clamp_max=2.0 ** 20)
        for k, v in change.items():
            setattr(params, k, v)
        bad_films.append(params)
        assert exp(r._ctx, d_h, d_s, params) == EINVAL, change
    # the metered resolves: ptss_resolve_linear's refusals and the state's
    for call in resolves:
        assert rsv(call, None, d_film, 0, Pf, d_s, d_lin, d_pix, d_hist) == EINVAL and rsv(call, r._ctx, None, 0, Pf, d_s, d_lin, d_pix, d_hist) == EINVAL
        assert rsv(call, r._ctx, d_film, 0, Pf, None, d_lin, d_pix, d_hist) == EINVAL
        assert rsv(call, r._ctx, d_film, 0, Pf, d_s, d_lin, d_pix, d_hist, None) == EINVAL
        for k in (4, 8, 12):
            assert rsv(call, r._ctx, off(d_film, k), 0, Pf - 1, d_s, d_lin, d_pix, d_hist) == EINVAL, k
            assert rsv(call, r._ctx, d_film, 0, Pf, d_s, off(d_lin, k), d_pix, d_hist) == EINVAL, k
            assert rsv(call, r._ctx, d_film, 0, Pf, d_s, d_lin, d_pix, off(d_hist, k)) == EINVAL, k
        for k in (1, 2, 3):
            assert rsv(call, r._ctx, d_film, 0, Pf, d_s, d_lin, off(d_pix, k), d_hist) == EINVAL, k
        for k in (1, 2, 4, 12):
            assert rsv(call, r._ctx, d_film, 0, Pf, off(d_s, k), d_lin, d_pix, d_hist) == EINVAL, k
        for first, count in ranges:
            assert rsv(call, r._ctx, d_film, first, count, d_s, d_lin, d_pix, d_hist) == ERANGE, (first, count)
        for params in bad_films:
            assert rsv(call, r._ctx, d_film, 0, Pf, d_s, d_lin, d_pix, d_hist, params) == EINVAL
        assert rsv(call, r._ctx, None, 0, 0, None, None, None, None) == 0   # count = 0
        assert rsv(call, r._ctx, d_film, 0, Pf, d_s, None, None, None) == 0   # nothing asked for: nothing launched
    out3 = (C.c_ulonglong * 3)()
    assert L.ptss_meter_launches(None, out3) == EINVAL and L.ptss_meter_launches(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.meter_launches() == counters and r.launched_kernels() == kernels
    assert r.linear_launches() == (0, 0) and r.film_launches() == (0, 0, 0) and r.film_rejected() == 0
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: a 4-byte aligned histogram and pixels, an 8-byte aligned state, 16-byte steps of the film, the boundary parameters
    edge = ptss.meter_params(low_permille=999, high_permille=0, rate=0.0, min_exposure=0.0, max_exposure=0.0)
    assert L.ptss_meter_linear(r._ctx, off(d_film, 16), 0, Pf - 1, off(d_h, 4), None) == 0
    assert exp(r._ctx, off(d_h, 4), off(d_s, 8), params_of(32, 256.0, 0.0), edge) == 0
    assert rsv(L.ptss_resolve_linear_metered, r._ctx, off(d_film, 16), 0, Pf - 1, off(d_s, 8), off(d_lin, 16), off(d_pix, 4), None, params_of(32, 256.0, 0.0)) == 0
    r.synchronize()
    assert r.meter_launches() == (3, 2, 3) and r.launched_kernels() == kernels
    r.close()
