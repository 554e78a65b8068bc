"""Tone curves for the two linear films on the GPU (ptss_tone_build, ptss_resolve_toned). Every test requires the device
to equal the host probes byte for byte, in both forms of the lookup, and ptss_tone_launches to count what a call launches. The context is
a 16 x 16 cornell.

1. The table of every curve x transfer x bit depth. 2. The toned resolve against the probe: both film kinds, the plain, metered and glare
   sources, sub-ranges around the workgroup's 256 threads and 1024 pixels, NULL outputs, empty pixels, films whose words wrap, states of NaN,
   0 and +inf exposure. 3. Films that sit on every threshold and on both of its neighbours: every comparison of the search is taken both
   ways, and the levels produced are exactly 0 .. K. 4. The anchor: the clamp with the 2.2 power at 8 bits is the plain, metered and glare
   resolves. 5. The loop on `mixed` against a shadow loop of the probes; frames, a second stream, two shards. 6. Refusals."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import oracle
import ptss
from glare_common import film_of, same_bytes
from linear_common import linear_film, params_of, same_words
from meter_common import new_state, state_equal
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from splat_common import splat_film
from test_gpu_kernel_coverage import compare
from test_tone_cpu import CONFIGS, LUMINANCE_CONFIGS, TONE_REFUSED, changed, table_of, tone_of

pytestmark = pytest.mark.gpu
FILMS = ("linear", "splat")
FORMS = (1, 2)   # the table staged in LDS; the guess settled against global memory
COUNTS = (1, 255, 256, 257, 1000)
FIRSTS = (0, 3)


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


def outputs_equal(got, want):
    for a, b in zip(got, want):
        if (a is None) != (b is None):
            return False
        if a is not None and not (np.array_equal(a, b) if a.dtype == np.uint8 else same_words(a, b)):
            return False
    return True


class Checker:
    """Device against probe for one context, in both forms, keeping the two counters."""

    def __init__(self, r):
        self.r, self.launches = r, list(r.tone_launches())

    def counted(self, what):
        assert list(self.r.tone_launches()) == self.launches, (what, self.r.tone_launches(), self.launches)

    def resolve(self, what, film, tone, table, params, state=None, glare=None, forms=FORMS, **kw):
        call = self.r.resolve_splat if film.dtype == ptss.SPLAT_DTYPE else self.r.resolve_linear
        want = ptss.probe_resolve_toned(film, tone, table, params=params, state=state, glare=glare, **kw)
        launched = any(kw.get(k, True) is not None for k in ("linear", "pixels", "history")) and kw.get("count", 1) != 0
        for form in forms:
            self.r.debug_tone_form(form)
            got = call(film, params=params, metered=state, glare=glare, tone=(tone, table), **kw)
            assert outputs_equal(got, want), (what, form)
            self.launches[1] += 1 if launched else 0
            self.counted((what, form))
        self.r.debug_tone_form(0)
        return want


def levels_of(pixels, bits):
    """(P, 3) levels of the words' bytes."""
    if bits == 10:
        return ptss.unpack_pixels10(pixels)[:, :3].astype(np.int64)
    return pixels[:, :3].astype(np.int64)


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------------------------
def test_the_table_equals_the_probe_for_every_curve_transfer_and_depth(small):
    before = small.tone_launches()
    for cfg in CONFIGS + LUMINANCE_CONFIGS:
        tone = tone_of(cfg)
        got = small.tone_build(tone)
        assert same_words(got.reshape(1, -1), table_of(cfg).reshape(1, -1)) and ptss.tone_table_sorted(got), cfg
    after = small.tone_launches()
    assert (after[0] - before[0], after[1] - before[1]) == (len(CONFIGS + LUMINANCE_CONFIGS), 0)
    for tone in (ptss.tone_params("reinhard", white=0.25, bits=10), ptss.tone_params("reinhard", white=65536.0),
                 ptss.tone_params("filmic", filmic=(0.0, 1.0, 0.0, 1.0, 1.0)), ptss.tone_params("filmic", "gamma22", 10, filmic=(1.0, 10.0, 2.0, 0.0, 1.0))):
        assert same_words(small.tone_build(tone).reshape(1, -1), ptss.probe_tone_build(tone).reshape(1, -1))   # NaN tails: levels no input reaches


# ---- 2. the resolve against the probe ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_the_toned_resolve_equals_the_probe(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    configs = CONFIGS + LUMINANCE_CONFIGS
    params = params_of(20, 65536.0, exposure=0.75)
    state = new_state()
    state["exposure"], state["updates"] = 2.5, 3
    film = film_of(40, 26, splat, params, seed=4)   # 1040 pixels, empty ones among them
    gw, gh = 33, 9
    gfilm = film_of(gw, gh, splat, params, seed=5)
    glare = ptss.glare_params(levels=3, mode="add", threshold=0.125, strength=0.5)
    pyr = ptss.probe_glare_build(gfilm, gw, gh, params, glare)
    big = film_of(33, 31, splat, params, seed=6)     # 1023 pixels: the glare source's count of 1000
    big_pyr = ptss.probe_glare_build(big, 33, 31, params, glare)
    k = 0
    for first in FIRSTS:
        for count in COUNTS:
            cfg = configs[k % len(configs)]
            k += 1
            tone, table = tone_of(cfg), table_of(cfg)
            c.resolve(("plain", first, count, cfg), film, tone, table, params, first_pixel=first, count=count)
            c.resolve(("metered", first, count, cfg), film, tone, table, params, state, first_pixel=first, count=count)
            if first + count <= gw * gh:
                c.resolve(("glare", first, count, cfg), gfilm, tone, table, params, state if count % 2 else None, (gw, gh, glare, pyr), first_pixel=first, count=count)
            else:
                c.resolve(("glare", first, count, cfg), big, tone, table, params, state, (33, 31, glare, big_pyr), first_pixel=first, count=count)
    for cfg in configs:   # every configuration over the whole film, and over the glare film
        c.resolve(("whole", cfg), film, tone_of(cfg), table_of(cfg), params, state)
        c.resolve(("whole glare", cfg), gfilm, tone_of(cfg), table_of(cfg), params, None, (gw, gh, glare, pyr), forms=(1 + k % 2,))
        k += 1
    cfg = ("filmic", "srgb", 10, False)
    tone, table = tone_of(cfg), table_of(cfg)
    P = len(film)
    before = dict(linear=np.full((P, 4), -3.0, np.float32), pixels=np.full((P, 4), 9, np.uint8), history=np.full((P, 4), -2.0, np.float32))
    for mask in range(8):   # each combination of NULL outputs; what lies outside the range keeps its bytes
        kw = {name: (before[name] if mask & (1 << i) else None) for i, name in enumerate(("linear", "pixels", "history"))}
        outs = c.resolve(("outputs", mask), film, tone, table, params, state if mask & 1 else None, first_pixel=65, count=257, **kw)
        for out, was in zip(outs, (before["linear"], before["pixels"], before["history"])):
            if out is not None:
                rows = np.ascontiguousarray(out).view(was.dtype).reshape(-1, 4)
                assert np.array_equal(rows[:65], was[:65]) and np.array_equal(rows[322:], was[322:]) and not np.array_equal(rows[65:322], was[65:322])
    c.resolve("count = 0", film, tone, table, params, first_pixel=10, count=0)
    high = film_of(37, 21, splat, params, kind="high")   # sums no call of the library leaves: the words wrap on both sides alike
    c.resolve("a film whose words wrap", high, tone, table, params, state)
    for exposure in (float("nan"), 0.0, float("inf"), -1.0):   # garbage pixels, the probe's, never a fault: no address depends on a value
        for cfg in (("filmic", "srgb", 10, False), ("reinhard", "gamma22", 8, True), ("clamp", "gamma22", 8, False)):
            state["exposure"] = exposure
            c.resolve(("exposure", exposure, cfg), film, tone_of(cfg), table_of(cfg), params, state)
            c.resolve(("exposure with glare", exposure, cfg), gfilm, tone_of(cfg), table_of(cfg), params, state, (gw, gh, glare, pyr), forms=(2,))


# ---- 3. films on every threshold ----------------------------------------------------------------------------------------------------------------------
def threshold_film(table, K, splat):
    """One pixel per threshold at scaleLog2 = 32: m - 1, m, m + 1 in its three channels, m = T[k] * 2^32 rounded up to an integer (the least
    fixed-point value at or above the threshold; a threshold below 2^-32 gives m = 1). One sample, or a weight of 1."""
    ks = [k for k in range(1, K + 1) if not np.isnan(table[k])]
    f = splat_film(len(ks) + 2) if splat else linear_film(len(ks) + 2)
    for i, k in enumerate(ks):
        m = max(int(-(-Fraction(float(table[k])) * (1 << 32) // 1)), 1)
        f["r"][i], f["g"][i], f["b"][i] = m - 1, m, m + 1
    f["r"][len(ks)] = f["g"][len(ks)] = f["b"][len(ks)] = 255 << 32   # far above display white
    if splat:
        f["weight"] = 65536
        f["weight"][len(ks) + 1] = 0
    else:
        f["samples"] = 1
        f["samples"][len(ks) + 1] = 0
    return f


@pytest.mark.parametrize("kind", FILMS)
def test_films_on_every_threshold_produce_every_level(small, kind):
    splat = kind == "splat"
    c = Checker(small)
    params = params_of(32, 256.0)
    for cfg in CONFIGS + LUMINANCE_CONFIGS:
        curve, transfer, bits, luminance = cfg
        K = (1 << bits) - 1
        tone, table = tone_of(cfg), table_of(cfg)
        film = threshold_film(table, K, splat)
        want = c.resolve(("thresholds", cfg), film, tone, table, params)
        levels = levels_of(want[1], bits)
        if not luminance or curve == "clamp":   # the channel input is the film's value itself (under the clamp s = div(Y, Y) = 1 while Y <= 1)
            assert set(np.unique(levels).tolist()) == set(range(K + 1)), cfg
            if not np.isnan(table[1:K + 1]).any():   # m itself is at its threshold and below the next one: (float)m 2^-32 is exact there or tiny
                assert (levels[:K, 1] == np.arange(1, K + 1)).all() and (levels[:K, 0] <= levels[:K, 1]).all() and (levels[:K, 1] <= levels[:K, 2]).all(), cfg
        else:
            assert len(np.unique(levels)) > K // 4, cfg


# ---- 4. the anchor --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_the_clamp_at_8_bits_is_the_plain_the_metered_and_the_glare_resolve(small, kind):
    splat = kind == "splat"
    params = params_of(20, 65536.0, exposure=1.5)
    w, h = 37, 21
    film = film_of(w, h, splat, params, seed=7)
    cfg = ("clamp", "gamma22", 8, False)
    tone = tone_of(cfg)
    table = small.tone_build(tone)
    state = new_state()
    state["exposure"], state["updates"] = 0.6, 1
    glare = ptss.glare_params(levels=4, mode="add", threshold=0.25, strength=0.3)
    pyr = small.glare_build(film, w, h, params, glare)
    resolve = small.resolve_splat if splat else small.resolve_linear
    for form in FORMS:
        small.debug_tone_form(form)
        for kw in (dict(), dict(metered=state), dict(glare=(w, h, glare, pyr)), dict(metered=state, glare=(w, h, glare, pyr))):
            for a, b in zip(resolve(film, params=params, tone=(tone, table), **kw), resolve(film, params=params, **kw)):
                assert a.tobytes() == b.tobytes(), (form, sorted(kw))
    small.debug_tone_form(0)


# ---- 5. the loop, frames, a second stream, two shards ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FILMS)
def test_the_loop_equals_a_shadow_loop_of_the_probes(kind):
    name, iterations = "mixed", 4
    splat = kind == "splat"
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params, meter, flt = ptss.linear_params(exposure=1.25), ptss.meter_params(rate=0.5), ptss.splat_filter("tent", 1.5)
    glare = ptss.glare_params(levels=5, mode="add", threshold=0.25, strength=0.25)
    cfgs = (("filmic", "srgb", 8, False), ("reinhard", "srgb", 10, True), ("filmic", "gamma22", 10, False))
    tables = [r.tone_build(tone_of(cfg)) for cfg in cfgs]
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = splat_film(N) if splat else linear_film(N)
    state = want_state = None
    for k in range(3):   # generate, trace, accumulate (with moments) or splat; meter, update; glare build; toned resolve
        what = (kind, k)
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=flt, params=params, homed_first_pixel=0)
            shadow = ptss.probe_splat_paths(res, pos, shadow, W, H, filter=flt, params=params, homed_first_pixel=0)[0]
        else:
            film = r.accumulate_paths_linear(res, film, params=params)
            shadow = ptss.probe_accumulate_linear(res, shadow, params=params)[0]
        assert film.tobytes() == shadow.tobytes(), what
        h = (r.meter_splat if splat else r.meter_linear)(film)
        state = r.meter_exposure(h, state, params, meter)
        want_state = ptss.probe_meter_exposure((ptss.probe_meter_splat if splat else ptss.probe_meter_linear)(shadow), want_state, params, meter)
        assert state_equal(state, want_state), what
        pyr = r.glare_build(film, W, H, params, glare)
        want_pyr = ptss.probe_glare_build(shadow, W, H, params, glare)
        assert same_bytes(pyr, want_pyr), what
        cfg, table = cfgs[k], tables[k]
        assert same_words(table.reshape(1, -1), table_of(cfg).reshape(1, -1)), what
        got = (r.resolve_splat if splat else r.resolve_linear)(film, params=params, metered=state, glare=(W, H, glare, pyr), tone=(tone_of(cfg), table))
        want = ptss.probe_resolve_toned(shadow, tone_of(cfg), table_of(cfg), params=params, state=want_state, glare=(W, H, glare, want_pyr))
        assert outputs_equal(got, want), what
        levels = levels_of(got[1], cfg[2])
        assert 0 < levels.max() and levels.min() < (1 << cfg[2]) - 1 and len(np.unique(levels)) > 16, what
    assert r.tone_launches() == (3, 3)
    r.close()


def test_frames_a_second_stream_and_two_shards():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    w, h = 65, 34
    P = w * h
    params = params_of(20, 65536.0)
    cfg = ("filmic", "srgb", 10, False)
    tone = tone_of(cfg)
    films = {splat: film_of(w, h, splat, params, seed=3) for splat in (False, True)}
    want = {splat: ptss.probe_resolve_toned(film, tone, table_of(cfg), params=params) for splat, film in films.items()}
    side = torch.cuda.Stream()
    dev = {splat: torch.from_numpy(film.view(np.int64).reshape(-1, 4).copy()).cuda() for splat, film in films.items()}
    d_table = torch.zeros(ptss.tone_table_floats(10), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for tick in range(4):   # four frames with the calls after each, on the context's stream and on a second one
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        for splat, film in films.items():
            got = (r.resolve_splat if splat else r.resolve_linear)(film, params=params, tone=(tone, r.tone_build(tone)))
            assert outputs_equal(got, want[splat]), tick
            outs = [torch.zeros((P, 4), dtype=t, device="cuda") for t in (torch.float32, torch.uint8, torch.float32)]
            with torch.cuda.stream(side):
                r.tone_build(tone, d_table)
                (r.resolve_splat if splat else r.resolve_linear)(dev[splat], params=params, linear=outs[0], pixels=outs[1], history=outs[2], tone=(tone, d_table))
            side.synchronize()
            assert outputs_equal([x.cpu().numpy() for x in outs], want[splat]), tick
        assert r.launched_kernels() == before, tick   # the tone kernels own no bit
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "four frames with the tone calls after each", W, H, 1)
    assert r.tone_launches() == (16, 16)
    o.close()
    r.close()
    for rank in (0, 1):
        s = ptss.Renderer(scene, 64, 48, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8)
        table = s.tone_build(tone)
        assert outputs_equal(s.resolve_linear(films[False], params=params, tone=(tone, table)), want[False]), rank
        assert s.tone_launches() == (1, 1)
        s.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    w, h = 20, 15
    Pf = w * h
    entries = ptss.glare_layout(w, h, 4)[1]
    floats = ptss.tone_table_floats(10)
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("t_film", Pf * 32), ("t_pyr", entries * 32), ("t_state", 48), ("t_table", floats * 4), ("t_lin", Pf * 16), ("t_pix", Pf * 4), ("t_hist", Pf * 16))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_film, d_pyr, d_s, d_table, d_lin, d_pix, d_hist = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    film_params, glare, good = ptss.linear_params(), ptss.glare_params(levels=4), ptss.tone_params(bits=10)
    host_film = film_of(w, h, False, film_params)
    ptss._hip_check(Hip.hipMemcpy(d_film, host_film.ctypes.data, host_film.nbytes, 1), "hipMemcpy")
    ref = lambda s: C.byref(s) if s is not None else None

    def build(ctx, table, tone=good):
        return L.ptss_tone_build(ctx, ref(tone), table, None)

    def rsv(ctx=r._ctx, film=d_film, kind=0, first=0, count=Pf, params=film_params, tone=good, table=d_table, s=d_s, width=w, height=h, g=glare, pyr=d_pyr,
            lin=d_lin, pix=d_pix, hist=d_hist):
        return L.ptss_resolve_toned(ctx, film, kind, first, count, ref(params), ref(tone), table, s, width, height, ref(g), pyr, lin, pix, hist, None)

    assert build(r._ctx, d_table) == 0 and rsv() == 0 and rsv(kind=1, g=None, pyr=None, s=None) == 0
    r.synchronize()
    counters, kernels = r.tone_launches(), r.launched_kernels()
    assert counters == (1, 2)

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    bad_tones = [changed(lambda: ptss.tone_params(bits=10), **change) for change in TONE_REFUSED]
    assert build(None, d_table) == EINVAL and build(r._ctx, None) == EINVAL and build(r._ctx, d_table, None) == EINVAL
    for k in (4, 8, 12):
        assert build(r._ctx, off(d_table, k)) == EINVAL
    for tone in bad_tones:
        assert build(r._ctx, d_table, tone) == EINVAL and rsv(tone=tone) == EINVAL and rsv(tone=tone, g=None, pyr=None) == EINVAL
    assert rsv(ctx=None) == EINVAL and rsv(film=None) == EINVAL and rsv(table=None) == EINVAL and rsv(pyr=None) == EINVAL and rsv(g=None) == EINVAL
    assert rsv(params=None) == EINVAL and rsv(tone=None) == EINVAL
    for kind in (2, -1, 77):
        assert rsv(kind=kind) == EINVAL
    for k in (4, 8, 12):
        assert rsv(film=off(d_film, k), count=Pf - 1) == EINVAL and rsv(table=off(d_table, k)) == EINVAL and rsv(pyr=off(d_pyr, k)) == EINVAL
        assert rsv(lin=off(d_lin, k)) == EINVAL and rsv(hist=off(d_hist, k)) == EINVAL
    for k in (1, 2, 3):
        assert rsv(pix=off(d_pix, k)) == EINVAL
    for k in (1, 2, 4, 12):
        assert rsv(s=off(d_s, k)) == EINVAL
    for first, count in ((0, Pf + 1), (Pf, 1), (1, Pf), (0, 2 ** 31), (2 ** 31, 1), (2 ** 63, 2 ** 63)):
        assert rsv(first=first, count=count) == ERANGE, (first, count)
    for first, count in ((0, 2 ** 31), (2 ** 31, 1), (2 ** 63, 2 ** 63)):
        assert rsv(first=first, count=count, g=None, pyr=None) == ERANGE, (first, count)
    for change in (dict(structSize=16), dict(scaleLog2=33), dict(clampMax=0.0), dict(exposure=-0.5), dict(reserved=1)):
        assert rsv(params=changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change)) == EINVAL
    assert rsv(g=changed(lambda: ptss.glare_params(levels=4), levels=9)) == EINVAL
    for width, height in ((0, h), (w, 0), (2 ** 22 + 1, 1), (46341, 46341)):
        assert rsv(count=1, width=width, height=height) == ERANGE
    assert rsv(film=None, count=0, table=None, pyr=None, s=None, lin=None, pix=None, hist=None) == 0   # count = 0
    assert rsv(lin=None, pix=None, hist=None) == 0   # nothing asked for: nothing launched
    out2 = (C.c_ulonglong * 2)()
    assert L.ptss_tone_launches(None, out2) == EINVAL and L.ptss_tone_launches(r._ctx, None) == EINVAL
    assert L.ptss_debug_tone_form(r._ctx, 3) == EINVAL and L.ptss_debug_tone_form(r._ctx, -1) == EINVAL and L.ptss_debug_tone_form(None, 1) == EINVAL
    assert L.ptss_tone_table_floats(8) == 260 and L.ptss_tone_table_floats(10) == 1028 and L.ptss_tone_table_floats(9) == 0
    r.synchronize()
    assert r.tone_launches() == counters and r.launched_kernels() == kernels
    assert r.linear_launches() == (0, 0) and r.meter_launches() == (0, 0, 0) and r.glare_launches() == (0, 0, 0)
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 16-byte steps of the film, an 8-byte aligned state or none, 4-byte aligned pixels, width and height of anything without a pyramid
    assert rsv(film=off(d_film, 16), count=Pf - 1, s=off(d_s, 8), lin=off(d_lin, 16), pix=off(d_pix, 4), hist=None, g=None, pyr=None, width=-5, height=0) == 0
    r.synchronize()
    assert r.tone_launches() == (1, 3)
    r.close()
