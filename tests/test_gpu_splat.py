"""The filtered linear film on the GPU (ptss_generate_rays_positions / ptss_splat_paths / ptss_splat_paths_homed / ptss_resolve_splat;
DESIGN.md §3.30). Every test requires the device to equal the host probes byte for byte, and the homed form to equal the scatter form. The
context is a 16 x 16 cornell; the film is 40 x 24, no multiple of the homed kernel's 16 x 16 tile.

1. Positions: the three cameras with and without jitter against the probe, rays and streams against ptss_generate_rays, an index with
   entries beyond the film. 2. Scatter: the rows of the CPU test for the three kinds and four radii in batches of 1, 63, 64, 65 and 257,
   permuted and split, 300 samples at one position, the carry from 2^62, the counters. 3. Homed: the full film, a batch from mid-row to
   mid-row, 1, 255, 256 and 257 samples, positions on the home square's corners and edges, strays; against the probe and the scatter call.
4. The box at radius 0.5 against the linear film's calls. 5. Resolve. 6. The loop against a shadow loop of the probes, the history
   through the denoiser. 7. No trace in frame state, a second stream, two shards. 8. Refusals."""
import ctypes as C

import numpy as np
import pytest

import ptss
from film_common import films, results_of, seeded_states, words
from linear_common import SCALES, params_of
from path_query_common import SCENES, camera_of, make_scene
from splat_common import (FH, FW, JITTER_SEED, film_words, filters, high_film, homed_positions, name_of, positions_of, radiance_rows, resolve_rows,
                          same_words, scatter_case, splat_film)

pytestmark = pytest.mark.gpu
P = FW * FH
FILTERS = filters()


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


class Checker:
    """Device against probe for one context, keeping the five counters of ptss_splat_stats."""

    def __init__(self, r):
        self.r, self.stats = r, list(r.splat_stats())

    def splat(self, what, res, pos, start, flt, params, homed=None, against_scatter=True):
        film = self.r.splat_paths(res, pos, start, FW, FH, filter=flt, params=params, homed_first_pixel=homed)
        want, dropped, clamped = ptss.probe_splat_paths(res, pos, start, FW, FH, filter=flt, params=params, homed_first_pixel=homed)
        assert film.tobytes() == want.tobytes(), what
        self.stats[0 if homed is None else 1] += 1 if len(res) else 0
        self.stats[3] += dropped
        self.stats[4] += clamped
        assert list(self.r.splat_stats()) == self.stats, what
        if homed is not None and against_scatter:   # the same non-stray samples through the atomic form: the same bytes
            keep = np.ones(len(res), bool)
            keep[[k for k in range(len(res)) if _stray(pos[k], homed + k)]] = False
            scatter = self.r.splat_paths(res[keep], pos[keep], start, FW, FH, filter=flt, params=params)
            assert scatter.tobytes() == film.tobytes(), what
            self.stats[0] += 1 if keep.any() else 0
            self.stats[4] += clamped   # (a sample inside its home square is inside the film: the scatter form drops none of them)
            assert list(self.r.splat_stats()) == self.stats, what
        return film

    def resolve(self, what, film, params, **kw):
        got = self.r.resolve_splat(film, params=params, **kw)
        want = ptss.probe_resolve_splat(film, params=params, **kw)
        for a, b in zip(got, want):
            assert (a is None) == (b is None), what
            assert a is None or (np.array_equal(a, b) if a.dtype == np.uint8 else same_words(a, b)), what
        launched = any(kw.get(k, True) is not None for k in ("linear", "pixels", "history")) and len(film) > 0 and kw.get("count", 1) != 0
        self.stats[2] += 1 if launched else 0
        assert list(self.r.splat_stats()) == self.stats, what
        return got


def _stray(at, home):
    hx, hy = home % FW, home // FW
    x, y = np.float32(at["x"]), np.float32(at["y"])
    return not (hx <= x <= hx + 1 and hy <= y <= hy + 1)


def long_scatter_case(n, seed=0):
    """The CPU test's scatter rows first, then random positions over the film and its rim, to n samples."""
    res, pos = scatter_case(seed)
    g = np.random.default_rng(seed + 5)
    more = n - len(pos)
    if more > 0:
        xy = np.stack([g.uniform(-2.5, FW + 2.5, more), g.uniform(-2.5, FH + 2.5, more)], axis=1).astype(np.float32)
        xy[::7] = np.round(xy[::7])
        pos = np.concatenate([pos, positions_of(xy)])
        res = radiance_rows(n, seed)
    return res[:n], pos[:n]


# ---- 1. positions ------------------------------------------------------------------------------------------------------------------------------
def test_positions_equal_the_probe_and_rays_equal_generate_rays(small):
    s0 = seeded_states(JITTER_SEED, P)
    launches = small.film_launches()[0]
    for cam in films(FW, FH):
        what = (cam.kind, cam.jitter)
        rays, rng, pos = small.generate_rays(cam, s0, positions=True)
        want_rays, want_rng, want_pos, _ = ptss.probe_film_positions(cam, s0)
        assert pos.tobytes() == want_pos.tobytes(), what
        plain_rays, plain_rng = small.generate_rays(cam, s0)   # a copy of the streams through ptss_generate_rays
        assert words(rays).tobytes() == words(plain_rays).tobytes() and words(rng).tobytes() == words(plain_rng).tobytes(), what
        assert words(rays).tobytes() == words(want_rays).tobytes() and words(rng).tobytes() == words(want_rng).tobytes(), what
        for n in (1, 65, 257):   # from a first pixel above 0
            rays, rng, pos = small.generate_rays(cam, s0[:n], first_pixel=333, positions=True)
            _, _, want_pos, _ = ptss.probe_film_positions(cam, s0[:n], first_pixel=333)
            assert pos.tobytes() == want_pos.tobytes(), (what, n)
        launches += 5
    assert small.film_launches()[0] == launches
    cam = ptss.film_camera("thinlens", FW, FH, jitter=1, lens_radius=0.2, focus_distance=4.0)
    index = np.arange(P, dtype=np.uint32)[::-1].copy()
    index[::5] = P + np.arange(len(index[::5]))
    index[3] = 2 ** 32 - 1
    before, rejected = np.full((P, 8), 7.0, np.float32), small.film_rejected()
    rays, rng, pos = small.generate_rays(cam, s0, index=index, rays=before, positions=True)
    want_rays, want_rng, want_pos, dropped = ptss.probe_film_positions(cam, s0, index=index, rays=before)
    out = index >= P
    assert dropped == out.sum() and small.film_rejected() == rejected + dropped
    assert words(rays).tobytes() == words(want_rays).tobytes() and words(rng).tobytes() == words(want_rng).tobytes()
    assert (words(rays)[out].view(np.float32) == 7.0).all() and words(rng)[out].tobytes() == words(s0)[out].tobytes()
    assert np.isnan(pos["x"][out]).all() and np.isnan(pos["y"][out]).all() and pos[~out].tobytes() == want_pos[~out].tobytes()


# ---- 2. scatter --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", FILTERS, ids=name_of)
def test_scatter_equals_the_probe(small, flt):
    c, params = Checker(small), ptss.linear_params()
    res, pos = long_scatter_case(600)
    used = splat_film()
    g = np.random.default_rng(3)
    used["r"], used["g"], used["b"], used["weight"] = g.integers(0, 2 ** 50, P), g.integers(0, 2 ** 33, P), 7, g.integers(0, 2 ** 30, P)
    film = c.splat("the rows", res, pos, used, flt, params)
    assert c.stats[3] > 0 and c.stats[4] > 0 and film.tobytes() != used.tobytes()
    for n in (1, 63, 64, 65, 257):
        for first in (0, 40):
            c.splat(("a batch", n, first), res[first:first + n], pos[first:first + n], splat_film(), flt, params)
    c.splat("nothing", res[:0], pos[:0], used, flt, params)
    at = positions_of([(17.25, 9.25)] * 300)   # 300 samples at one position: every atomic of a wave on the same entries
    film = c.splat("300 samples at one position", radiance_rows(300, 1), at, splat_film(), flt, params)
    assert np.count_nonzero(film["weight"]) <= 16
    hi = params_of(20, 2.0 ** 20)   # q = 2^40 on a film whose sums start at 2^62
    top = results_of(np.full((300, 3), 2.0 ** 20, np.float32))
    film = c.splat("the carry from 2^62", top, at, high_film(), flt, hi)
    assert int(film["r"].max()) > (1 << 62) + 300 * (1 << 35)
    c.splat("the carry, spread", top, pos[:300], high_film(), flt, hi)


@pytest.mark.parametrize("seed", range(3))
def test_a_batch_permuted_and_split_gives_the_same_bytes(small, seed):
    g = np.random.default_rng(40 + seed)
    flt = FILTERS[(seed * 5 + 1) % len(FILTERS)]
    params = params_of(*SCALES[seed])
    res, pos = long_scatter_case(1500, seed)
    start = high_film() if seed == 1 else splat_film()
    whole = small.splat_paths(res, pos, start, FW, FH, filter=flt, params=params)
    assert whole.tobytes() == ptss.probe_splat_paths(res, pos, start, FW, FH, filter=flt, params=params)[0].tobytes()
    for _ in range(2):
        order = g.permutation(len(res))
        assert small.splat_paths(res[order], pos[order], start, FW, FH, filter=flt, params=params).tobytes() == whole.tobytes()
        cut = int(g.integers(1, len(res)))
        first = small.splat_paths(res[order][:cut], pos[order][:cut], start, FW, FH, filter=flt, params=params)
        assert small.splat_paths(res[order][cut:], pos[order][cut:], first, FW, FH, filter=flt, params=params).tobytes() == whole.tobytes()


# ---- 3. homed ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", FILTERS, ids=name_of)
def test_homed_equals_the_probe_and_the_scatter_call(small, flt):
    c, params = Checker(small), ptss.linear_params()
    K = int(flt.radius + 0.5)
    pos, stray = homed_positions(0, P)
    film = c.splat("the full film", radiance_rows(P, 2), pos, splat_film(), flt, params, homed=0)
    assert stray.sum() > 0 and np.count_nonzero(film["weight"]) > P // 5   # (half the positions sit on an edge, where a narrow tent is 0)
    first, n = FW * 7 + 17, FW * 6 + 11   # from mid-row to mid-row: rows 7 .. 13
    pos, stray = homed_positions(first, n, seed=1)
    used = high_film()
    film = c.splat("mid-row to mid-row", radiance_rows(n, 3), pos, used, flt, params, homed=first)
    rows = film_words(film).reshape(FH, FW, 4)
    was = film_words(used).reshape(FH, FW, 4)
    assert np.array_equal(rows[:7 - K], was[:7 - K]) and np.array_equal(rows[14 + K:], was[14 + K:])   # beyond the dilated rows: untouched
    if flt.radius >= 1.0:   # the rows beside the batch receive their taps (a radius of 0.5 reaches them only from a sample on the shared edge)
        assert not np.array_equal(rows[6], was[6]) and not np.array_equal(rows[14], was[14])
    if flt.radius == 2.0 and flt.alpha <= 2.0:   # (the steep Gaussian is below a weight of 2^-17 one and a half pixels out)
        assert not np.array_equal(rows[5], was[5]) and not np.array_equal(rows[15], was[15])
    for n in (1, 255, 256, 257):
        for first in (0, 13, P - n):
            pos, _ = homed_positions(first, n, seed=n)
            c.splat(("a batch", n, first), radiance_rows(n, n), pos, splat_film(), flt, params, homed=first)
    hi = params_of(20, 2.0 ** 20)
    pos, _ = homed_positions(FW - 3, 300, seed=9)
    c.splat("the carry from 2^62", results_of(np.full((300, 3), 2.0 ** 20, np.float32)), pos, high_film(), flt, hi, homed=FW - 3)
    bad = positions_of(np.full((70, 2), np.nan, np.float32))   # nothing but strays: nothing written, every sample counted
    film = c.splat("strays only", radiance_rows(70, 0), bad, used, flt, params, homed=100, against_scatter=False)
    assert film.tobytes() == used.tobytes()


# ---- 4. the box at radius 0.5 is the linear film ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [0, 1])
def test_the_box_identity_against_the_linear_calls(small, jitter):
    box, params = ptss.splat_filter("box", 0.5), ptss.linear_params(exposure=0.8)
    cam = ptss.film_camera("pinhole", FW, FH, jitter=jitter)
    rng = seeded_states(JITTER_SEED, P)   # (test_splat_cpu: no position these streams give lies on an integer)
    homed = scatter = splat_film()
    linear = np.zeros(P, ptss.LINEAR_DTYPE)
    for k in range(3):
        _, rng, pos = small.generate_rays(cam, rng, positions=True)
        res = radiance_rows(P, seed=k)
        homed = small.splat_paths(res, pos, homed, FW, FH, filter=box, params=params, homed_first_pixel=0)
        scatter = small.splat_paths(res, pos, scatter, FW, FH, filter=box, params=params)
        linear = small.accumulate_paths_linear(res, linear, params=params)
        assert homed.tobytes() == scatter.tobytes(), k
        assert all(np.array_equal(homed[ch], linear[ch]) for ch in "rgb") and np.array_equal(homed["weight"], linear["samples"].astype(np.uint64) << 16), k
        for a, b in zip(small.resolve_splat(homed, params=params), small.resolve_linear(linear, params=params)):
            assert a.tobytes() == b.tobytes(), k


# ---- 5. resolve ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_log2, clamp_max", SCALES)
def test_resolve_equals_the_probe(small, scale_log2, clamp_max):
    c = Checker(small)
    for exposure in (0.0, 1.0, 0.37, 40.0):
        params = params_of(scale_log2, clamp_max, exposure)
        c.resolve(("the rows of the CPU test", exposure), resolve_rows(params), params)
    params = params_of(scale_log2, clamp_max, 0.8)
    res, pos = long_scatter_case(900, scale_log2)
    film, _, _ = ptss.probe_splat_paths(res, pos, splat_film(), FW, FH, filter=ptss.splat_filter("gaussian", 2.0, 1.0), params=params)
    before = dict(linear=np.full((P, 4), -3.0, np.float32), pixels=np.full((P, 4), 9, np.uint8), history=np.full((P, 4), -2.0, np.float32))
    for mask in range(8):   # each combination of NULL outputs; what is not asked for and what lies outside the range keeps its bytes
        kw = {k: (before[k] if mask & (1 << i) else None) for i, k in enumerate(("linear", "pixels", "history"))}
        c.resolve(("outputs", mask), film, params, **kw)
        linear, pixels, history = c.resolve(("a sub-range", mask), film, params, first_pixel=65, count=257, **kw)
        for out, was in ((linear, before["linear"]), (pixels, before["pixels"]), (history, before["history"])):
            if out is not None:
                rows = np.ascontiguousarray(out).view(was.dtype).reshape(-1, 4)
                assert np.array_equal(rows[:65], was[:65]) and np.array_equal(rows[65 + 257:], was[65 + 257:]) and not np.array_equal(rows[65:322], was[65:322])
    c.resolve("count = 0", film, params, first_pixel=10, count=0)


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement):
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), FW, FH, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", FW, FH, cam, jitter=1)
    params, flt = ptss.linear_params(exposure=1.5), ptss.splat_filter("gaussian", 2.0, 2.0) if placement == "lds" else ptss.splat_filter()
    rng = r.seed_path_rng(P, seed, 0, skip=0)
    film = shadow = splat_film()
    for k in range(4):   # four rounds of generate with positions, trace, homed splat, resolve
        what = (placement, k)
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL if k % 2 else None)
        film = r.splat_paths(res, pos, film, FW, FH, filter=flt, params=params, homed_first_pixel=0)
        shadow, dropped, _ = ptss.probe_splat_paths(res, pos, shadow, FW, FH, filter=flt, params=params, homed_first_pixel=0)   # the device's own results
        assert film.tobytes() == shadow.tobytes() and dropped == 0, what   # (a draw of exactly 1 lands on the closed square's far edge: no stray)
        linear, pixels, history = r.resolve_splat(film, params=params)
        want_linear, want_pixels, want_history = ptss.probe_resolve_splat(shadow, params=params)
        assert same_words(linear, want_linear) and np.array_equal(pixels, want_pixels) and same_words(history, want_history), what
    assert (film["weight"] > 0).all() and float(linear["r"].max()) > 0 and r.splat_stats()[:3] == (0, 4, 4)
    film_cam.jitter = 0
    feat = r.ray_features(r.generate_rays(film_cam, rng)[0])
    dn = ptss.default_denoise_params(levels=2)
    want, _ = ptss.probe_denoise_history(want_history, feat, FW, FH, dn)
    assert np.array_equal(r.denoise_history(history=history, features=feat, levels=2), want)
    r.close()


# ---- 7. no trace in frame state; a second stream; two shards -------------------------------------------------------------------------------------
def test_a_second_stream_and_untouched_frame_state():
    torch = pytest.importorskip("torch")
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    params, flt = ptss.linear_params(exposure=0.7), ptss.splat_filter("tent", 1.5)
    res, pos = long_scatter_case(3000, 4)
    want_film, dropped, clamped = ptss.probe_splat_paths(res, pos, splat_film(), FW, FH, filter=flt, params=params)
    want_linear, want_px, want_hs = ptss.probe_resolve_splat(want_film, params=params)
    hpos, stray = homed_positions(0, P, seed=2)
    want_homed, hdropped, hclamped = ptss.probe_splat_paths(res[:P], hpos, splat_film(), FW, FH, filter=flt, params=params, homed_first_pixel=0)
    side = torch.cuda.Stream()
    d_res = torch.from_numpy(words(res).view(np.float32).copy()).cuda()
    d_pos = torch.from_numpy(words(pos).view(np.float32).copy()).cuda()
    d_hpos = torch.from_numpy(words(hpos).view(np.float32).copy()).cuda()
    r.generate_frame()
    kernels = r.launched_kernels()
    for tick in range(3):
        with torch.cuda.stream(side):
            d_film = torch.zeros((P, 4), dtype=torch.int64, device="cuda")
            d_homed = torch.zeros((P, 4), dtype=torch.int64, device="cuda")
            d_linear = torch.zeros((P, 4), dtype=torch.float32, device="cuda")
            d_px = torch.zeros((P, 4), dtype=torch.uint8, device="cuda")
            d_hs = torch.zeros((P, 4), dtype=torch.float32, device="cuda")
            r.splat_paths(d_res, d_pos, d_film, FW, FH, filter=flt, params=params)
            r.splat_paths(d_res[:P], d_hpos, d_homed, FW, FH, filter=flt, params=params, homed_first_pixel=0)
            r.resolve_splat(d_film, params=params, linear=d_linear, pixels=d_px, history=d_hs)
        side.synchronize()
        assert np.array_equal(d_film.cpu().numpy().view(np.uint64), film_words(want_film)), tick
        assert np.array_equal(d_homed.cpu().numpy().view(np.uint64), film_words(want_homed)), tick
        assert np.array_equal(d_px.cpu().numpy(), want_px) and same_words(d_linear.cpu().numpy(), want_linear) and same_words(d_hs.cpu().numpy(), want_hs), tick
        r.generate_frame()
    assert r.splat_stats() == (3, 3, 3, 3 * (dropped + hdropped), 3 * (clamped + hclamped))
    assert r.launched_kernels() == kernels and r.film_launches() == (0, 0, 0) and r.linear_launches() == (0, 0) and r.film_rejected() == 0
    r.close()


def test_a_sharded_context_answers_as_the_unsharded_one():
    name = "mixed"
    scene = make_scene(name)
    flt = ptss.splat_filter("gaussian", 1.5, 1.0)
    res, pos = long_scatter_case(2000, 6)
    want_film, dropped, clamped = ptss.probe_splat_paths(res, pos, splat_film(), FW, FH, filter=flt)
    hpos, _ = homed_positions(5, P - 9, seed=3)
    want_homed, hdropped, hclamped = ptss.probe_splat_paths(res[:P - 9], hpos, want_film, FW, FH, filter=flt, homed_first_pixel=5)
    want = ptss.probe_resolve_splat(want_homed)
    for rank in (0, 1):   # two shards
        r = ptss.Renderer(scene, 64, 48, max_iterations=4, seed=SCENES[name][3], tile_rank=rank, tile_world=2, band_rows=8)
        film = r.splat_paths(res, pos, splat_film(), FW, FH, filter=flt)   # all of the film, whatever rows the shard owns
        assert film.tobytes() == want_film.tobytes(), rank
        film = r.splat_paths(res[:P - 9], hpos, film, FW, FH, filter=flt, homed_first_pixel=5)
        assert film.tobytes() == want_homed.tobytes(), rank
        linear, px, hs = r.resolve_splat(film)
        assert same_words(linear, want[0]) and np.array_equal(px, want[1]) and same_words(hs, want[2]), rank
        assert r.splat_stats() == (1, 1, 1, dropped + hdropped, clamped + hclamped)
        r.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n = 300
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("s_res", n * 16), ("s_pos", n * 8), ("s_film", P * 32), ("s_lin", P * 16), ("s_pix", P * 4), ("s_hist", P * 16), ("s_rng", n * 24),
             ("s_rays", n * 32), ("s_index", n * 4))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_res, d_pos, d_film, d_lin, d_pix, d_hist, d_rng, d_rays, d_index = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    good, flt = ptss.linear_params(), ptss.splat_filter()
    cam = ptss.film_camera("pinhole", FW, FH, jitter=1)
    ref = lambda s: C.byref(s) if s is not None else None
    sct = lambda ctx, res, pos, count, film, w=FW, h=FH, f=flt, p=good: L.ptss_splat_paths(ctx, res, pos, count, film, w, h, ref(f), ref(p), None)
    hom = lambda ctx, res, pos, first, count, film, w=FW, h=FH, f=flt, p=good: L.ptss_splat_paths_homed(ctx, res, pos, first, count, film, w, h, ref(f), ref(p), None)
    rsv = lambda ctx, film, first, count, lin, pix, hist, p=good: L.ptss_resolve_splat(ctx, film, first, count, ref(p), lin, pix, hist, None)
    gen = lambda ctx, first, index, count, rng, rays, pos, c=cam: L.ptss_generate_rays_positions(ctx, ref(c), first, index, count, rng, rays, pos, None)
    assert gen(r._ctx, 0, None, n, d_rng, d_rays, d_pos) == 0
    assert sct(r._ctx, d_res, d_pos, n, d_film) == 0 and hom(r._ctx, d_res, d_pos, 0, n, d_film) == 0
    assert rsv(r._ctx, d_film, 0, P, d_lin, d_pix, d_hist) == 0
    r.synchronize()
    stats, kernels, film_launches = r.splat_stats(), r.launched_kernels(), r.film_launches()
    assert stats[:3] == (1, 1, 1) and film_launches == (1, 0, 0) and r.film_rejected() == 0

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    both = lambda res, pos, film, **kw: (sct(r._ctx, res, pos, n, film, **kw), hom(r._ctx, res, pos, 0, n, film, **kw))
    assert sct(None, d_res, d_pos, n, d_film) == EINVAL and hom(None, d_res, d_pos, 0, n, d_film) == EINVAL
    assert both(None, d_pos, d_film) == both(d_res, None, d_film) == both(d_res, d_pos, None) == (EINVAL, EINVAL)
    for k in (4, 8, 12):
        assert both(off(d_res, k), d_pos, d_film) == both(d_res, d_pos, off(d_film, k)) == (EINVAL, EINVAL), k
        assert rsv(r._ctx, off(d_film, k), 0, P - 1, d_lin, d_pix, d_hist) == EINVAL, k
        assert rsv(r._ctx, d_film, 0, P, off(d_lin, k), d_pix, d_hist) == EINVAL and rsv(r._ctx, d_film, 0, P, d_lin, d_pix, off(d_hist, k)) == EINVAL, k
        assert gen(r._ctx, 0, None, n, d_rng, off(d_rays, k), d_pos) == EINVAL, k
    for k in (1, 2, 4, 6):
        assert both(d_res, off(d_pos, k), d_film) == (EINVAL, EINVAL), k
        assert gen(r._ctx, 0, None, n, d_rng, d_rays, off(d_pos, k)) == EINVAL, k
    for k in (1, 2, 3):
        assert rsv(r._ctx, d_film, 0, P, d_lin, off(d_pix, k), d_hist) == EINVAL, k
        assert gen(r._ctx, 0, off(d_index, k), n, d_rng, d_rays, d_pos) == EINVAL and gen(r._ctx, 0, None, n, off(d_rng, k), d_rays, d_pos) == EINVAL, k
    assert gen(r._ctx, 0, None, n, d_rng, d_rays, None) == EINVAL and gen(r._ctx, 0, None, 0, None, None, None) == EINVAL   # positions are required
    assert gen(None, 0, None, n, d_rng, d_rays, d_pos) == EINVAL and gen(r._ctx, 0, None, n, None, d_rays, d_pos) == EINVAL
    assert gen(r._ctx, 0, None, n, d_rng, d_rays, d_pos, None) == EINVAL and gen(r._ctx, P - n + 1, None, n, d_rng, d_rays, d_pos) == ERANGE
    # the sizes
    for w, h in ((0, FH), (FW, 0), (-1, FH), (2 ** 22 + 1, 1), (1, 2 ** 22 + 1), (2 ** 22, 2 ** 9), (2 ** 16, 2 ** 15)):
        assert both(d_res, d_pos, d_film, w=w, h=h) == (ERANGE, ERANGE), (w, h)
    assert sct(r._ctx, d_res, d_pos, 2 ** 31, d_film) == ERANGE and hom(r._ctx, d_res, d_pos, 0, 2 ** 31, d_film) == ERANGE
    for first, count in ((P - n + 1, n), (P, 1), (2 ** 63, 2)):
        assert hom(r._ctx, d_res, d_pos, first, count, d_film) == ERANGE, (first, count)
    assert rsv(None, d_film, 0, P, d_lin, d_pix, d_hist) == EINVAL and rsv(r._ctx, None, 0, P, d_lin, d_pix, d_hist) == EINVAL
    for first, count in ((0, 2 ** 31), (2 ** 31, 1), (2 ** 31 - 1, 1), (2 ** 30, 2 ** 30), (2 ** 63, 2 ** 63)):
        assert rsv(r._ctx, d_film, first, count, d_lin, d_pix, d_hist) == ERANGE, (first, count)
    # the filter and the parameters
    assert both(d_res, d_pos, d_film, f=None) == both(d_res, d_pos, d_film, p=None) == (EINVAL, EINVAL)
    assert rsv(r._ctx, d_film, 0, P, d_lin, d_pix, d_hist, None) == EINVAL
    for change in (dict(structSize=16), dict(structSize=0), dict(kind=3), dict(kind=-1), dict(radius=0.49), dict(radius=2.01), dict(radius=float("nan")),
                   dict(reserved=1), dict(kind=2, alpha=0.0), dict(kind=2, alpha=-1.0), dict(kind=2, alpha=float("inf")), dict(kind=2, alpha=float("nan"))):
        bad = ptss.splat_filter()
        for k, v in change.items():
            setattr(bad, k, v)
        assert both(d_res, d_pos, d_film, f=bad) == (EINVAL, EINVAL), change
        assert sct(r._ctx, None, None, 0, None, f=bad) == EINVAL, change   # with n = 0 as well
    for change in (dict(structSize=16), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=float("nan")),
                   dict(scaleLog2=32, clampMax=257.0), dict(exposure=-0.5), dict(exposure=float("inf")), dict(reserved=1)):
        params = ptss.linear_params(clamp_max=2.0 ** 20)
        for k, v in change.items():
            setattr(params, k, v)
        assert both(d_res, d_pos, d_film, p=params) == (EINVAL, EINVAL), change
        assert rsv(r._ctx, d_film, 0, P, d_lin, d_pix, d_hist, params) == EINVAL, change
    assert sct(r._ctx, None, None, 0, None) == 0 and hom(r._ctx, None, None, 0, 0, None) == 0 and rsv(r._ctx, None, 0, 0, None, None, None) == 0
    assert rsv(r._ctx, d_film, 0, P, None, None, None) == 0   # nothing asked for: nothing launched
    out5 = (C.c_ulonglong * 5)()
    assert L.ptss_splat_stats(None, out5) == EINVAL and L.ptss_splat_stats(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.splat_stats() == stats and r.launched_kernels() == kernels and r.film_launches() == film_launches and r.film_rejected() == 0
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 8-byte aligned positions, 16-byte steps, the boundary values
    edge, wide = params_of(32, 256.0, 0.0), ptss.splat_filter("gaussian", 2.0, 1e-3)
    assert sct(r._ctx, off(d_res, 16), off(d_pos, 8), n - 2, off(d_film, 16), w=FW - 1, f=wide, p=edge) == 0
    assert hom(r._ctx, off(d_res, 16), off(d_pos, 8), P - FW - n, n - 2, off(d_film, 16), w=FW, h=FH - 1, f=ptss.splat_filter("box", 0.5), p=edge) == 0
    assert rsv(r._ctx, off(d_film, 16), 0, P - 1, off(d_lin, 16), off(d_pix, 4), None, edge) == 0
    assert gen(r._ctx, 3, off(d_index, 4), n - 2, off(d_rng, 4), off(d_rays, 16), off(d_pos, 8)) == 0
    r.synchronize()
    assert r.splat_stats()[:3] == (2, 2, 2) and r.launched_kernels() == kernels and r.film_launches() == (2, 0, 0)
    r.close()
