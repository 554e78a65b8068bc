"""The linear film on the GPU (ptss_accumulate_paths_linear / ptss_resolve_linear). Every test requires the device to
equal the host probes byte for byte. The context is a 16 x 16 cornell; the film is the siblings' 64 x 48 (a film's size is the caller's, and
an identity map of 257 rays from a first pixel above 0 needs more than 256 pixels).

1. Accumulate: identity maps from a first pixel above 0, a permuted index, sorted indices whose runs cross wave and workgroup edges, one
   pixel for every ray, entries beyond the film inside and between runs, the adversarial rows, runs of 64 and 300 samples at q = 2^40 on a
   film that starts at 2^62 (the carry between the two words of the on-chip sum), a film carried over four calls, permutations and splits.
2. Resolve: each combination of NULL outputs, a sub-range, the rows of the CPU test. 3. The loop generate -> trace -> accumulate -> resolve
   against a shadow loop of the two probes, the history through the denoiser. 4. No trace in frame state, a second stream, a sharded
   context. 5. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from film_common import BATCHES, results_of, words
from linear_common import SCALES, adversarial_results, film_words, high_film, linear_film, params_of, resolve_rows, same_words
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu
P = W * H


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


def runs_index(lengths, g):
    """A sorted index: run k names a pixel of its own lengths[k] times, the pixels increasing."""
    pixels = np.sort(g.choice(P, len(lengths), replace=False))
    return np.repeat(pixels, lengths).astype(np.uint32)


class Checker:
    """Device against probe for one context, keeping the two counters the calls move."""

    def __init__(self, r):
        self.r, self.rejected, self.launches = r, r.film_rejected(), r.linear_launches()

    def accumulate(self, what, rows, start, params, **kw):
        film = self.r.accumulate_paths_linear(rows, start, params=params, **kw)
        want, dropped = ptss.probe_accumulate_linear(rows, start, params=params, **kw)
        assert film.tobytes() == want.tobytes(), what
        self.rejected += dropped
        self.launches = (self.launches[0] + (1 if len(rows) else 0), self.launches[1])
        assert self.r.film_rejected() == self.rejected and self.r.linear_launches() == self.launches, what
        return film

    def resolve(self, what, film, params, **kw):
        got = self.r.resolve_linear(film, params=params, **kw)
        want = ptss.probe_resolve_linear(film, params=params, **kw)
        for a, b in zip(got, want):
            assert (a is None) == (b is None), what
            assert a is None or (np.array_equal(a, b) if a.dtype == np.uint8 else same_words(a, b)), what
        launched = any(kw.get(k, True) is not None for k in ("linear", "pixels", "history")) and len(film) > 0 and kw.get("count", 1) != 0
        self.launches = (self.launches[0], self.launches[1] + (1 if launched else 0))
        assert self.r.linear_launches() == self.launches, what
        return got


# ---- 1. accumulate ------------------------------------------------------------------------------------------------------------------------------
def test_accumulate_equals_the_probe(small):
    c, g = Checker(small), np.random.default_rng(9)
    params = ptss.linear_params()
    rad = adversarial_results(params)
    more = np.concatenate([rad["radiance"], (g.uniform(0, 1.4, (P - len(rad), 3)) ** 6 * 30).astype(np.float32)])   # one row per film pixel
    res = results_of(more)
    start = linear_film(P)   # a film that has been in use
    start["r"], start["g"], start["b"] = g.integers(0, 2 ** 50, P), g.integers(0, 2 ** 33, P), 7
    start["samples"], start["clamped"] = 40, g.integers(0, 3, P)

    film = c.accumulate("identity map", res, start, params)
    assert (film["samples"] == 41).all()
    for n in BATCHES:   # 1, 63, 64, 65, 257 rays from a first pixel > 0: the rest stays untouched
        film = c.accumulate(("first pixel 1000", n), res[:n], start, params, first_pixel=1000)
        rest = np.ones(P, bool)
        rest[1000:1000 + n] = False
        assert film[rest].tobytes() == start[rest].tobytes() and (film["samples"][~rest] == 41).all(), n
    c.accumulate("permuted index", res, start, params, index=g.permutation(P).astype(np.uint32))
    for k, lengths in enumerate(([1, 2, 63, 64, 65, 300, 1, 1, 65, 64, 63, 2, 300, 64, 64, 1, 300], [300, 300, 65, 1, 63, 63, 2, 64, 1, 1, 1, 65, 300],
                                 [64] * 12 + [1] * 70 + [2] * 40, [3] * 600)):
        index = runs_index(lengths, g)
        film = c.accumulate(("sorted runs", k), res[:len(index)], start, params, index=index)
        assert film["samples"].sum() == 40 * P + len(index)
        wild = index.copy()   # entries beyond the film inside runs and between them
        inside = g.choice(len(wild), 40, replace=False)
        wild[inside] = g.choice([P, P + 1, 2 ** 31, 2 ** 32 - 1], 40)
        edges = np.flatnonzero(np.diff(index) != 0)[::3]
        wild[edges] = P + 7
        rejected = c.rejected
        c.accumulate(("sorted runs with entries beyond the film", k), res[:len(wild)], start, params, index=wild)
        assert c.rejected == rejected + int((wild >= P).sum()) > rejected
    film = c.accumulate("every ray on one pixel", res, start, params, index=np.full(P, 1234, np.uint32))
    assert film["samples"][1234] == 40 + P and film["samples"].sum() == 41 * P
    c.accumulate("many to few", res, start, params, index=(g.integers(0, 40, P) * 77).astype(np.uint32))   # duplicates that are not neighbours
    c.accumulate("nothing inside the film", res[:300], start, params, index=np.full(300, P, np.uint32))
    film = want = start   # a film carried over four calls, with and without an index
    for k in range(4):
        index = None if k % 2 == 0 else np.sort(g.integers(0, P, P)).astype(np.uint32)
        rows = res[g.permutation(P)]
        film = small.accumulate_paths_linear(rows, film, index=index, params=params)
        want, _ = ptss.probe_accumulate_linear(rows, want, index=index, params=params)
        assert film.tobytes() == want.tobytes(), k
    assert film["samples"].sum() == 44 * P


@pytest.mark.parametrize("scale_log2, clamp_max", SCALES[:3])
def test_adversarial_rows_and_the_carry_at_every_scale(small, scale_log2, clamp_max):
    c, g = Checker(small), np.random.default_rng(scale_log2)
    params = params_of(scale_log2, clamp_max)
    res = adversarial_results(params)
    M = len(res)
    film = c.accumulate("identity", res, linear_film(P), params, first_pixel=5)
    assert 0 < film["clamped"].sum() < M
    c.accumulate("sorted with duplicates", res, linear_film(P), params, index=np.sort(g.integers(0, 60, M)).astype(np.uint32))
    c.accumulate("one pixel", res, high_film(P), params, index=np.full(M, 77, np.uint32))
    # runs of 64 and of 300 samples, all at q = 2^40, on a film that starts at 2^62: aligned to a wave, across waves, across a workgroup
    top = results_of(np.full((1000, 3), clamp_max, np.float32))
    for lengths in ([64, 300, 64], [1, 64, 300], [63, 300, 64, 64], [200, 64, 300]):
        index = runs_index(lengths, g)
        film = c.accumulate(("2^40 per sample", lengths), top[:len(index)], high_film(P), params, index=index)
        for p, n in zip(np.unique(index), lengths):
            assert int(film["r"][p]) == int(film["g"][p]) == int(film["b"][p]) == (1 << 62) + (n << 40) and film["samples"][p] == 5 + n, (lengths, p)
    film = c.accumulate("2^40 per sample, identity", top, high_film(P), params, first_pixel=1)
    assert int(film["b"][1000]) == (1 << 62) + (1 << 40) and int(film["b"][1001]) == 1 << 62


@pytest.mark.parametrize("seed", range(3))
def test_a_batch_permuted_and_split_gives_the_same_bytes(small, seed):
    g = np.random.default_rng(40 + seed)
    params = params_of(*SCALES[seed])
    res = adversarial_results(params, seed=seed)
    res = np.concatenate([res, res[::-1], res])[:1500]
    n = len(res)
    index = np.sort(g.integers(0, 90, n)).astype(np.uint32) if seed else g.integers(0, P + 2, n).astype(np.uint32)
    start = high_film(P) if seed == 1 else linear_film(P)
    whole = small.accumulate_paths_linear(res, start, index=index, params=params)
    assert whole.tobytes() == ptss.probe_accumulate_linear(res, start, index=index, params=params)[0].tobytes()
    for _ in range(2):
        order = g.permutation(n)
        assert small.accumulate_paths_linear(res[order], start, index=index[order], params=params).tobytes() == whole.tobytes()
        cut = int(g.integers(1, n))
        first = small.accumulate_paths_linear(res[order][:cut], start, index=index[order][:cut], params=params)
        assert small.accumulate_paths_linear(res[order][cut:], first, index=index[order][cut:], params=params).tobytes() == whole.tobytes()


# ---- 2. resolve ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_log2, clamp_max", SCALES)
def test_resolve_equals_the_probe(small, scale_log2, clamp_max):
    c = Checker(small)
    for exposure in (0.0, 1.0, 0.37, 40.0):
        params = params_of(scale_log2, clamp_max, exposure)
        c.resolve(("the rows of the CPU test", exposure), resolve_rows(params), params)
    params = params_of(scale_log2, clamp_max, 0.8)
    g = np.random.default_rng(scale_log2 + 1)
    rows = adversarial_results(params)
    film, _ = ptss.probe_accumulate_linear(rows, linear_film(700), index=g.integers(0, 700, len(rows)).astype(np.uint32), params=params)
    before = dict(linear=np.full((700, 4), -3.0, np.float32), pixels=np.full((700, 4), 9, np.uint8), history=np.full((700, 4), -2.0, np.float32))
    for mask in range(8):   # each combination of NULL outputs; what is not asked for and what lies outside the range keeps its bytes
        kw = {k: (before[k] if mask & (1 << i) else None) for i, k in enumerate(("linear", "pixels", "history"))}
        c.resolve(("outputs", mask), film, params, **kw)
        linear, pixels, history = c.resolve(("a sub-range", mask), film, params, first_pixel=65, count=257, **kw)
        for out, was in ((linear, before["linear"]), (pixels, before["pixels"]), (history, before["history"])):
            if out is not None:
                rows = np.ascontiguousarray(out).view(was.dtype).reshape(-1, 4)
                assert np.array_equal(rows[:65], was[:65]) and np.array_equal(rows[65 + 257:], was[65 + 257:]) and not np.array_equal(rows[65:322], was[65:322])
    c.resolve("count = 0", film, params, first_pixel=10, count=0)


def test_an_exposure_on_a_threshold_of_the_contexts_table(small):
    """mean = 1 exactly, exposure = a threshold and its neighbours: the device's table form against the probe's literal tone map."""
    c = Checker(small)
    Tq = np.empty(257, dtype=np.float32)
    assert ptss.host_lib().ptss_probe_quant_table(Tq.ctypes.data_as(C.POINTER(C.c_float))) == 0
    film = linear_film(3)
    film["r"], film["g"], film["b"], film["samples"] = 1 << 20, 3 << 20, 1 << 20, (1, 3, 1)
    for k in (1, 2, 18, 128, 201, 255):
        for x, byte in ((np.nextafter(Tq[k], np.float32(-1)), k - 1), (Tq[k], k), (np.nextafter(Tq[k], np.float32(2)), k)):
            _, pixels, _ = c.resolve((k, float(x)), film, ptss.linear_params(exposure=float(x)))
            assert pixels[0, 0] == pixels[1, 1] == pixels[2, 2] == byte, (k, float(x))


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement):
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params = ptss.linear_params(exposure=1.5)
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = linear_film(N)
    for k in range(4):   # four rounds of generate, trace, linear accumulate, resolve
        what = (placement, k)
        rays, rng = r.generate_rays(film_cam, rng)
        res, rng = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL if k % 2 else None)
        film = r.accumulate_paths_linear(res, film, params=params)
        shadow, dropped = ptss.probe_accumulate_linear(res, shadow, params=params)   # the probe fed the device's own trace results
        assert film.tobytes() == shadow.tobytes() and dropped == 0, what
        linear, pixels, history = r.resolve_linear(film, params=params)
        want_linear, want_pixels, want_history = ptss.probe_resolve_linear(shadow, params=params)
        assert same_words(linear, want_linear) and np.array_equal(pixels, want_pixels) and same_words(history, want_history), what
    assert (film["samples"] == 4).all() and float(linear["r"].max()) > 0 and r.linear_launches() == (4, 4)
    film_cam.jitter = 0
    feat = r.ray_features(r.generate_rays(film_cam, rng)[0])
    dn = ptss.default_denoise_params(levels=2)
    want, _ = ptss.probe_denoise_history(want_history, feat, W, H, dn)
    assert np.array_equal(r.denoise_history(history=history, features=feat, levels=2), want)
    r.close()


# ---- 4. no trace in frame state; a second stream; a sharded context --------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    Pf, n = 80 * 30, 3000
    g = np.random.default_rng(1)
    res = results_of((g.uniform(0, 1.3, (n, 3)) ** 5 * 20).astype(np.float32))
    index = np.sort(g.integers(0, Pf, n)).astype(np.uint32)
    params = ptss.linear_params(exposure=0.7)
    want_film, _ = ptss.probe_accumulate_linear(res, linear_film(Pf), index=index, params=params)
    want_linear, want_px, want_hs = ptss.probe_resolve_linear(want_film, params=params)
    side = torch.cuda.Stream()
    d_res = torch.from_numpy(words(res).view(np.float32).copy()).cuda()
    d_index = torch.from_numpy(index.view(np.int32).copy()).cuda()
    for tick in range(20):   # twenty frames with the two calls after each
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        film = r.accumulate_paths_linear(res, linear_film(Pf), index=index, params=params)   # on the context's stream
        linear, px, hs = r.resolve_linear(film, params=params)
        assert film.tobytes() == want_film.tobytes() and same_words(linear, want_linear) and np.array_equal(px, want_px) and same_words(hs, want_hs), tick
        with torch.cuda.stream(side):   # and on a second one
            d_film = torch.zeros((Pf, 4), dtype=torch.int64, device="cuda")
            d_linear = torch.zeros((Pf, 4), dtype=torch.float32, device="cuda")
            d_px = torch.zeros((Pf, 4), dtype=torch.uint8, device="cuda")
            d_hs = torch.zeros((Pf, 4), dtype=torch.float32, device="cuda")
            r.accumulate_paths_linear(d_res, d_film, index=d_index, params=params)
            r.resolve_linear(d_film, params=params, linear=d_linear, pixels=d_px, history=d_hs)
        side.synchronize()
        assert np.array_equal(d_film.cpu().numpy().view(np.uint64), film_words(want_film)) and np.array_equal(d_px.cpu().numpy(), want_px), tick
        assert same_words(d_linear.cpu().numpy(), want_linear) and same_words(d_hs.cpu().numpy(), want_hs), tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "twenty frames with the two linear calls after each", W, H, 1)
    assert r.linear_launches() == (40, 40) and r.film_launches() == (0, 0, 0) and r.adaptive_launches() == (0, 0) and r.film_rejected() == 0
    o.close()
    r.close()


def test_a_sharded_context_answers_as_the_unsharded_one():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    g = np.random.default_rng(5)
    res = results_of((g.uniform(0, 1.3, (N, 3)) ** 5 * 20).astype(np.float32))
    index = np.sort(g.integers(0, N, N)).astype(np.uint32)
    want_film, _ = ptss.probe_accumulate_linear(res, linear_film(N), index=index)
    want = ptss.probe_resolve_linear(want_film)
    for rank in (0, 1):   # two shards
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8)
        film = r.accumulate_paths_linear(res, linear_film(N), index=index)   # all of the film, whatever rows the shard owns
        assert film.tobytes() == want_film.tobytes(), rank
        linear, px, hs = r.resolve_linear(film)
        assert same_words(linear, want[0]) and np.array_equal(px, want[1]) and same_words(hs, want[2]), rank
        assert r.linear_launches() == (1, 1)
        r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n, Pf = 300, 20 * 15
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("l_res", n * 16), ("l_film", Pf * 32), ("l_lin", Pf * 16), ("l_pix", Pf * 4), ("l_hist", Pf * 16), ("l_index", n * 4))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_res, d_film, d_lin, d_pix, d_hist, d_index = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    good = ptss.linear_params()
    ref = lambda params: C.byref(params) if params is not None else None
    acc = lambda ctx, res, index, first, count, film, pixels, params=good: L.ptss_accumulate_paths_linear(ctx, res, index, first, count, film, pixels, ref(params), None)
    rsv = lambda ctx, film, first, count, lin, pix, hist, params=good: L.ptss_resolve_linear(ctx, film, first, count, ref(params), lin, pix, hist, None)
    assert acc(r._ctx, d_res, None, 0, n, d_film, Pf) == 0
    assert rsv(r._ctx, d_film, 0, Pf, d_lin, d_pix, d_hist) == 0
    r.synchronize()
    counters, kernels = r.linear_launches(), r.launched_kernels()
    assert counters == (1, 1) and r.film_rejected() == 0 and r.film_launches() == (0, 0, 0)

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    # ptss_accumulate_paths_linear: ptss_accumulate_paths' refusals
    assert acc(None, d_res, None, 0, n, d_film, Pf) == EINVAL
    assert acc(r._ctx, None, None, 0, n, d_film, Pf) == EINVAL and acc(r._ctx, d_res, None, 0, n, None, Pf) == EINVAL
    for k in (4, 8, 12):
        assert acc(r._ctx, off(d_res, k), None, 0, n, d_film, Pf) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, off(d_film, k), Pf) == EINVAL, k
        assert rsv(r._ctx, off(d_film, k), 0, Pf - 1, d_lin, d_pix, d_hist) == EINVAL, k
        assert rsv(r._ctx, d_film, 0, Pf, off(d_lin, k), d_pix, d_hist) == EINVAL, k
        assert rsv(r._ctx, d_film, 0, Pf, d_lin, d_pix, off(d_hist, k)) == EINVAL, k
    for k in (1, 2, 3):
        assert acc(r._ctx, d_res, off(d_index, k), 0, n, d_film, Pf) == EINVAL, k
        assert rsv(r._ctx, d_film, 0, Pf, d_lin, off(d_pix, k), d_hist) == EINVAL, k
    assert acc(r._ctx, d_res, d_index, 0, 2 ** 31, d_film, Pf) == ERANGE
    assert acc(r._ctx, d_res, d_index, 0, n, d_film, 2 ** 31) == ERANGE
    for first, count, pixels in ((1, n, n), (Pf - n + 1, n, Pf), (Pf, 1, Pf), (0, n, n - 1), (2 ** 63, 2, Pf)):
        assert acc(r._ctx, d_res, None, first, count, d_film, pixels) == ERANGE, (first, count, pixels)
    # ptss_resolve_linear
    assert rsv(None, d_film, 0, Pf, d_lin, d_pix, d_hist) == EINVAL and rsv(r._ctx, None, 0, Pf, d_lin, d_pix, d_hist) == EINVAL
    for first, count in ((0, 2 ** 31), (2 ** 31, 1), (2 ** 31 - 1, 1), (2 ** 30, 2 ** 30), (2 ** 63, 2 ** 63)):
        assert rsv(r._ctx, d_film, first, count, d_lin, d_pix, d_hist) == ERANGE, (first, count)
    # the parameters, for both
    assert acc(r._ctx, d_res, None, 0, n, d_film, Pf, None) == EINVAL and rsv(r._ctx, d_film, 0, Pf, d_lin, d_pix, d_hist, None) == EINVAL
    for change in (dict(structSize=16), dict(structSize=0), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=-1.0),
                   dict(clampMax=float("inf")), dict(clampMax=float("nan")), dict(clampMax=float(np.nextafter(np.float32(2.0 ** 20), np.float32(np.inf)))),
                   dict(scaleLog2=32, clampMax=257.0), dict(scaleLog2=0, clampMax=2.0 ** 41), dict(exposure=-0.5), dict(exposure=float("inf")),
                   dict(exposure=float("nan")), dict(reserved=1)):
        params = ptss.linear_params(clamp_max=2.0 ** 20)
        for k, v in change.items():
            setattr(params, k, v)
        assert acc(r._ctx, d_res, None, 0, n, d_film, Pf, params) == EINVAL, change
        assert rsv(r._ctx, d_film, 0, Pf, d_lin, d_pix, d_hist, params) == EINVAL, change
    assert acc(r._ctx, None, None, 0, 0, None, Pf) == 0 and rsv(r._ctx, None, 0, 0, None, None, None) == 0   # n = 0, count = 0
    assert rsv(r._ctx, d_film, 0, Pf, None, None, None) == 0   # nothing asked for: nothing launched
    out2 = (C.c_ulonglong * 2)()
    assert L.ptss_linear_launches(None, out2) == EINVAL and L.ptss_linear_launches(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.linear_launches() == counters and r.launched_kernels() == kernels and r.film_rejected() == 0
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: a 4-byte aligned index and pixels, 16-byte steps, the boundary parameters
    edge = params_of(32, 256.0, 0.0)
    assert acc(r._ctx, off(d_res, 16), off(d_index, 4), 0, n - 2, off(d_film, 16), Pf - 1, edge) == 0
    assert rsv(r._ctx, off(d_film, 16), 0, Pf - 1, off(d_lin, 16), off(d_pix, 4), None, edge) == 0
    r.synchronize()
    assert r.linear_launches() == (2, 2) and r.launched_kernels() == kernels and r.film_rejected() == 0
    r.close()
