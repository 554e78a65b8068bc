"""Adaptive sampling on the linear film on the GPU (ptss_accumulate_paths_linear_stats / ptss_plan_samples_linear). Every
test requires the device to equal the host probes byte for byte.

1. The accumulate against the probe (moments) and against ptss_accumulate_paths_linear (film): identity maps, a permuted index, sorted
   indices whose runs cross wave and workgroup edges, one pixel for every ray, entries beyond the film inside and between runs, the
   adversarial rows at three scales, runs whose on-chip sums carry between their 32-bit words, a NULL film, a batch permuted and split.
2. The plan's cdf, index and info against the probe: films below, at and beyond the scan's tiles and beyond one pass of the tile sums,
   budgets around a wave, every kind of content. 3. The loop generate -> trace -> accumulate -> plan -> resolve against a shadow loop of
   the probes, on the linear film and beside the filtered one. 4. No trace in frame state, a second stream, two shards. 5. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from adaptive_common import SCAN_TILE
from film_common import BATCHES, results_of, words
from linear_common import SCALES, adversarial_results, film_words, high_film, linear_film, params_of, same_words
from linstats_common import (check_plan, consistent_moments, conversion_rows, high_moments, moment_words, moments_of_rows, random_word_moments,
                             row_of_ys, zero_moments)
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu
P = W * H   # 64 x 48: one and a half scan tiles


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


class Checker:
    """Device against probe and against ptss_accumulate_paths_linear for one context, keeping the counters."""

    def __init__(self, r):
        self.r, self.rejected, self.launches, self.linear = r, r.film_rejected(), r.linear_stats_launches()[0], r.linear_launches()[0]

    def accumulate(self, what, res, film, moments, params, **kw):
        r = self.r
        f, m = r.accumulate_paths_linear_stats(res, film, moments, params=params, **kw)
        want_f, want_m, dropped = ptss.probe_accumulate_linear_stats(res, film, moments, params=params, **kw)
        assert moment_words(m).tobytes() == moment_words(want_m).tobytes(), what
        assert film_words(f).tobytes() == film_words(want_f).tobytes(), what
        plain = r.accumulate_paths_linear(res, film, params=params, **kw)   # the film's bytes are the plain call's
        assert film_words(f).tobytes() == film_words(plain).tobytes(), what
        none, m2 = r.accumulate_paths_linear_stats(res, None, moments, params=params, **kw)   # a NULL film: moments only, the same
        assert none is None and moment_words(m2).tobytes() == moment_words(want_m).tobytes(), what
        self.rejected += 3 * dropped   # the three device calls count what they drop
        self.launches += 2 if len(res) else 0
        self.linear += 1 if len(res) else 0
        assert r.film_rejected() == self.rejected and r.linear_stats_launches()[0] == self.launches and r.linear_launches()[0] == self.linear, what
        return f, m, dropped


def runs_index(lengths, pixels, g):
    """A sorted index: run k names a pixel of its own lengths[k] times, the pixels increasing."""
    chosen = np.sort(g.choice(pixels, len(lengths), replace=False))
    return np.repeat(chosen, lengths).astype(np.uint32)


RUNS = ([1, 2, 63, 64, 65, 300, 1, 1, 65, 64, 63, 2, 300, 64, 64, 1, 300], [300, 300, 65, 1, 63, 63, 2, 64, 1, 1, 1, 65, 300], [64] * 12 + [1] * 70 + [2] * 40)


# ---- 1. the accumulate ---------------------------------------------------------------------------------------------------------------------------
def test_accumulate_equals_the_probe_and_the_linear_film(small):
    c, g = Checker(small), np.random.default_rng(9)
    params = ptss.linear_params()
    res = results_of((g.uniform(0, 1.3, (P, 3)) ** 4 * 50).astype(np.float32))
    film, moments = high_film(P), high_moments(P)
    for n in BATCHES:   # identity maps from a first pixel above 0: the rest stays untouched
        f, m, _ = c.accumulate(("first pixel 1000", n), res[:n], film, moments, params, first_pixel=1000)
        rest = np.ones(P, bool)
        rest[1000:1000 + n] = False
        assert (m["samples"][rest] == 5).all() and (m["samples"][~rest] == 6).all() and (f["samples"][~rest] == 6).all()
        assert moment_words(m)[rest].tobytes() == moment_words(moments)[rest].tobytes() and film_words(f)[rest].tobytes() == film_words(film)[rest].tobytes()
    c.accumulate("the whole film", res, film, moments, params)
    c.accumulate("permuted index", res, film, moments, params, index=g.permutation(P).astype(np.uint32))
    for k, lengths in enumerate(RUNS):   # runs that start anywhere in a wave and cross wave and workgroup edges
        index = runs_index(lengths, P, g)
        _, m, _ = c.accumulate(("sorted runs", k), res[:len(index)], film, moments, params, index=index)
        assert int(m["samples"].sum()) == 5 * P + len(index)
        wild = index.copy()   # entries beyond the film inside runs and between them
        inside = g.choice(len(wild), 40, replace=False)
        wild[inside] = g.choice([P, P + 1, 2 ** 31, 2 ** 32 - 1], 40)
        wild[np.flatnonzero(np.diff(index) != 0)[::3]] = P + 7
        _, m, dropped = c.accumulate(("sorted runs with entries beyond the film", k), res[:len(wild)], film, moments, params, index=wild)
        assert dropped >= 40 and int(m["samples"].sum()) == 5 * P + len(wild) - dropped
    _, m, _ = c.accumulate("every ray on one pixel", res, film, moments, params, index=np.full(P, 1234, np.uint32))
    assert int(m["samples"][1234]) == 5 + P
    c.accumulate("many to few", res, film, moments, params, index=g.integers(0, 40, P).astype(np.uint32) * 77)   # duplicates that are not neighbours
    c.accumulate("nothing inside the film", res[:300], film, moments, params, index=np.full(300, P, np.uint32))
    c.accumulate("nothing at all", res[:0], film, moments, params)


@pytest.mark.parametrize("scale_log2,clamp_max", SCALES[:3])
def test_accumulate_of_the_adversarial_rows(small, scale_log2, clamp_max):
    c, g = Checker(small), np.random.default_rng(scale_log2)
    params = params_of(scale_log2, clamp_max)
    res = adversarial_results(params)
    n = len(res)
    c.accumulate("identity", res, linear_film(n + 9), zero_moments(n + 9), params, first_pixel=4)
    c.accumulate("permuted", res, high_film(n), high_moments(n), params, index=g.permutation(n).astype(np.uint32))
    c.accumulate("sorted, many to few", res, high_film(41), high_moments(41), params, index=np.sort(g.integers(0, 41, n)).astype(np.uint32))


def test_on_chip_sums_carry_between_their_words(small):
    """Runs of 64 and 300 samples with y = 2^40 (sqHi at its maximum) and with a y whose sqLo is at least 2^39, on words that start at
    2^62: every on-chip sum passes 2^32 inside a wave."""
    c = Checker(small)
    params = params_of(0, 2.0 ** 40)   # scaleLog2 0: a radiance is its own fixed-point value
    y_low = 741456           # the first integer whose square reaches 2^39 (and stays below 2^40): sqHi = 0, sqLo >= 2^39
    assert (y_low * y_low) >> 40 == 0 and y_low * y_low >= 1 << 39
    for what, y in (("y = 2^40", float(1 << 40)), ("sqLo >= 2^39", float(y_low))):
        rows = results_of(np.full((364, 3), y, np.float32))   # grey: the luminance is the channel
        index = np.repeat(np.array([7, 2000], np.uint32), [64, 300])
        f, m, _ = c.accumulate(what, rows, high_film(P), high_moments(P), params, index=index)
        yi = int(y)
        for p, k in ((7, 64), (2000, 300)):
            assert [int(v) for v in moment_words(m)[p]] == [(1 << 62) + k * yi, (1 << 62) + k * ((yi * yi) & ((1 << 40) - 1)), (1 << 62) + k * ((yi * yi) >> 40), 5 + k]
            assert int(f["r"][p]) == (1 << 62) + k * yi
        c.accumulate((what, "identity"), rows[:300], high_film(P), high_moments(P), params, first_pixel=100)


@pytest.mark.parametrize("seed", range(2))
def test_a_batch_permuted_and_split_gives_the_same_bytes(small, seed):
    r, g = small, np.random.default_rng(70 + seed)
    params = params_of(*SCALES[1 + seed])
    res = adversarial_results(params, seed=seed)
    n = len(res)
    index = np.sort(g.integers(0, P + 3, n)).astype(np.uint32) if seed else g.integers(0, P + 3, n).astype(np.uint32)
    f0, m0 = r.accumulate_paths_linear_stats(res, high_film(P), high_moments(P), index=index, params=params)
    want_f, want_m, _ = ptss.probe_accumulate_linear_stats(res, high_film(P), high_moments(P), index=index, params=params)
    assert film_words(f0).tobytes() == film_words(want_f).tobytes() and moment_words(m0).tobytes() == moment_words(want_m).tobytes()
    order = g.permutation(n)
    f1, m1 = r.accumulate_paths_linear_stats(res[order], high_film(P), high_moments(P), index=index[order], params=params)
    cut = int(g.integers(1, n))
    fa, ma = r.accumulate_paths_linear_stats(res[order][:cut], high_film(P), high_moments(P), index=index[order][:cut], params=params)
    f2, m2 = r.accumulate_paths_linear_stats(res[order][cut:], fa, ma, index=index[order][cut:], params=params)
    for f, m in ((f1, m1), (f2, m2)):
        assert film_words(f).tobytes() == film_words(f0).tobytes() and moment_words(m).tobytes() == moment_words(m0).tobytes()


# ---- 2. the plan -------------------------------------------------------------------------------------------------------------------------------
PLAN = dict(min_samples=4, max_samples=40, threshold=0.05)
FILM_PIXELS = (1, 15, SCAN_TILE + 1, 64 * 48, 2 * SCAN_TILE + 1)   # 1, 15, 2,049, 3,072 and 4,097


def plan_films(pixels):
    """name -> moments of `pixels` pixels: every kind of content the plan meets."""
    g = np.random.default_rng(pixels)
    flat = consistent_moments(np.full(pixels, 10), g, spread=0.0)    # every pixel converged
    noisy = consistent_moments(g.integers(0, 48, pixels), g)          # unsampled, live, converged and capped pixels mixed
    out = {"all zero": zero_moments(pixels), "all converged": flat, "mixed": noisy, "random words": random_word_moments(pixels, g)}
    live = row_of_ys([0, 1 << 30] * 5)
    for where, p in (("first", 0), ("last", pixels - 1), ("before a tile edge", SCAN_TILE - 1), ("at a tile edge", SCAN_TILE), ("at the second tile edge", 2 * SCAN_TILE)):
        if p < pixels and (where in ("first", "last") or pixels > SCAN_TILE):
            m = flat.copy()
            moment_words(m)[p] = live
            out["one live pixel " + where] = m
    full = noisy.copy()
    full["samples"][::2] = 40   # pixels at maxSamples between live ones
    full["samples"][1::5] = 39
    out["pixels at maxSamples"] = full
    rows = [row for _, row in conversion_rows()]   # D on both conversion paths, over and over
    out["both conversion paths"] = moments_of_rows([rows[k % len(rows)] for k in range(pixels)])
    return out


@pytest.mark.parametrize("pixels", FILM_PIXELS)
def test_plan_equals_the_host_probe(small, pixels):
    r, params = small, ptss.linear_params()
    launches, other = r.linear_stats_launches()[1], (r.adaptive_launches(), r.linear_launches())
    seen_uniform = seen_live = 0
    for name, moments in plan_films(pixels).items():
        plan = ptss.linear_plan_params(**dict(PLAN, max_samples=1 << 23)) if name == "both conversion paths" else ptss.linear_plan_params(**PLAN)
        for n in (1, 63, 64, 65, 257, 4 * pixels):
            cdf, index, info = r.plan_samples_linear(moments, n, params, plan)
            want_cdf, want_index, want_info = ptss.probe_plan_samples_linear(moments, n, params, plan)
            assert np.array_equal(cdf, want_cdf), (name, n)
            assert np.array_equal(index, want_index), (name, n)
            assert info == want_info, (name, n, info, want_info)
            launches += 1
        seen_uniform += info["uniform"]
        seen_live += info["activePixels"] > 0
        if name == "all zero":
            assert info["unsampledPixels"] == pixels and info["totalWeight"] == pixels << 19
        if name == "all converged":
            assert info["uniform"] == 1 and info["activePixels"] == 0
        if name.startswith("one live pixel"):
            assert info["activePixels"] == 1 and len(np.unique(index)) == 1
        if name == "pixels at maxSamples":
            assert info["cappedPixels"] >= 2 * pixels // 5
        if pixels <= 64 * 48 and name in ("mixed", "random words", "pixels at maxSamples", "both conversion paths"):
            check_plan(moments, 4 * pixels, params, plan, cdf, index, info)   # (the last budget) the model's weights and the three properties
    assert seen_uniform >= 1 and seen_live >= 3
    assert r.linear_stats_launches()[1] == launches and (r.adaptive_launches(), r.linear_launches()) == other


def test_plan_of_a_film_beyond_one_pass_of_the_tile_sums(small):
    """The one workgroup that scans the tile sums takes 1,024 tiles per pass and carries the sum over: a film of 1,024 tiles and a pixel
    under the new reduce."""
    r, params, plan = small, ptss.linear_params(), ptss.linear_plan_params(**PLAN)
    pixels = 1024 * SCAN_TILE + 1
    g = np.random.default_rng(7)
    lone = zero_moments(pixels)   # every pixel capped but the last, the second pass's only one
    lone["samples"] = 40
    lone["samples"][pixels - 1] = 0
    for what, m in (("random words", random_word_moments(pixels, g)), ("only the last pixel", lone)):
        for n in (257, 100001):
            cdf, index, info = r.plan_samples_linear(m, n, params, plan)
            want_cdf, want_index, want_info = ptss.probe_plan_samples_linear(m, n, params, plan)
            assert np.array_equal(cdf, want_cdf) and np.array_equal(index, want_index) and info == want_info, (what, n, info, want_info)
    assert info == dict(totalWeight=1 << 19, activePixels=1, unsampledPixels=1, cappedPixels=pixels - 1, uniform=0) and (index == pixels - 1).all()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement):
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params, plan = ptss.linear_params(exposure=1.5), ptss.linear_plan_params(min_samples=4, max_samples=64, threshold=0.05)
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = linear_film(N)
    moments = shadow_m = zero_moments(N)
    index = None
    rejected0 = r.film_rejected()
    for k in range(8):   # four uniform rounds, then four planned rounds of 3,072 rays
        what = (placement, k)
        rays, rng = r.generate_rays(film_cam, rng, index=index)   # ray slot i keeps stream i whatever pixel it is given
        res, rng = r.trace_paths(rays, rng, iterations)
        film, moments = r.accumulate_paths_linear_stats(res, film, moments, index=index, params=params)
        shadow, shadow_m, dropped = ptss.probe_accumulate_linear_stats(res, shadow, shadow_m, index=index, params=params)   # the device's own results
        assert film_words(film).tobytes() == film_words(shadow).tobytes() and moment_words(moments).tobytes() == moment_words(shadow_m).tobytes(), what
        assert dropped == 0 and int(moments["samples"].sum()) == (k + 1) * N and np.array_equal(moments["samples"], film["samples"]), what
        if k >= 3:
            cdf, index, info = r.plan_samples_linear(moments, N, params, plan)
            want_cdf, want_index, want_info = ptss.probe_plan_samples_linear(shadow_m, N, params, plan)
            assert np.array_equal(cdf, want_cdf) and np.array_equal(index, want_index) and info == want_info, what
            assert info["unsampledPixels"] == 0 and 0 < info["activePixels"] < N and info["uniform"] == 0, (what, info)
    assert film["samples"].min() >= 4 and film["samples"].max() > 8   # the planned rays went to some pixels and not to others
    linear, pixels, history = r.resolve_linear(film, params=params)
    want_linear, want_pixels, want_history = ptss.probe_resolve_linear(shadow, params=params)
    assert same_words(linear, want_linear) and np.array_equal(pixels, want_pixels) and same_words(history, want_history)
    assert r.film_rejected() == rejected0 and r.linear_stats_launches() == (8, 5) and r.linear_launches() == (0, 1) and r.adaptive_launches() == (0, 0)
    r.close()


def test_the_loop_beside_a_filtered_film():
    """Moments by index pixel, accumulated with a NULL film beside ptss_splat_paths' scatter form."""
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params, plan, flt = ptss.linear_params(), ptss.linear_plan_params(min_samples=4, max_samples=64, threshold=0.05), ptss.splat_filter()
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = np.zeros(N, dtype=ptss.SPLAT_DTYPE)
    moments = shadow_m = zero_moments(N)
    index = None
    for k in range(8):
        rays, rng, pos = r.generate_rays(film_cam, rng, index=index, positions=True)
        res, rng = r.trace_paths(rays, rng, iterations)
        film = r.splat_paths(res, pos, film, W, H, filter=flt, params=params)
        shadow, _, _ = ptss.probe_splat_paths(res, pos, shadow, W, H, filter=flt, params=params)
        scatter = index if index is not None else np.arange(N, dtype=np.uint32)   # the scatter form, also for the uniform rounds
        none, moments = r.accumulate_paths_linear_stats(res, None, moments, index=scatter, params=params)
        _, shadow_m, dropped = ptss.probe_accumulate_linear_stats(res, None, shadow_m, index=scatter, params=params)
        assert none is None and dropped == 0 and film.tobytes() == shadow.tobytes() and moment_words(moments).tobytes() == moment_words(shadow_m).tobytes(), k
        if k >= 3:
            cdf, index, info = r.plan_samples_linear(moments, N, params, plan)
            want_cdf, want_index, want_info = ptss.probe_plan_samples_linear(shadow_m, N, params, plan)
            assert np.array_equal(cdf, want_cdf) and np.array_equal(index, want_index) and info == want_info, k
    linear, pixels, history = r.resolve_splat(film, params=params)
    want_linear, want_pixels, want_history = ptss.probe_resolve_splat(shadow, params=params)
    assert same_words(linear, want_linear) and np.array_equal(pixels, want_pixels) and same_words(history, want_history)
    assert moments["samples"].min() >= 4 and moments["samples"].max() > 8 and r.linear_stats_launches() == (8, 5)
    r.close()


# ---- 4. no trace in frame state; a second stream; two shards -------------------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    pixels, n = 80 * 30, 3000
    g = np.random.default_rng(1)
    res = results_of(g.uniform(0, 3, (n, 3)).astype(np.float32))
    index = np.sort(g.integers(0, pixels, n)).astype(np.uint32)
    params, plan = ptss.linear_params(), ptss.linear_plan_params(min_samples=1, max_samples=64, threshold=0.05)
    want_film, want_m, _ = ptss.probe_accumulate_linear_stats(res, linear_film(pixels), zero_moments(pixels), index=index, params=params)
    want_cdf, want_index, want_info = ptss.probe_plan_samples_linear(want_m, n, params, plan)
    side = torch.cuda.Stream()
    d_res = torch.from_numpy(words(res).view(np.float32).copy()).cuda()
    d_index = torch.from_numpy(index.view(np.int32).copy()).cuda()
    for tick in range(4):
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        film, moments = r.accumulate_paths_linear_stats(res, linear_film(pixels), zero_moments(pixels), index=index, params=params)   # on the context's stream
        cdf, got_index, info = r.plan_samples_linear(moments, n, params, plan)
        assert film_words(film).tobytes() == film_words(want_film).tobytes() and moment_words(moments).tobytes() == moment_words(want_m).tobytes(), tick
        assert np.array_equal(cdf, want_cdf) and np.array_equal(got_index, want_index) and info == want_info, tick
        with torch.cuda.stream(side):   # and on a second one
            d_film = torch.zeros((pixels, 4), dtype=torch.int64, device="cuda")
            d_m = torch.zeros((pixels, 4), dtype=torch.int64, device="cuda")
            d_cdf = torch.zeros(ptss.plan_cdf_entries(pixels), dtype=torch.int64, device="cuda")
            d_plan = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_info = torch.zeros(4, dtype=torch.int64, device="cuda")
            r.accumulate_paths_linear_stats(d_res, d_film, d_m, index=d_index, params=params)
            r.plan_samples_linear(d_m, n, params, plan, cdf=d_cdf, index=d_plan, info=d_info)
        side.synchronize()
        assert d_film.cpu().numpy().tobytes() == film_words(want_film).tobytes() and d_m.cpu().numpy().tobytes() == moment_words(want_m).tobytes(), tick
        assert np.array_equal(d_cdf.cpu().numpy().view(np.uint64)[:pixels], want_cdf) and np.array_equal(d_plan.cpu().numpy().view(np.uint32), want_index), tick
        assert ptss.plan_info_dict(d_info.cpu().numpy()) == want_info, tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "four frames with the two calls after each", W, H, 1)
    assert r.linear_stats_launches() == (8, 8) and r.linear_launches() == (0, 0) and r.adaptive_launches() == (0, 0) and r.film_launches() == (0, 0, 0)
    assert r.film_rejected() == 0
    o.close()
    r.close()


def test_a_sharded_context_answers_as_the_unsharded_one():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    g = np.random.default_rng(5)
    res = results_of(g.uniform(0, 3, (N, 3)).astype(np.float32))
    index = np.sort(g.integers(0, N, N)).astype(np.uint32)
    params, plan = ptss.linear_params(), ptss.linear_plan_params(min_samples=1, max_samples=64, threshold=0.05)
    want_film, want_m, _ = ptss.probe_accumulate_linear_stats(res, linear_film(N), zero_moments(N), index=index, params=params)
    want = ptss.probe_plan_samples_linear(want_m, N, params, plan)
    for rank in (None, 0, 1):
        tile = {} if rank is None else dict(tile_rank=rank, tile_world=2, band_rows=8)
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, **tile)
        film, moments = r.accumulate_paths_linear_stats(res, linear_film(N), zero_moments(N), index=index, params=params)   # all of the film, whatever rows the shard owns
        assert film_words(film).tobytes() == film_words(want_film).tobytes() and moment_words(moments).tobytes() == moment_words(want_m).tobytes(), rank
        cdf, got_index, info = r.plan_samples_linear(moments, N, params, plan)
        assert np.array_equal(cdf, want[0]) and np.array_equal(got_index, want[1]) and info == want[2], rank
        assert r.linear_stats_launches() == (1, 1)
        r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n, pixels = 300, 20 * 15
    entries = ptss.plan_cdf_entries(pixels)
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("s_res", n * 16), ("s_film", pixels * 32), ("s_mom", pixels * 32), ("s_index", n * 4), ("s_cdf", entries * 8), ("s_info", 32))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_res, d_film, d_mom, d_index, d_cdf, d_info = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    good, gplan = ptss.linear_params(), ptss.linear_plan_params()
    ref = lambda s: C.byref(s) if s is not None else None
    acc = lambda ctx, res, index, first, count, film, mom, px, p=good: L.ptss_accumulate_paths_linear_stats(ctx, res, index, first, count, film, mom, px, ref(p), None)
    plan = lambda ctx, mom, px, count, cdf, index, info, p=good, q=gplan: L.ptss_plan_samples_linear(ctx, mom, px, ref(p), ref(q), count, cdf, index, info, None)
    assert acc(r._ctx, d_res, None, 0, n, d_film, d_mom, pixels) == 0
    assert plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, d_info) == 0
    r.synchronize()
    counters, kernels = r.linear_stats_launches(), r.launched_kernels()
    others = (r.linear_launches(), r.adaptive_launches(), r.film_launches())
    assert counters == (1, 1) and r.film_rejected() == 0 and others == ((0, 0), (0, 0), (0, 0, 0))

    def snapshot():
        out = []
        for (_, size), dev in zip(sizes, bufs):
            host = np.empty(size + 16, np.uint8)
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
            out.append(host)
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)

    def changed(make, **change):
        s = make()
        for k, v in change.items():
            setattr(s, k, v)
        return s

    bad_film = [changed(ptss.linear_params, **c) for c in (dict(structSize=16), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=float("inf")),
                                                           dict(scaleLog2=32, clampMax=257.0), dict(exposure=-1.0), dict(exposure=float("nan")), dict(reserved=1))]
    # ptss_accumulate_paths_linear_stats: ptss_accumulate_paths_linear's refusals, and the moments'
    assert acc(None, d_res, None, 0, n, d_film, d_mom, pixels) == EINVAL
    assert acc(r._ctx, None, None, 0, n, d_film, d_mom, pixels) == EINVAL and acc(r._ctx, d_res, None, 0, n, d_film, None, pixels) == EINVAL
    assert acc(r._ctx, d_res, None, 0, n, d_film, d_mom, pixels, None) == EINVAL
    for p in bad_film:
        assert acc(r._ctx, d_res, None, 0, n, d_film, d_mom, pixels, p) == EINVAL and acc(r._ctx, d_res, None, 0, 0, d_film, d_mom, pixels, p) == EINVAL
        assert plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, d_info, p) == EINVAL
    for k in (4, 8, 12):
        assert acc(r._ctx, off(d_res, k), None, 0, n, d_film, d_mom, pixels) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, off(d_film, k), d_mom, pixels) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, d_film, off(d_mom, k), pixels) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, None, off(d_mom, k), pixels) == EINVAL, k
        assert plan(r._ctx, off(d_mom, k), pixels, n, d_cdf, d_index, d_info) == EINVAL, k
    for k in (1, 2, 3):
        assert acc(r._ctx, d_res, off(d_index, k), 0, n, d_film, d_mom, pixels) == EINVAL, k
        assert plan(r._ctx, d_mom, pixels, n, d_cdf, off(d_index, k), d_info) == EINVAL, k
    assert acc(r._ctx, d_res, d_index, 0, 2 ** 31, d_film, d_mom, pixels) == ERANGE
    assert acc(r._ctx, d_res, d_index, 0, n, d_film, d_mom, 2 ** 31) == ERANGE
    for first, count, px in ((1, n, n), (pixels - n + 1, n, pixels), (pixels, 1, pixels), (0, n, n - 1), (2 ** 63, 2, pixels)):
        assert acc(r._ctx, d_res, None, first, count, d_film, d_mom, px) == ERANGE, (first, count, px)
    assert acc(r._ctx, None, None, 0, 0, None, None, pixels) == 0   # n = 0
    # ptss_plan_samples_linear: ptss_plan_samples' refusals, and the plan parameters'
    assert plan(None, d_mom, pixels, n, d_cdf, d_index, d_info) == EINVAL
    assert plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, d_info, None) == EINVAL and plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, d_info, good, None) == EINVAL
    assert plan(r._ctx, None, pixels, n, d_cdf, d_index, d_info) == EINVAL and plan(r._ctx, d_mom, pixels, n, None, d_index, d_info) == EINVAL
    assert plan(r._ctx, d_mom, pixels, n, d_cdf, None, d_info) == EINVAL
    for change in (dict(structSize=20), dict(structSize=0), dict(minSamples=0), dict(maxSamples=0), dict(maxSamples=(1 << 23) + 1), dict(minSamples=9, maxSamples=8),
                   dict(threshold=-0.25), dict(threshold=float("inf")), dict(threshold=float("nan")), dict(floor=float("inf")), dict(floor=float("nan")),
                   dict(floor=-1.0), dict(floor=0.0), dict(floor=2.0 ** -21), dict(floor=65537.0)):
        q = changed(ptss.linear_plan_params, **change)
        assert plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, d_info, good, q) == EINVAL, change
        assert plan(r._ctx, d_mom, pixels, 0, d_cdf, d_index, d_info, good, q) == EINVAL, change
    for k in range(3):
        q = ptss.linear_plan_params()
        q.reserved[k] = 1
        assert plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, d_info, good, q) == EINVAL, k
    for k in (1, 2, 4, 6):
        assert plan(r._ctx, d_mom, pixels, n, off(d_cdf, k), d_index, d_info) == EINVAL, k
        assert plan(r._ctx, d_mom, pixels, n, d_cdf, d_index, off(d_info, k)) == EINVAL, k
    for px in (0, 2 ** 31, 2 ** 40):
        assert plan(r._ctx, d_mom, px, n, d_cdf, d_index, d_info) == ERANGE, px
    for count in (2 ** 31, 2 ** 40):
        assert plan(r._ctx, d_mom, pixels, count, d_cdf, d_index, d_info) == ERANGE, count
    assert plan(r._ctx, None, pixels, 0, None, None, None) == 0   # n = 0
    out2 = (C.c_ulonglong * 2)()
    assert L.ptss_linear_stats_launches(None, out2) == EINVAL and L.ptss_linear_stats_launches(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.linear_stats_launches() == counters and r.launched_kernels() == kernels and r.film_rejected() == 0
    assert (r.linear_launches(), r.adaptive_launches(), r.film_launches()) == others
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: a NULL film, 16-byte offsets, a 4-byte aligned index, a NULL info, the boundary parameters
    assert acc(r._ctx, d_res, off(d_index, 4), 0, n - 2, None, off(d_mom, 16), pixels - 1) == 0
    edge = ptss.linear_plan_params(min_samples=1 << 23, max_samples=1 << 23, threshold=0.0, floor=2.0 ** -20)
    assert plan(r._ctx, off(d_mom, 16), pixels - 1, n - 1, off(d_cdf, 8), off(d_index, 4), None, good, edge) == 0
    r.synchronize()
    assert r.linear_stats_launches() == (2, 2) and r.launched_kernels() == kernels and r.film_rejected() == 0
    r.close()
