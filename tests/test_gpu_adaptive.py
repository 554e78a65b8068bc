"""Adaptive film sampling on the GPU (ptss_accumulate_paths_stats / ptss_plan_samples). Every test requires the device
to equal the host probes byte for byte.

1. ptss_accumulate_paths_stats against ptss_accumulate_paths (film, pixels, history, rejected) and the probe (moments): identity maps,
   a permuted index, sorted indices whose runs cross wave and workgroup edges, one pixel for every ray, entries beyond the film inside
   and between runs, the tone map's adversarial rows, a film carried over four calls, each combination of NULL outputs.
2. ptss_plan_samples' cdf, index and info against the probe: films below, at and beyond the scan's tiles and beyond one pass of the tile
   sums, budgets around a wave, every kind of film content. 3. The loop generate -> trace -> accumulate -> plan against a shadow loop of the two probes.
4. No trace in frame state, a second stream, a sharded context. 5. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from adaptive_common import SCAN_TILE, check_plan, film_of, random_bytes_film
from film_common import BATCHES, adversarial_radiance, results_of, words
from path_query_common import H, N, SCENES, W, camera_of, make_scene
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu


def same_words(a, b):
    """Equal 32-bit words, a NaN standing for any NaN."""
    a, b = words(a), words(b)
    if a.shape != b.shape:
        return False
    fa, fb = a.view(np.float32), b.view(np.float32)
    return bool(((a == b) | (np.isnan(fa) & np.isnan(fb))).all())


@pytest.fixture(scope="module")
def small():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    yield r
    r.close()


# ---- 1. accumulation with moments ----------------------------------------------------------------------------------------------------------
def runs_index(lengths, P, g):
    """A sorted index: run k names a pixel of its own lengths[k] times, the pixels increasing."""
    pixels = np.sort(g.choice(P, len(lengths), replace=False))
    return np.repeat(pixels, lengths).astype(np.uint32)


def test_stats_accumulate_equals_accumulate_and_the_probe(small):
    r, g = small, np.random.default_rng(9)
    rad = adversarial_radiance()
    M, P = len(rad), W * H
    more = np.concatenate([rad, g.uniform(0, 1.2, (P - M, 3)).astype(np.float32) ** 3])   # one row per film pixel, the adversarial rows first
    res = results_of(more)
    start = np.zeros(P, dtype=ptss.FILM_DTYPE)
    start["r"], start["g"], start["b"], start["samples"] = 1000, 2000, 3000, 40   # a film that has been in use
    m0 = g.integers(0, 2 ** 40, P).astype(np.uint64)
    px0, hs0 = np.full((P, 4), 9, np.uint8), np.full((P, 4), -2.0, np.float32)
    before = r.film_rejected()
    launches = r.adaptive_launches()[0]

    def check(what, n, **kw):
        nonlocal before, launches
        for pixels, history in ((px0, hs0), (px0, None), (None, hs0), (None, None)):   # each combination of the two outputs
            film, moments, px, hs = r.accumulate_paths_stats(res[:n], start, m0, pixels=pixels, history=history, **kw)
            launches += 1
            plain, plain_px, plain_hs = r.accumulate_paths(res[:n], start, pixels=pixels, history=history, **kw)
            want, want_m, want_px, want_hs, rejected = ptss.probe_accumulate_stats(res[:n], start, m0, pixels=pixels, history=history, **kw)
            assert np.array_equal(words(film), words(plain)) and np.array_equal(words(film), words(want)), what
            assert np.array_equal(moments, want_m), what
            assert (px is None) == (pixels is None) and (hs is None) == (history is None)
            assert px is None or (np.array_equal(px, plain_px) and np.array_equal(px, want_px)), what
            assert hs is None or (same_words(hs, plain_hs) and same_words(hs, want_hs)), what
            before += 2 * rejected   # both device calls count what they drop
            assert r.film_rejected() == before, what
        assert r.adaptive_launches()[0] == launches
        return film, moments

    film, _ = check("identity map", P)
    assert (film["samples"] == 41).all()
    for n in BATCHES:   # a part of the film from a first pixel > 0: the rest stays untouched
        film, moments = check(("first pixel 1000", n), n, first_pixel=1000)
        rest = np.ones(P, bool)
        rest[1000:1000 + n] = False
        assert (film["samples"][rest] == 40).all() and np.array_equal(moments[rest], m0[rest]), n
    check("permuted index", P, index=g.permutation(P).astype(np.uint32))
    # sorted indices: runs of 1, 2, 63, 64, 65 and 300 in several orders, so that runs start anywhere in a wave and cross wave and workgroup edges
    for k, lengths in enumerate(([1, 2, 63, 64, 65, 300, 1, 1, 65, 64, 63, 2, 300, 64, 64, 1, 300], [300, 300, 65, 1, 63, 63, 2, 64, 1, 1, 1, 65, 300],
                                 [64] * 12 + [1] * 70 + [2] * 40, [3] * 600)):
        index = runs_index(lengths, P, g)
        film, _ = check(("sorted runs", k), len(index), index=index)
        assert film["samples"].sum() == 40 * P + len(index)
        wild = index.copy()   # entries beyond the film inside runs and between them
        inside = g.choice(len(wild), 40, replace=False)
        wild[inside] = g.choice([P, P + 1, 2 ** 31, 2 ** 32 - 1], 40)
        edges = np.flatnonzero(np.diff(index) != 0)[::3]
        wild[edges] = P + 7
        check(("sorted runs with entries beyond the film", k), len(wild), index=wild)
    film, _ = check("every ray on one pixel", P, index=np.full(P, 1234, np.uint32))
    assert film["samples"][1234] == 40 + P and film["samples"].sum() == 41 * P
    few = g.integers(0, 40, P).astype(np.uint32) * 77   # duplicates that are not neighbours
    check("many to few", P, index=few)
    check("nothing inside the film", 300, index=np.full(300, P, np.uint32))
    # a film carried over four calls, with and without an index
    film, moments, want, want_m = start, m0, start, m0
    for k in range(4):
        index = None if k % 2 == 0 else np.sort(g.integers(0, P, P)).astype(np.uint32)
        rows = results_of(g.permutation(more))
        film, moments, px, hs = r.accumulate_paths_stats(rows, film, moments, index=index, pixels=True, history=True)
        want, want_m, want_px, want_hs, _ = ptss.probe_accumulate_stats(rows, want, want_m, index=index, pixels=True, history=True)
        assert np.array_equal(words(film), words(want)) and np.array_equal(moments, want_m) and np.array_equal(px, want_px) and same_words(hs, want_hs), k
    assert film["samples"].sum() == 44 * P


# ---- 2. the plan -------------------------------------------------------------------------------------------------------------------------------
PLAN = dict(min_samples=4, max_samples=40, threshold=0.75)
FILM_PIXELS = (1, 5 * 3, 64 * 48, SCAN_TILE + 1, 2 * SCAN_TILE + 1)   # (the scan has two levels: no tile of tiles)


def plan_films(P):
    """name -> (film, moments) of P pixels: every kind of content the plan meets."""
    g = np.random.default_rng(P)
    flat, flat_m = film_of(np.full(P, 10), g, spread=0.0)   # every pixel converged
    noisy, noisy_m = film_of(g.integers(0, 48, P), g)        # unsampled, live, converged and capped pixels mixed
    out = {"all zero": (np.zeros(P, ptss.FILM_DTYPE), np.zeros(P, np.uint64)), "all converged": (flat, flat_m), "mixed": (noisy, noisy_m),
           "random bytes": random_bytes_film(P, g)}
    for where, p in (("first", 0), ("last", P - 1), ("before a tile edge", SCAN_TILE - 1), ("at a tile edge", SCAN_TILE), ("at the second tile edge", 2 * SCAN_TILE)):
        if p < P and (where in ("first", "last") or P > SCAN_TILE):
            film, moments = flat.copy(), flat_m.copy()
            film["r"][p], film["g"][p], film["b"][p] = 1000, 800, 1200
            moments[p] = 10 * (255 ** 2) * 2   # far from its mean: a live pixel
            out["one live pixel " + where] = (film, moments)
    capped = flat.copy()   # weights at the cap of 2^19 - 1: moments no film of bytes could have
    out["weights at the cap"] = (capped, np.full(P, 2 ** 40, np.uint64))
    full = noisy.copy()
    full["samples"][::2] = 40   # pixels at maxSamples between live ones
    full["samples"][1::5] = 39
    out["pixels at maxSamples"] = (full, noisy_m)
    return out


@pytest.mark.parametrize("P", FILM_PIXELS)
def test_plan_equals_the_host_probe(small, P):
    r, params = small, ptss.plan_params(**PLAN)
    launches = r.adaptive_launches()[1]
    seen_uniform = seen_live = 0
    for name, (film, moments) in plan_films(P).items():
        for n in (1, 63, 64, 65, 257, 4 * P):
            cdf, index, info = r.plan_samples(film, moments, n, params)
            want_cdf, want_index, want_info = ptss.probe_plan_samples(film, moments, n, params)
            assert np.array_equal(cdf, want_cdf), (name, n)
            assert np.array_equal(index, want_index), (name, n)
            assert info == want_info, (name, n, info, want_info)
            launches += 1
        seen_uniform += info["uniform"]
        seen_live += info["activePixels"] > 0
        if name == "all zero":
            assert info["unsampledPixels"] == P and info["totalWeight"] == P << 19
        if name == "all converged":
            assert info["uniform"] == 1 and info["activePixels"] == 0
        if name.startswith("one live pixel"):
            assert info["activePixels"] == 1 and len(np.unique(index)) == 1
        if name == "weights at the cap":
            assert info["totalWeight"] == P * 524287
        if name == "pixels at maxSamples":
            assert info["cappedPixels"] >= 2 * P // 5   # every second pixel, less the tenth that plan_films sets to 39 afterwards
        if P <= 64 * 48 and name in ("mixed", "random bytes", "pixels at maxSamples"):
            check_plan(film, moments, 4 * P, params, cdf, index, info)   # (the last budget) the model's weights and the three properties
    assert seen_uniform >= 1 and seen_live >= 3
    assert r.adaptive_launches()[1] == launches


def test_plan_of_a_film_beyond_one_pass_of_the_tile_sums(small):
    """The one workgroup that scans the tile sums takes 1,024 tiles per pass and carries the sum over: a film of 1,024 tiles and a pixel."""
    r, params = small, ptss.plan_params(**PLAN)
    P = 1024 * SCAN_TILE + 1
    g = np.random.default_rng(7)
    film, moments = random_bytes_film(P, g)
    lone = np.zeros(P, ptss.FILM_DTYPE)   # every pixel capped but the last, the second pass's only one
    lone["samples"] = 40
    lone["samples"][P - 1] = 0
    for what, f, m in (("random bytes", film, moments), ("only the last pixel", lone, np.zeros(P, np.uint64))):
        for n in (257, 100001):
            cdf, index, info = r.plan_samples(f, m, n, params)
            want_cdf, want_index, want_info = ptss.probe_plan_samples(f, m, n, params)
            assert np.array_equal(cdf, want_cdf) and np.array_equal(index, want_index) and info == want_info, (what, n, info, want_info)
    assert info == dict(totalWeight=1 << 19, activePixels=1, unsampledPixels=1, cappedPixels=P - 1, uniform=0) and (index == P - 1).all()


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_the_loop_equals_a_shadow_loop_of_the_probes(placement):
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    params = ptss.plan_params(min_samples=4, max_samples=64, threshold=0.5)
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = shadow = np.zeros(N, dtype=ptss.FILM_DTYPE)
    moments = shadow_m = np.zeros(N, dtype=np.uint64)
    index = None
    rejected0 = r.film_rejected()
    for k in range(8):   # four uniform rounds, then four planned rounds of 3,072 rays
        what = (placement, k)
        rays, rng = r.generate_rays(film_cam, rng, index=index)   # ray slot i keeps stream i whatever pixel it is given
        res, rng = r.trace_paths(rays, rng, iterations)
        total = int(film["samples"].sum())
        film, moments, pixels, history = r.accumulate_paths_stats(res, film, moments, index=index, pixels=True, history=True)
        shadow, shadow_m, want_px, want_hs, dropped = ptss.probe_accumulate_stats(res, shadow, shadow_m, index=index, pixels=True, history=True)
        assert np.array_equal(words(film), words(shadow)) and np.array_equal(moments, shadow_m), what
        assert np.array_equal(pixels, want_px) and same_words(history, want_hs), what
        assert dropped == 0 and int(film["samples"].sum()) == total + N - dropped, what
        if k >= 3:
            cdf, index, info = r.plan_samples(film, moments, N, params)
            want_cdf, want_index, want_info = ptss.probe_plan_samples(shadow, shadow_m, N, params)
            assert np.array_equal(cdf, want_cdf) and np.array_equal(index, want_index) and info == want_info, what
            assert info["unsampledPixels"] == 0 and 0 < info["activePixels"] < N and info["uniform"] == 0, (what, info)
            assert (np.diff(index.astype(np.int64)) >= 0).all()
    assert film["samples"].min() >= 4 and film["samples"].max() > 8   # the planned rays went to some pixels and not to others
    assert r.film_rejected() == rejected0 and r.adaptive_launches() == (8, 5)
    r.close()


# ---- 4. no trace in frame state; a second stream; a sharded context --------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    P, n = 80 * 30, 3000
    g = np.random.default_rng(1)
    res = results_of(g.uniform(0, 1, (n, 3)).astype(np.float32))
    index = np.sort(g.integers(0, P, n)).astype(np.uint32)
    params = ptss.plan_params(min_samples=1, max_samples=64, threshold=0.5)
    zero, zero_m = np.zeros(P, ptss.FILM_DTYPE), np.zeros(P, np.uint64)
    want_film, want_m, want_px, _, _ = ptss.probe_accumulate_stats(res, zero, zero_m, index=index, pixels=True)
    want_cdf, want_index, want_info = ptss.probe_plan_samples(want_film, want_m, n, params)
    side = torch.cuda.Stream()
    d_res = torch.from_numpy(words(res).view(np.float32).copy()).cuda()
    d_index = torch.from_numpy(index.view(np.int32).copy()).cuda()
    for tick in range(6):
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        film, moments, px, _ = r.accumulate_paths_stats(res, zero, zero_m, index=index, pixels=True)   # on the context's stream
        cdf, plan, info = r.plan_samples(film, moments, n, params)
        assert np.array_equal(words(film), words(want_film)) and np.array_equal(moments, want_m) and np.array_equal(px, want_px), tick
        assert np.array_equal(cdf, want_cdf) and np.array_equal(plan, want_index) and info == want_info, tick
        with torch.cuda.stream(side):   # and on a second one
            d_film = torch.zeros((P, 4), dtype=torch.int32, device="cuda")
            d_m = torch.zeros(P, dtype=torch.int64, device="cuda")
            d_px = torch.zeros((P, 4), dtype=torch.uint8, device="cuda")
            d_cdf = torch.zeros(ptss.plan_cdf_entries(P), dtype=torch.int64, device="cuda")
            d_plan = torch.zeros(n, dtype=torch.int32, device="cuda")
            d_info = torch.zeros(4, dtype=torch.int64, device="cuda")
            r.accumulate_paths_stats(d_res, d_film, d_m, index=d_index, pixels=d_px)
            r.plan_samples(d_film, d_m, n, params, cdf=d_cdf, index=d_plan, info=d_info)
        side.synchronize()
        assert np.array_equal(d_film.cpu().numpy().view(np.uint32), words(want_film)) and np.array_equal(d_px.cpu().numpy(), want_px), tick
        assert np.array_equal(d_m.cpu().numpy().view(np.uint64), want_m), tick
        assert np.array_equal(d_cdf.cpu().numpy().view(np.uint64)[:P], want_cdf) and np.array_equal(d_plan.cpu().numpy().view(np.uint32), want_index), tick
        assert ptss.plan_info_dict(d_info.cpu().numpy()) == want_info, tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "six frames with the two adaptive calls after each", W, H, 1)
    assert r.adaptive_launches() == (12, 12) and r.film_launches() == (0, 0, 0) and r.film_rejected() == 0
    o.close()
    r.close()


def test_a_sharded_context_answers_as_the_unsharded_one():
    name = "mixed"
    seed = SCENES[name][3]
    scene = make_scene(name)
    g = np.random.default_rng(5)
    res = results_of(g.uniform(0, 1, (N, 3)).astype(np.float32))
    index = np.sort(g.integers(0, N, N)).astype(np.uint32)
    params = ptss.plan_params(min_samples=1, max_samples=64, threshold=0.5)
    zero, zero_m = np.zeros(N, ptss.FILM_DTYPE), np.zeros(N, np.uint64)
    want_film, want_m, want_px, _, _ = ptss.probe_accumulate_stats(res, zero, zero_m, index=index, pixels=True)
    want = ptss.probe_plan_samples(want_film, want_m, N, params)
    for rank in (None, 0, 1):
        tile = {} if rank is None else dict(tile_rank=rank, tile_world=2, band_rows=8)
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, **tile)
        film, moments, px, _ = r.accumulate_paths_stats(res, zero, zero_m, index=index, pixels=True)   # all of the film, whatever rows the shard owns
        assert np.array_equal(words(film), words(want_film)) and np.array_equal(moments, want_m) and np.array_equal(px, want_px), rank
        cdf, plan, info = r.plan_samples(film, moments, N, params)
        assert np.array_equal(cdf, want[0]) and np.array_equal(plan, want[1]) and info == want[2], rank
        assert r.adaptive_launches() == (1, 1)
        r.close()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n, P = 300, 20 * 15
    entries = ptss.plan_cdf_entries(P)
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    sizes = (("a_res", n * 16), ("a_film", P * 16), ("a_mom", P * 8), ("a_pix", P * 4), ("a_hist", P * 16), ("a_index", n * 4), ("a_cdf", entries * 8),
             ("a_info", 32))
    bufs = [r._device_buffer(name, size + 16) for name, size in sizes]
    d_res, d_film, d_mom, d_pix, d_hist, d_index, d_cdf, d_info = bufs
    for (_, size), dev in zip(sizes, bufs):
        ptss._hip_check(Hip.hipMemset(dev, 0, size + 16), "hipMemset")
    good = ptss.plan_params()
    acc = lambda ctx, res, index, first, count, film, mom, pixels, px, hs: L.ptss_accumulate_paths_stats(ctx, res, index, first, count, film, mom, pixels, px, hs, None)
    plan = lambda ctx, film, mom, pixels, params, count, cdf, index, info: L.ptss_plan_samples(ctx, film, mom, pixels, C.byref(params) if params is not None else None,
                                                                                               count, cdf, index, info, None)
    assert acc(r._ctx, d_res, None, 0, n, d_film, d_mom, P, d_pix, d_hist) == 0
    assert plan(r._ctx, d_film, d_mom, P, good, n, d_cdf, d_index, d_info) == 0
    r.synchronize()
    counters, kernels = r.adaptive_launches(), r.launched_kernels()
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
    # ptss_accumulate_paths_stats: ptss_accumulate_paths' refusals, and the moments'
    assert acc(None, d_res, None, 0, n, d_film, d_mom, P, d_pix, d_hist) == EINVAL
    assert acc(r._ctx, None, None, 0, n, d_film, d_mom, P, d_pix, d_hist) == EINVAL and acc(r._ctx, d_res, None, 0, n, None, d_mom, P, d_pix, d_hist) == EINVAL
    assert acc(r._ctx, d_res, None, 0, n, d_film, None, P, d_pix, d_hist) == EINVAL
    for k in (4, 8, 12):
        assert acc(r._ctx, off(d_res, k), None, 0, n, d_film, d_mom, P, d_pix, d_hist) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, off(d_film, k), d_mom, P, d_pix, d_hist) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, d_film, d_mom, P, d_pix, off(d_hist, k)) == EINVAL, k
    for k in (1, 2, 3, 4, 5, 6, 7):
        assert acc(r._ctx, d_res, None, 0, n, d_film, off(d_mom, k), P, d_pix, d_hist) == EINVAL, k
    for k in (1, 2, 3):
        assert acc(r._ctx, d_res, off(d_index, k), 0, n, d_film, d_mom, P, d_pix, d_hist) == EINVAL, k
        assert acc(r._ctx, d_res, None, 0, n, d_film, d_mom, P, off(d_pix, k), d_hist) == EINVAL, k
    assert acc(r._ctx, d_res, d_index, 0, 2 ** 31, d_film, d_mom, P, d_pix, d_hist) == ERANGE
    assert acc(r._ctx, d_res, d_index, 0, n, d_film, d_mom, 2 ** 31, d_pix, d_hist) == ERANGE
    for first, count, pixels in ((1, n, n), (P - n + 1, n, P), (P, 1, P), (0, n, n - 1), (2 ** 63, 2, P)):
        assert acc(r._ctx, d_res, None, first, count, d_film, d_mom, pixels, d_pix, d_hist) == ERANGE, (first, count, pixels)
    assert acc(r._ctx, None, None, 0, 0, None, None, P, None, None) == 0   # n = 0
    # ptss_plan_samples
    assert plan(None, d_film, d_mom, P, good, n, d_cdf, d_index, d_info) == EINVAL and plan(r._ctx, d_film, d_mom, P, None, n, d_cdf, d_index, d_info) == EINVAL
    assert plan(r._ctx, None, d_mom, P, good, n, d_cdf, d_index, d_info) == EINVAL and plan(r._ctx, d_film, None, P, good, n, d_cdf, d_index, d_info) == EINVAL
    assert plan(r._ctx, d_film, d_mom, P, good, n, None, d_index, d_info) == EINVAL and plan(r._ctx, d_film, d_mom, P, good, n, d_cdf, None, d_info) == EINVAL
    for change in (dict(structSize=12), dict(structSize=0), dict(minSamples=0), dict(maxSamples=0), dict(maxSamples=(1 << 23) + 1), dict(minSamples=9, maxSamples=8),
                   dict(threshold=-0.25), dict(threshold=float("inf")), dict(threshold=float("nan"))):
        params = ptss.plan_params()
        for k, v in change.items():
            setattr(params, k, v)
        assert plan(r._ctx, d_film, d_mom, P, params, n, d_cdf, d_index, d_info) == EINVAL, change
    for k in (4, 8, 12):
        assert plan(r._ctx, off(d_film, k), d_mom, P, good, n, d_cdf, d_index, d_info) == EINVAL, k
    for k in (1, 2, 4, 6):
        assert plan(r._ctx, d_film, off(d_mom, k), P, good, n, d_cdf, d_index, d_info) == EINVAL, k
        assert plan(r._ctx, d_film, d_mom, P, good, n, off(d_cdf, k), d_index, d_info) == EINVAL, k
        assert plan(r._ctx, d_film, d_mom, P, good, n, d_cdf, d_index, off(d_info, k)) == EINVAL, k
    for k in (1, 2, 3):
        assert plan(r._ctx, d_film, d_mom, P, good, n, d_cdf, off(d_index, k), d_info) == EINVAL, k
    for pixels in (0, 2 ** 31, 2 ** 40):
        assert plan(r._ctx, d_film, d_mom, pixels, good, n, d_cdf, d_index, d_info) == ERANGE, pixels
    for count in (2 ** 31, 2 ** 40):
        assert plan(r._ctx, d_film, d_mom, P, good, count, d_cdf, d_index, d_info) == ERANGE, count
    assert plan(r._ctx, None, None, P, good, 0, None, None, None) == 0   # n = 0
    out2 = (C.c_ulonglong * 2)()
    assert L.ptss_adaptive_launches(None, out2) == EINVAL and L.ptss_adaptive_launches(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.adaptive_launches() == counters and r.launched_kernels() == kernels and r.film_rejected() == 0
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    # what is allowed: 8-byte aligned moments, a 4-byte aligned index, NULL outputs, the boundary parameters
    assert acc(r._ctx, d_res, off(d_index, 4), 0, n - 2, d_film, off(d_mom, 8), P, off(d_pix, 4), None) == 0
    edge = ptss.plan_params(min_samples=1 << 23, max_samples=1 << 23, threshold=0.0)
    assert plan(r._ctx, d_film, off(d_mom, 8), P, edge, n - 1, off(d_cdf, 8), off(d_index, 4), None) == 0
    r.synchronize()
    assert r.adaptive_launches() == (2, 2) and r.launched_kernels() == kernels and r.film_rejected() == 0
    r.close()
