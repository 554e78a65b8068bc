"""Path queries with the refill schedule on the GPU (ptss_trace_paths_opt with PTSS_PATHS_REFILL).

Every comparison is byte for byte: the 16-byte result rows and all six stream words.
1. The refill call equals ptss_trace_paths: eight scenes, the image staged in LDS and read in place, the frame's own 64 x 48 eye rays
   and streams, maxIterations 1, 2, 8, 15, 64, maxWorkgroups 1, 2, 7, 0. With one workgroup 3,072 rays go through 256 lanes: the queue
   is twelve fills deep.  2. Batch edges.  3. Arbitrary rays (NaN, infinite and zero components), shuffled, with duplicates.
4. The oracle directly.  5. The counters against the bound of tests/path_refill_common.py and against the plain schedule's count.
6. Continuation.  7. Frames untouched.  8. Shards and a re-sorted live mesh.  9. The film.  10. Refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from film_common import ROUNDS, frames_of
from path_query_common import (H, MOVED_FIRST, N, SCENES, W, camera_of, expected, eye_rays, in_place, make_scene, moved_mesh,
                               satisfies_identity_condition)
from path_refill_common import BLOCK, WAVES, plain_wave_iterations, wave_iteration_bound
from test_gpu_film import arbitrary_rays
from test_gpu_kernel_coverage import compare
from test_gpu_path_query import open_scene, outside_rays

pytestmark = pytest.mark.gpu

MAX_ITERATIONS = (1, 2, 8, 15, 64)
MAX_WORKGROUPS = (1, 2, 7, 0)
COUNTED = 15   # maxIterations of the counter test


def words(a):
    """The 32-bit words of a record or float array, one row per entry."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def same_bytes(got, want):
    return np.array_equal(words(got[0]), words(want[0])) and np.array_equal(words(got[1]), words(want[1]))


def mismatches(got, want):
    return int((words(got[0]) != words(want[0])).any(axis=1).sum()), int((words(got[1]) != words(want[1])).any(axis=1).sum())


def renderer(name, placement="lds", **kw):
    _, every, _, seed = SCENES[name]
    r = ptss.Renderer(make_scene(name, placement), W, H, max_iterations=8, seed=seed, every_sphere_loop=every, **kw)
    r.set_camera(camera_of(name))
    return r


_INPUTS = {}


def inputs(name):
    """(the frame's own eye rays, its streams) of a case; computed once per process and never modified."""
    if name not in _INPUTS:
        seed = SCENES[name][3]
        rays = eye_rays(camera_of(name), seed)
        r = renderer(name)
        _INPUTS[name] = (rays, r.seed_path_rng(N, seed, 0, skip=2))
        r.close()
    return _INPUTS[name]


# ---- 1. equals the plain schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
@pytest.mark.parametrize("name", list(SCENES))
def test_refill_equals_the_plain_schedule(name, placement):
    rays, s0 = inputs(name)
    r = renderer(name, placement)
    calls = 0
    for iterations in MAX_ITERATIONS:
        want = r.trace_paths(rays.copy(), s0.copy(), iterations)
        assert want[0]["bounces"].min() >= 1 and want[0]["bounces"].max() <= iterations
        for cap in MAX_WORKGROUPS:
            got = r.trace_paths(rays.copy(), s0.copy(), iterations, schedule="refill", max_workgroups=cap)
            calls += 1
            assert same_bytes(got, want), (name, placement, iterations, cap, mismatches(got, want))
    stats = r.path_refill_stats()
    assert stats[:2] == ((0, calls) if placement == "lds" else (calls, 0)), stats
    assert r.path_launches() == ((0, len(MAX_ITERATIONS)) if placement == "lds" else (len(MAX_ITERATIONS), 0))
    # LANE_PER_RAY through the new entry point IS ptss_trace_paths: the same bytes, counted as its launch
    got = r.trace_paths(rays.copy(), s0.copy(), 8, schedule="lane_per_ray", max_workgroups=3)
    assert same_bytes(got, r.trace_paths(rays.copy(), s0.copy(), 8))
    assert sum(r.path_launches()) == len(MAX_ITERATIONS) + 2 and r.path_refill_stats()[:2] == stats[:2]
    r.close()


# ---- 2. batch edges -------------------------------------------------------------------------------------------------------------------
def test_batch_edges():
    name = "mixed"
    rays, s0 = inputs(name)
    r = renderer(name)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        want = r.trace_paths(rays[:n].copy(), s0[:n].copy(), 8)
        for cap in (1, 0):
            got = r.trace_paths(rays[:n].copy(), s0[:n].copy(), 8, schedule="refill", max_workgroups=cap)
            assert same_bytes(got, want), (n, cap, mismatches(got, want))
    before = r.path_refill_stats()
    res, after = r.trace_paths(rays[:0], s0[:0], 8, schedule="refill", max_workgroups=1)   # n = 0: nothing launched, nothing counted
    assert len(res) == 0 and len(after) == 0
    assert r.path_refill_stats() == before
    r.close()


# ---- 3. arbitrary rays ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_arbitrary_rays_shuffled_with_duplicates(placement):
    n = 4096
    g = np.random.default_rng(17)
    pick = g.permutation(n)
    pick[g.integers(0, n, 300)] = pick[g.integers(0, n, 300)]   # duplicated rays, each with a stream of its own
    batches = {"mixed": arbitrary_rays(n)[pick],                    # NaN, infinite and zero components among them
               "open": outside_rays(n)[pick]}                       # hits, misses and a point light
    assert np.isnan(batches["mixed"]).any() and np.isinf(batches["mixed"][:, [0, 1, 2, 4, 5, 6]]).any()
    assert (batches["mixed"][:, 4:7] == 0).all(axis=1).any()
    for what, rays in batches.items():
        scene = ptss.Scene("mixed") if what == "mixed" else open_scene()
        r = ptss.Renderer(in_place(scene) if placement == "in_place" else scene, 16, 16, max_iterations=3)
        s0 = r.seed_path_rng(n, 0xC0FFEE, 0, 0)
        want = r.trace_paths(rays.copy(), s0.copy(), 3)
        for cap in (1, 3, 0):
            got = r.trace_paths(rays.copy(), s0.copy(), 3, schedule="refill", max_workgroups=cap)
            assert same_bytes(got, want), (what, placement, cap, mismatches(got, want))
        r.close()


# ---- 4. the oracle directly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "mesh", "many_spheres"])
def test_refill_against_the_oracle(name):
    iterations = 8
    e = expected(name, iterations)
    assert satisfies_identity_condition(e.live_counts, iterations)
    rays, s0 = inputs(name)
    r = renderer(name)
    for cap in (1, 0):
        res, after = r.trace_paths(rays.copy(), s0.copy(), iterations, schedule="refill", max_workgroups=cap)
        nan = np.isnan(e.radiance)
        assert np.array_equal(np.isnan(res["radiance"]), nan), (name, cap)   # (x86 and gfx950 make different default NaNs)
        assert np.array_equal(words(res["radiance"])[~nan], words(e.radiance)[~nan]), (name, cap)
        assert np.array_equal(words(after), e.states), (name, cap)
        assert int(res["bounces"].sum()) == int(e.live_counts.sum()), (name, cap)
    r.close()


# ---- 5. counters ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
@pytest.mark.parametrize("name", list(SCENES))
def test_counters(name, placement):
    rays, s0 = inputs(name)
    r = renderer(name, placement)
    plain, _ = r.trace_paths(rays.copy(), s0.copy(), COUNTED)
    bounces = plain["bounces"].astype(np.int64)
    plain_count = plain_wave_iterations(bounces)
    bound = wave_iteration_bound(bounces, 1 * WAVES, COUNTED)
    print(f"{name} {placement}: sum(bounces) {int(bounces.sum())}, mean {bounces.mean():.2f}, plain wave iterations {plain_count}, bound {bound}")
    assert bound < plain_count, (name, bound, plain_count)   # the case can show a gain (else it is replaced in path_query_common)
    launches, kernels = r.path_launches(), r.launched_kernels()
    before = r.path_refill_stats()
    assert before == (0, 0, 0, 0, 0)
    got = r.trace_paths(rays.copy(), s0.copy(), COUNTED, schedule="refill", max_workgroups=1)
    after = r.path_refill_stats()
    wave_iterations, lane_iterations, dequeues = (after[k] - before[k] for k in (2, 3, 4))
    print(f"  refill: wave iterations {wave_iterations}, lane iterations {lane_iterations}, dequeues {dequeues}, "
          f"occupancy {lane_iterations / (64.0 * wave_iterations):.3f} against {bounces.sum() / (64.0 * plain_count):.3f}")
    assert np.array_equal(words(got[0]), words(plain))
    assert lane_iterations == int(bounces.sum())
    assert wave_iterations <= bound, (wave_iterations, bound)
    assert wave_iterations < plain_count, (wave_iterations, plain_count)
    assert dequeues > 0
    assert after[:2] == ((0, 1) if placement == "lds" else (1, 0))
    assert r.path_launches() == launches and r.launched_kernels() == kernels
    r.close()


# ---- 6. continuation ------------------------------------------------------------------------------------------------------------------
def test_continuation_and_order_independence():
    torch = pytest.importorskip("torch")
    name = "mixed"
    rays, s0 = inputs(name)
    r = renderer(name)
    res1, s1 = r.trace_paths(rays.copy(), s0.copy(), 4)
    res2, s2 = r.trace_paths(rays.copy(), s1.copy(), 4)
    assert not np.array_equal(words(s1), words(s2))
    # two refill calls with the states carried on the device (one stream: the calls are ordered)
    d_rays = torch.from_numpy(rays.copy()).cuda()
    d_rng = torch.from_numpy(words(s0).view(np.int32).copy()).cuda()
    first = r.trace_paths(d_rays, d_rng, 4, schedule="refill", max_workgroups=2)
    second = r.trace_paths(d_rays, d_rng, 4, schedule="refill", max_workgroups=2)
    torch.cuda.synchronize()
    assert np.array_equal(words(first.cpu().numpy()), words(res1)) and np.array_equal(words(second.cpu().numpy()), words(res2))
    assert np.array_equal(d_rng.cpu().numpy().view(np.uint32), words(s2))
    # a permuted batch gives permuted results, and so does a part of the batch that ends inside a wave
    perm = np.random.default_rng(1).permutation(N)
    got = r.trace_paths(rays[perm], s0[perm], 4, schedule="refill", max_workgroups=1)
    assert same_bytes(got, (res1[perm], s1[perm]))
    got = r.trace_paths(rays[:1001].copy(), s0[:1001].copy(), 4, schedule="refill", max_workgroups=1)
    assert same_bytes(got, (res1[:1001], s1[:1001]))
    r.close()


# ---- 7. frames untouched --------------------------------------------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed = SCENES[name][3]
    scene = make_scene(name)
    rays, s0 = inputs(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    twin = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)   # frames only
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    want = r.trace_paths(rays.copy(), s0.copy(), bounces)
    paths = r.path_launches()
    side = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.copy()).cuda()
    for tick in range(20):
        # a refill query on a second stream, enqueued first so that it runs beside the frame; then the frame; then one behind it on the
        # context's stream (which waits for it: the two refill calls are ordered by the host)
        with torch.cuda.stream(side):
            d_rng = torch.from_numpy(words(s0).view(np.int32).copy()).cuda()
            d_res = r.trace_paths(d_rays, d_rng, bounces, schedule="refill", max_workgroups=2)
        r.generate_frame()
        twin.generate_frame()
        o.generate_frame()
        side.synchronize()
        assert np.array_equal(words(d_res.cpu().numpy()), words(want[0])), tick
        assert np.array_equal(d_rng.cpu().numpy().view(np.uint32), words(want[1])), tick
        before = r.launched_kernels()
        got = r.trace_paths(rays.copy(), s0.copy(), bounces, schedule="refill")
        assert same_bytes(got, want), tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "twenty frames with two refill queries around each", W, H, 1)
    for p in (0, N // 2 + 7, N - 1):
        assert np.array_equal(r.rng_state(p), twin.rng_state(p)), p
    assert r.launched_kernels() == twin.launched_kernels()   # what the frames alone set
    assert r.path_launches() == paths and r.path_refill_stats()[:2] == (0, 40) and twin.path_refill_stats() == (0, 0, 0, 0, 0)
    twin.close()
    o.close()
    r.close()


# ---- 8. shards; a live scene ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_a_sharded_context_answers_as_the_unsharded_one(name):
    _, every, _, seed = SCENES[name]
    rays, s0 = inputs(name)
    whole = renderer(name)
    want = whole.trace_paths(rays.copy(), s0.copy(), 4)
    whole.close()
    for rank in range(2):
        r = ptss.Renderer(make_scene(name), W, H, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8, every_sphere_loop=every)
        got = r.trace_paths(rays.copy(), s0.copy(), 4, schedule="refill", max_workgroups=1)   # all of the frame's rays, whatever rows the shard owns
        assert same_bytes(got, want), (name, rank, mismatches(got, want))
        assert sum(r.path_refill_stats()[:2]) == 1 and sum(r.path_launches()) == 0
        r.close()


@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_equality_in_a_new_pose(placement):
    seed = SCENES["mesh"][3]
    scene, moved = moved_mesh()
    rays, s0 = inputs("mesh")
    r = ptss.Renderer(in_place(scene) if placement == "in_place" else scene, W, H, max_iterations=8, seed=seed)
    r.set_camera(camera_of("mesh"))
    assert r.triangle_leaves() > 0
    old = r.trace_paths(rays.copy(), s0.copy(), 8)
    assert same_bytes(r.trace_paths(rays.copy(), s0.copy(), 8, schedule="refill", max_workgroups=1), old)
    r.update_triangles(moved, first=MOVED_FIRST)
    r.resort_triangles()
    assert r.update_rejected() == 0 and r.resort_launches() == 1
    new = r.trace_paths(rays.copy(), s0.copy(), 8)
    assert not np.array_equal(words(new[0]), words(old[0]))
    for cap in (1, 0):
        got = r.trace_paths(rays.copy(), s0.copy(), 8, schedule="refill", max_workgroups=cap)
        assert same_bytes(got, new), (placement, cap, mismatches(got, new))
    r.close()


# ---- 9. the film ----------------------------------------------------------------------------------------------------------------------
def test_a_pinhole_film_with_the_refill_trace_is_the_frame_loop():
    name, iterations = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    f = frames_of(name, iterations)
    r = ptss.Renderer(make_scene(name), W, H, max_iterations=iterations, seed=seed)
    r.set_camera(cam)
    film_cam = ptss.film_camera("pinhole", W, H, cam, jitter=1)
    rng = r.seed_path_rng(N, seed, 0, skip=0)
    film = np.zeros(N, dtype=ptss.FILM_DTYPE)
    for k in range(ROUNDS):
        assert satisfies_identity_condition(f.live_counts[k], iterations), k
        rays, rng = r.generate_rays(film_cam, rng)
        res, rng = r.trace_paths(rays, rng, iterations, schedule="refill", max_workgroups=(1, 0, 5)[k])
        film, pixels, history = r.accumulate_paths(res, film, pixels=True, history=True)
        assert np.array_equal(words(film)[:, :3], f.accum[k]), k
        assert np.array_equal(pixels, f.pixels[k]), k
        assert np.array_equal(words(rng), f.states[k]), k
        r.generate_frame()   # ... and the live context's own frame
        assert np.array_equal(words(film)[:, :3], r.accumulator()) and np.array_equal(pixels, r.pixels()), k
        for p in (0, N // 2 + 7, N - 1):
            assert np.array_equal(r.rng_state(p), words(rng)[p]), (k, p)
    assert sum(r.path_launches()) == 0 and r.path_refill_stats()[:2] == (0, ROUNDS)
    r.close()


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n = 300
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    rays = eye_rays(ptss.default_camera(), 3, 20, 15)
    d_rays, d_rng, d_res = (r._device_buffer(name, size) for name, size in (("t_rays", n * 32 + 16), ("t_rng", n * 24 + 16), ("t_res", n * 16 + 16)))
    ptss._hip_check(Hip.hipMemcpy(d_rays, rays.ctypes.data, n * 32, 1), "hipMemcpy")
    assert L.ptss_seed_path_rng(r._ctx, d_rng, n, 9, 0, 0, None) == 0
    good = ptss.path_options("refill", 1)
    trace = lambda ctx, a, b, c, count, it, o=good: L.ptss_trace_paths_opt(ctx, a, b, c, count, it, C.byref(o) if o is not None else None, None)
    assert trace(r._ctx, d_rays, d_rng, d_res, n, 2) == 0
    stats, launches, kernels = r.path_refill_stats(), r.path_launches(), r.launched_kernels()
    assert stats[:2] == (0, 1) and stats[3] > 0 and launches == (0, 0)

    def snapshot():
        out = [np.empty(n * 24 + 16, np.uint8), np.empty(n * 16 + 16, np.uint8)]
        for host, dev in zip(out, (d_rng, d_res)):
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    # everything ptss_trace_paths refuses
    assert trace(None, d_rays, d_rng, d_res, n, 2) == EINVAL
    for a, b, c in ((None, d_rng, d_res), (d_rays, None, d_res), (d_rays, d_rng, None)):
        assert trace(r._ctx, a, b, c, n, 2) == EINVAL
    for k in (4, 8, 12):
        assert trace(r._ctx, off(d_rays, k), d_rng, d_res, n, 2) == EINVAL, k
        assert trace(r._ctx, d_rays, d_rng, off(d_res, k), n, 2) == EINVAL, k
    for k in (1, 2, 3):
        assert trace(r._ctx, d_rays, off(d_rng, k), d_res, n, 2) == EINVAL, k
    for it in (0, 65, 2 ** 31, 2 ** 32 - 1):
        assert trace(r._ctx, d_rays, d_rng, d_res, n, it) == EINVAL, it
    for count in (2 ** 31, 2 ** 31 + 1, 2 ** 40):
        assert trace(r._ctx, d_rays, d_rng, d_res, count, 2) == ERANGE, count
    # ... and the options'
    assert trace(r._ctx, d_rays, d_rng, d_res, n, 2, None) == EINVAL
    for field, value in (("structSize", 12), ("structSize", 20), ("structSize", 0), ("schedule", 2), ("schedule", -1), ("maxWorkgroups", -1),
                         ("maxWorkgroups", -2 ** 31), ("reserved", 1), ("reserved", -1)):
        for schedule in ("refill", "lane_per_ray"):
            bad = ptss.path_options(schedule, 1)
            setattr(bad, field, value)
            assert trace(r._ctx, d_rays, d_rng, d_res, n, 2, bad) == EINVAL, (field, value, schedule)
            assert trace(r._ctx, None, None, None, 0, 2, bad) == EINVAL, (field, value, schedule)   # with n = 0 as well
    assert trace(r._ctx, None, None, None, 0, 2) == 0   # n = 0
    assert L.ptss_path_refill_stats(None, (C.c_ulonglong * 5)()) == EINVAL and L.ptss_path_refill_stats(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.path_refill_stats() == stats and r.path_launches() == launches and r.launched_kernels() == kernels
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    assert trace(r._ctx, d_rays, off(d_rng, 4), d_res, n, 64, ptss.path_options("refill", 2 ** 31 - 1)) == 0   # all allowed
    r.synchronize()
    assert r.path_refill_stats()[:2] == (0, 2) and r.path_launches() == launches and r.launched_kernels() == kernels
    r.close()
