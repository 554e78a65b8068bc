"""Batched path queries on the GPU (ptss_seed_path_rng / ptss_trace_paths).

1. The frame identity, the main pin: fed a frame's own eye rays (ptss_camera_ray with the pixel's two jitter draws) and streams
   (ptss_seed_path_rng(seed, 0, skip 2) in pixel order) the query returns the oracle's radiance0 of that frame, the oracle's final
   stream states and as many entered iterations as the oracle's live counts add up to — and what the GPU context's own first frame
   left in its float accumulator — bit for bit, for eight scenes, maxIterations 1, 2, 4, 8, the image staged in LDS and read in place.
2. One iteration on arbitrary rays against the oracle's closest hit and shade().
3. Seeding. 4. Continuation and order independence. 5. No trace in frame state; sharded contexts. 6. Refusals.
7. The identity again after ptss_update_triangles + ptss_resort_triangles on the mesh scene.
The cases (tests/path_query_common.py) all keep the frame's loop guard silent, which tests/test_path_query_cpu.py checks."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
import refprobe
from path_query_common import (H, ITERATIONS, MOVED_FIRST, N, SCENES, W, camera_of, expected, expected_moved, eye_rays, in_place, make_scene, moved_mesh,
                               satisfies_identity_condition)
from test_gpu_edge_scenes import COOK, CREAM, FLOOR, GLASS, GREEN, LAMP, MIRROR, PHONG, RED, build
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


def words(a):
    """The 32-bit words of a record or float array, one row per entry."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def same_radiance(a, b):
    """Equal float32 words, NaN against NaN (x86 and gfx950 make different default NaNs)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return bool((np.isnan(a) | (a.view(np.uint32) == b.view(np.uint32))).all())


def check_identity(r, e, rays, seed, iterations, what):
    """Test 1's identity for one renderer and one maxIterations: the oracle's frame `e`, then the context's own first frame."""
    s0 = r.seed_path_rng(N, seed, 0, skip=2)
    res, after = r.trace_paths(rays, s0, iterations)
    assert satisfies_identity_condition(e.live_counts, iterations), what
    assert np.array_equal(res["radiance"], e.radiance, equal_nan=True), (what, int((res["radiance"] != e.radiance).sum()))
    assert same_radiance(res["radiance"], e.radiance), what
    assert np.array_equal(words(after), e.states), (what, int((words(after) != e.states).any(axis=1).sum()))
    assert int(res["bounces"].sum()) == int(e.live_counts.sum()), what
    assert res["bounces"].min() >= 1 and res["bounces"].max() <= iterations
    r.set_max_iterations(iterations)
    r.reseed(seed)   # the context's streams as created, and a reset: the next frame is a first frame
    r.generate_frame()
    assert np.array_equal(r.live_counts(), e.live_counts), what
    assert np.array_equal(res["radiance"], r.float_accumulator(), equal_nan=True), what
    for p in (0, N // 2 + 7, N - 1):
        assert np.array_equal(r.rng_state(p), words(after)[p]), (what, p)
    return res, after


# ---- 1. the frame identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
@pytest.mark.parametrize("name", list(SCENES))
def test_frame_identity(name, placement):
    _, every, _, seed = SCENES[name]
    scene, cam = make_scene(name, placement), camera_of(name)
    r = ptss.Renderer(scene, W, H, max_iterations=8, seed=seed, float_accumulator=True, every_sphere_loop=every)
    r.set_camera(cam)
    rays = eye_rays(cam, seed)
    rays[:, 3] = np.float32(0.5)   # tmax is ignored: a path starts at distance +inf
    for iterations in ITERATIONS:
        check_identity(r, expected(name, iterations), rays, seed, iterations, (name, placement, iterations))
    launches = r.path_launches()
    assert launches == ((0, len(ITERATIONS)) if placement == "lds" else (len(ITERATIONS), 0)), (name, placement, launches)
    r.close()


# ---- 2. one iteration on arbitrary rays ------------------------------------------------------------------------------------------------
def open_scene():
    """Spheres of every material class on a floor under a lamp, an area light and a point light; nothing around them: rays from outside
    hit spheres, hit triangles, or miss."""
    spheres = [((0, 0, -3), 0.8, COOK), ((-1.6, -0.2, -4), 0.7, GLASS), ((1.5, 0.1, -3.5), 0.6, MIRROR), ((0.6, 0.9, -5), 0.5, PHONG),
               ((-1.8, -0.3, -6.2), 0.7, CREAM), ((0.1, -0.4, -6.4), 0.6, RED), ((2.2, -0.2, -5.6), 0.8, GREEN)]
    s = build(spheres=spheres, triangles=FLOOR + LAMP, area=[((50, 50, 50), 2)], point=[((-2.5, 2.0, -2.0), (30, 30, 30))])
    s.desc.defaultColor.x, s.desc.defaultColor.y, s.desc.defaultColor.z = 0.25, 0.5, 0.125
    return s


def outside_rays(n, seed=5):
    """n rays from a shell above the floor around the geometry, towards a box somewhat larger than it: towards it and past it."""
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.15
    o = np.array([0.0, 0.5, -4.5]) + 14.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    target = g.uniform([-4.5, -1.0, -9.5], [4.5, 3.5, 0.5], size=(n, 3))
    target[: n // 3, 1] = -1.0   # a third aims at the floor's plane
    v = target - o
    return ptss.make_rays(o, v / np.linalg.norm(v, axis=1, keepdims=True), INF)


@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_one_iteration_is_closest_hit_plus_shade(placement):
    n, seed = 4096, 0xC0FFEE
    scene = open_scene()
    rays = outside_rays(n)
    P = refprobe.Probes("oracle")
    P.use_scene(scene.desc)
    rays6 = np.concatenate([rays[:, 0:3], rays[:, 4:7]], axis=1)
    kind, _, hit = P.closest_hit(rays6, INF)
    point, normal, mat = hit[:, 1:4], hit[:, 4:7], np.where(kind != 0, hit[:, 7].astype(np.int32), 0)
    shade, state6 = P.shade(point, normal, mat, seed)   # entry i draws from stream curand_init(seed, i, 0)
    P.close()
    cos_i = -(rays[:, 4:7].astype(np.float64) * normal.astype(np.float64)).sum(axis=1)
    miss, front = kind == 0, (kind != 0) & (cos_i > 1e-3)
    # the rays were chosen so that the comparison means something
    assert miss.sum() + front.sum() >= n // 2 and miss.sum() > 100 and (front & (kind == 1)).sum() > 100 and (front & (kind == 2)).sum() > 100

    r = ptss.Renderer(in_place(scene) if placement == "in_place" else scene, 16, 16, max_iterations=3)
    s0 = r.seed_path_rng(n, seed, 0, 0)
    res, after = r.trace_paths(rays, s0, 1)
    r.close()
    default = np.array([0.25, 0.5, 0.125], dtype=np.float32)
    assert np.array_equal(words(res["radiance"][miss]), words(np.broadcast_to(default, (int(miss.sum()), 3))))
    assert np.array_equal(words(after)[miss], words(s0)[miss])   # a miss draws nothing
    emit = np.array([[m.emmitance.x, m.emmitance.y, m.emmitance.z] for m in (scene.desc.materials[int(k)] for k in mat)], dtype=np.float32)
    want = (np.float32(0) + emit) + shade   # float32, in the thread body's order
    assert want.dtype == np.float32
    assert np.array_equal(words(res["radiance"][front]), words(want[front])), int((words(res["radiance"]) != words(want)).any(axis=1)[front].sum())
    assert np.array_equal(words(after)[front], state6[front])
    assert (res["bounces"] == 1).all()
    assert (shade[front] != 0).any(axis=1).sum() > 100   # lit surfaces among them: the shadow tests took part


# ---- 3. seeding ------------------------------------------------------------------------------------------------------------------------
def advance(state6, draws):
    """`draws` draws of the product's host XORWOW (ptss_probe_rng_draw) from state6 -> (the state afterwards, the uniforms)."""
    s = np.array(state6, dtype=np.uint32)
    raw, uni = np.zeros(max(draws, 1), np.uint32), np.zeros(max(draws, 1), np.float32)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    assert ptss.host_lib().ptss_probe_rng_draw(s.ctypes.data_as(u32p), raw.ctypes.data_as(u32p), uni.ctypes.data_as(f32p), draws) == 0
    return s, uni[:draws]


def test_seeding():
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    seed = 0x0123456789ABCDEF
    for s in (0, 1, 2 ** 31, 2 ** 32 - 1):
        got = words(r.seed_path_rng(1, seed, first_sequence=s, skip=0))[0]
        assert np.array_equal(got, oracle.probe_rng(seed, s, 0)[0]), s
        for skip in (1, 2, 64):   # skip draws, one by one
            want, uni = advance(got, skip)
            assert np.array_equal(words(r.seed_path_rng(1, seed, first_sequence=s, skip=skip))[0], want), (s, skip)
            if skip == 2:
                assert np.array_equal(uni, oracle.probe_rng(seed, s, 2)[2]), s   # ... which are the oracle's draws
    whole = r.seed_path_rng(1000, seed)   # four blocks, the last one partly filled
    for k in (1, 255, 256, 777):
        assert np.array_equal(words(r.seed_path_rng(1000 - k, seed, first_sequence=k)), words(whole)[k:]), k
    assert np.array_equal(words(whole)[:3], np.array([oracle.probe_rng(seed, s, 0)[0] for s in range(3)]))
    top = r.seed_path_rng(5, 77, first_sequence=2 ** 32 - 5)   # firstSequence + n = 2^32 exactly
    assert np.array_equal(words(top)[4], oracle.probe_rng(77, 2 ** 32 - 1, 0)[0])
    assert len(r.seed_path_rng(0, seed)) == 0
    assert r.path_launches() == (0, 0)
    r.close()


# ---- 4. continuation, order independence -----------------------------------------------------------------------------------------------
def test_continuation_and_order_independence():
    torch = pytest.importorskip("torch")
    name = "mixed"
    seed, cam = SCENES[name][3], camera_of(name)
    r = ptss.Renderer(make_scene(name), W, H, max_iterations=4, seed=seed)
    rays = eye_rays(cam, seed)
    s0 = r.seed_path_rng(N, seed, 0, skip=2)
    res1, s1 = r.trace_paths(rays, s0, 4)
    res2, s2 = r.trace_paths(rays, s1, 4)
    assert not np.array_equal(words(s1), words(s2)) and not np.array_equal(res1["radiance"], res2["radiance"])
    # the same two calls with the states carried on the device
    d_rays = torch.from_numpy(rays).cuda()
    d_rng = r.seed_path_rng(N, seed, 0, skip=2, device=True)
    assert np.array_equal(d_rng.cpu().numpy().view(np.uint32), words(s0))
    first = r.trace_paths(d_rays, d_rng, 4)
    second = r.trace_paths(d_rays, d_rng, 4)
    torch.cuda.synchronize()
    for got, want in ((first, res1), (second, res2)):
        got = got.cpu().numpy()
        assert same_radiance(got[:, :3], want["radiance"]) and np.array_equal(got[:, 3].view(np.uint32), want["bounces"])
    assert np.array_equal(d_rng.cpu().numpy().view(np.uint32), words(s2))
    # a permuted batch gives permuted results
    perm = np.random.default_rng(1).permutation(N)
    res_p, s_p = r.trace_paths(rays[perm], s0[perm], 4)
    assert same_radiance(res_p["radiance"], res1["radiance"][perm]) and np.array_equal(res_p["bounces"], res1["bounces"][perm])
    assert np.array_equal(words(s_p), words(s1)[perm])
    # ... and so does a part of the batch that ends inside a wave
    res_h, s_h = r.trace_paths(rays[:1001], s0[:1001], 4)
    assert same_radiance(res_h["radiance"], res1["radiance"][:1001]) and np.array_equal(words(s_h), words(s1)[:1001])
    r.close()


# ---- 5. no trace in frame state; sharded contexts -----------------------------------------------------------------------------------------
def test_frames_are_untouched():
    torch = pytest.importorskip("torch")
    name, bounces = "mixed", 4
    seed, cam = SCENES[name][3], camera_of(name)
    scene = make_scene(name)
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)
    twin = ptss.Renderer(scene, W, H, max_iterations=bounces, seed=seed, float_accumulator=True)   # frames only
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, seed=seed)
    rays = eye_rays(cam, seed)
    s0 = r.seed_path_rng(N, seed, 0, skip=2)
    want, _ = r.trace_paths(rays, s0, bounces)   # before the first frame: 1 launch
    side = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays).cuda()
    for tick in range(20):
        r.generate_frame()
        twin.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        got, _ = r.trace_paths(rays, s0, bounces)   # on the context's stream
        assert same_radiance(got["radiance"], want["radiance"]), tick
        with torch.cuda.stream(side):   # and on a second one
            d_rng = torch.from_numpy(words(s0).view(np.int32).copy()).cuda()
            d_res = r.trace_paths(d_rays, d_rng, bounces)
        side.synchronize()
        assert same_radiance(d_res.cpu().numpy()[:, :3], want["radiance"]), tick
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, "twenty frames with two path queries after each", W, H, 1)
    assert r.launched_kernels() == twin.launched_kernels()   # what the frames alone set
    assert r.path_launches() == (0, 1 + 2 * 20) and twin.path_launches() == (0, 0)
    twin.close()
    o.close()
    r.close()


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_a_sharded_context_answers_as_the_unsharded_one(name):
    _, every, _, seed = SCENES[name]
    scene, cam = make_scene(name), camera_of(name)
    rays = eye_rays(cam, seed)
    e = expected(name, 4)
    for rank in range(2):
        r = ptss.Renderer(scene, W, H, max_iterations=4, seed=seed, tile_rank=rank, tile_world=2, band_rows=8, every_sphere_loop=every)
        res, after = r.trace_paths(rays, r.seed_path_rng(N, seed, 0, skip=2), 4)   # all of the frame's rays, whatever rows the shard owns
        assert np.array_equal(res["radiance"], e.radiance, equal_nan=True) and np.array_equal(words(after), e.states), (name, rank)
        assert sum(r.path_launches()) == 1
        r.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter_and_touch_no_buffer():
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    EINVAL, ERANGE = -1, -5
    n = 300
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    rays = eye_rays(ptss.default_camera(), 3, 20, 15)
    d_rays, d_rng, d_res = (r._device_buffer(name, size) for name, size in (("t_rays", n * 32 + 16), ("t_rng", n * 24 + 16), ("t_res", n * 16 + 16)))
    ptss._hip_check(Hip.hipMemcpy(d_rays, rays.ctypes.data, n * 32, 1), "hipMemcpy")
    assert L.ptss_seed_path_rng(r._ctx, d_rng, n, 9, 0, 0, None) == 0
    assert L.ptss_trace_paths(r._ctx, d_rays, d_rng, d_res, n, 2, None) == 0
    r.synchronize()
    counters, kernels = r.path_launches(), r.launched_kernels()
    assert counters == (0, 1)

    def snapshot():
        out = [np.empty(n * 24 + 16, np.uint8), np.empty(n * 16 + 16, np.uint8)]
        for host, dev in zip(out, (d_rng, d_res)):
            ptss._hip_check(Hip.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2), "hipMemcpy")
        return out

    before = snapshot()
    off = lambda p, k: C.c_void_p(p.value + k)
    trace = lambda ctx, a, b, c, count, it: L.ptss_trace_paths(ctx, a, b, c, count, it, None)
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
    assert trace(r._ctx, None, None, None, 0, 2) == 0   # n = 0

    seed = lambda ctx, p, count, first, skip: L.ptss_seed_path_rng(ctx, p, count, 9, first, skip, None)
    assert seed(None, d_rng, n, 0, 0) == EINVAL
    assert seed(r._ctx, None, n, 0, 0) == EINVAL
    for k in (1, 2, 3):
        assert seed(r._ctx, off(d_rng, k), n, 0, 0) == EINVAL, k
    for skip in (65, 2 ** 32 - 1):
        assert seed(r._ctx, d_rng, n, 0, skip) == EINVAL, skip
    assert seed(r._ctx, d_rng, 2 ** 31, 0, 0) == ERANGE
    for first, count in ((2 ** 32 - n + 1, n), (2 ** 32, 1), (2 ** 64 - 1, 2), (2 ** 32 - 1, 2)):
        assert seed(r._ctx, d_rng, count, first, 0) == ERANGE, (first, count)
    assert seed(r._ctx, None, 0, 0, 0) == 0   # n = 0
    out2 = (C.c_ulonglong * 2)()
    assert L.ptss_path_launches(None, out2) == EINVAL and L.ptss_path_launches(r._ctx, None) == EINVAL

    r.synchronize()
    assert r.path_launches() == counters and r.launched_kernels() == kernels
    for a, b in zip(before, snapshot()):
        assert np.array_equal(a, b)
    assert trace(r._ctx, d_rays, d_rng, d_res, n, 64) == 0   # 64 is allowed; a 4-byte aligned dev_rng is
    assert seed(r._ctx, off(d_rng, 4), n, 2 ** 32 - n, 64) == 0
    r.synchronize()
    assert r.path_launches() == (0, 2) and r.launched_kernels() == kernels
    r.close()


# ---- 7. after ptss_update_triangles + ptss_resort_triangles ---------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["lds", "in_place"])
def test_identity_in_a_new_pose(placement):
    seed, cam = SCENES["mesh"][3], camera_of("mesh")
    scene, moved = moved_mesh()
    r = ptss.Renderer(in_place(scene) if placement == "in_place" else scene, W, H, max_iterations=8, seed=seed, float_accumulator=True)
    r.set_camera(cam)
    rays = eye_rays(cam, seed)
    assert r.triangle_leaves() > 0
    check_identity(r, expected("mesh", 4), rays, seed, 4, ("old pose", placement))
    r.update_triangles(moved, first=MOVED_FIRST)
    r.resort_triangles()
    assert r.update_rejected() == 0 and r.resort_launches() == 1
    for iterations in ITERATIONS:
        check_identity(r, expected_moved(iterations), rays, seed, iterations, ("new pose", placement, iterations))
    r.close()
