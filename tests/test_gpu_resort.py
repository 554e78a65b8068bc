"""ptss_resort_triangles: the kd order of a live mesh image rebuilt on the device. The yardsticks are the host
probe of the same rule (ptss.probe_kd_order, csrc/ptorder.h — positions must be EQUAL), the packer (the leaves as sets), the host
refit (bounds, bit for bit), a fresh everySphereLoop context (queries) and the oracle (frames: accumulator, pixels, float sums, live
counts per frame, RNG records). Frames are at most 48 x 32; the oracle's frames of a (size, pose, seed) are computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import ptss
from live_context_common import Subject, above_guard, oracle_snapshot, query_rays, scene as kind_scene, snapshot_equal
from resort_common import leaf_of, mesh_scene, packer_positions, scatter
from scene_update_common import deform, stored

pytestmark = pytest.mark.gpu

SIZES = (512, 777, 5134, 20000)
FRAME = {512: (48, 32), 777: (48, 32), 5134: (32, 24), 20000: (24, 16)}   # the oracle walks every triangle for every ray
BOUNCES, SEED1, SEED2 = 3, 0x5EED, 0xC0FFEE
LIGHT_TRIANGLES = (12, 13)   # the box light of the Cornell preset, part of the mesh (resort_common.table)


@functools.lru_cache(maxsize=None)
def scene_of(T, pose="packed"):
    s = mesh_scene(T)
    return s if pose == "packed" else s.with_triangles(scatter(s.triangles))


@functools.lru_cache(maxsize=None)
def _reference(T, pose, seed, first_tick, frames):
    w, h = FRAME[T]
    o = oracle.Oracle(scene_of(T, pose).desc, w, h, max_iterations=BOUNCES, seed=seed)
    out = []
    try:
        for k in range(frames):
            o.generate_frame(first_tick + k)
            snap = oracle_snapshot(o, w * h, 1)
            for v in snap.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            out.append(snap)
    finally:
        o.close()
    return out


def reference(T, pose, seed, frames, first_tick=1):
    """The oracle's first `frames` frames of a fresh context on that pose, at ticks first_tick, first_tick + 1, ..."""
    return _reference(T, pose, seed, first_tick, 6 if pose == "packed" else 3)[:frames]


def subject(T, **extra):
    """A live context (one per rank) on the packed pose."""
    w, h = FRAME[T]
    return Subject("base", scene_of(T), w, h, BOUNCES, SEED1, **extra)


def frames(sub, want, first_tick, what):
    """Renders len(want) frames and compares every one's live counts, the last one's sums, pixels and RNG records."""
    for k, snap in enumerate(want):
        sub.generate_frame(first_tick + k)
        sub.synchronize()
        assert np.array_equal(sub.live_counts(), snap["live"]), (what, "live counts of frame", first_tick + k)
    snapshot_equal(sub, want[-1], what)


def samples_since_reset(r):
    v = C.c_int()
    assert ptss.device_lib().ptss_samples_since_reset(r._ctx, C.byref(v)) == 0
    return v.value


def positions(sub, T):
    return [r.triangle_positions(T) for r in sub.ranks]


def resort(sub, stream=None):
    for r in sub.ranks:
        r.resort_triangles(stream=stream)


# ---- the unchanged pose ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SIZES)
def test_unchanged_pose_renders_on_and_stores_the_probes_order(T):
    scene = scene_of(T)
    want = reference(T, "packed", SEED1, 6)
    w, h = FRAME[T]
    rays = query_rays(scene.triangles, w, h)
    prev = deform(scene.triangles, 0.3)
    sub = subject(T)
    try:
        r = sub.ranks[0]
        assert np.array_equal(r.triangle_positions(T), packer_positions(scene))
        frames(sub, want[:3], 1, "before the re-sort")
        hits, shadows, feats = r.intersect(rays).tobytes(), r.occluded(rays).tobytes(), r.features().tobytes()
        motion = [a.tobytes() for a in r.features_motion(prev)]
        kernels, held = r.launched_kernels(), samples_since_reset(r)
        assert r.resort_launches() == 0
        r.resort_triangles()
        pos = r.triangle_positions(T)
        assert np.array_equal(pos, ptss.probe_kd_order(scene.triangles))
        assert np.array_equal(leaf_of(pos), leaf_of(packer_positions(scene)))
        assert r.resort_launches() == 1 and r.launched_kernels() - kernels <= {("refit",)} and ("refit",) in r.launched_kernels()
        assert samples_since_reset(r) == held   # no reset
        assert r.intersect(rays).tobytes() == hits and r.occluded(rays).tobytes() == shadows
        assert r.features().tobytes() == feats
        assert [a.tobytes() for a in r.features_motion(prev)] == motion
        bounds = r.triangle_bounds()
        order = np.empty(T, dtype=np.int64)
        order[pos] = np.arange(T)
        assert np.array_equal(bounds.view(np.uint32), ptss.probe_mesh_refit(stored(scene.triangles)[order]).view(np.uint32))
        frames(sub, want[3:], 4, "behind the re-sort")   # the accumulation continues: six frames of one oracle
        assert samples_since_reset(r) > held
        r.resort_triangles()                              # a second call changes nothing
        assert np.array_equal(r.triangle_positions(T), pos) and r.triangle_bounds().tobytes() == bounds.tobytes()
        assert r.resort_launches() == 2
        assert r.intersect(rays).tobytes() == hits
    finally:
        sub.close()


# ---- a pose that scatters every triangle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", SIZES)
def test_scattered_pose(T):
    scene, moved = scene_of(T), scene_of(T, "scattered")
    new = moved.triangles
    w, h = FRAME[T]
    sub = subject(T)
    try:
        r = sub.ranks[0]
        r.generate_frame()
        before = r.triangle_positions(T)
        r.update_triangles(new)
        assert np.array_equal(r.triangle_positions(T), before)   # the update keeps the order ...
        r.resort_triangles()
        pos = r.triangle_positions(T)
        assert np.array_equal(pos, ptss.probe_kd_order(new))     # ... the re-sort rebuilds it
        assert np.array_equal(leaf_of(pos), leaf_of(packer_positions(moved)))
        assert not np.array_equal(leaf_of(pos), leaf_of(before))
        order = np.empty(T, dtype=np.int64)
        order[pos] = np.arange(T)
        assert np.array_equal(r.triangle_bounds().view(np.uint32), ptss.probe_mesh_refit(stored(new)[order]).view(np.uint32))
        assert r.update_rejected() == 0
        rays = query_rays(new, w, h)
        fresh = ptss.Renderer(moved, w, h, max_iterations=BOUNCES, every_sphere_loop=True)
        try:
            assert r.intersect(rays).tobytes() == fresh.intersect(rays).tobytes()
            assert np.array_equal(r.occluded(rays), fresh.occluded(rays))
        finally:
            fresh.close()
        sub.reseed(SEED2)
        frames(sub, reference(T, "scattered", SEED2, 3, first_tick=2), 2, "the scattered pose, re-sorted")
    finally:
        sub.close()


def test_area_lights_follow_their_triangles():
    """The box light's two triangles belong to the mesh; the area-light row names them by stored position."""
    T = 777
    moved = scene_of(T, "scattered")
    sub = subject(T)
    try:
        r = sub.ranks[0]
        r.generate_frame()
        r.update_triangles(moved.triangles)
        before = r.triangle_positions(T)[list(LIGHT_TRIANGLES)]
        r.resort_triangles()
        after = r.triangle_positions(T)[list(LIGHT_TRIANGLES)]
        assert before[0] != after[0] and before[1] != after[1], "the pose must move the light's triangles in the stored order"
        sub.reseed(SEED2)
        frames(sub, reference(T, "scattered", SEED2, 3, first_tick=2), 2, "the light's triangles at new positions")
    finally:
        sub.close()


def test_a_refused_record_is_sorted_by_the_geometry_it_kept():
    T = 777
    scene = scene_of(T)
    new = scatter(scene.triangles)
    effective = new.copy()
    effective[100] = scene.triangles[100]
    new["vertex1"][100, 1] = np.nan
    sub = subject(T)
    try:
        r = sub.ranks[0]
        r.update_triangles(new)
        r.resort_triangles()
        assert r.update_rejected() == 1
        pos = r.triangle_positions(T)
        assert np.array_equal(pos, ptss.probe_kd_order(effective))
        w, h = FRAME[T]
        rays = query_rays(effective, w, h)
        fresh = ptss.Renderer(scene.with_triangles(effective), w, h, max_iterations=BOUNCES, every_sphere_loop=True)
        try:
            assert r.intersect(rays).tobytes() == fresh.intersect(rays).tobytes()
        finally:
            fresh.close()
    finally:
        sub.close()


# ---- other configurations ---------------------------------------------------------------------------------------------------------
def test_on_a_callers_stream():
    torch = pytest.importorskip("torch")
    T = 777
    want = reference(T, "packed", SEED1, 6)
    sub = subject(T)
    try:
        r = sub.ranks[0]
        frames(sub, want[:3], 1, "before the re-sort")
        side = torch.cuda.Stream()
        r.synchronize()                                   # the caller orders the call behind the frames ...
        r.resort_triangles(stream=side.cuda_stream)
        assert np.array_equal(r.triangle_positions(T), ptss.probe_kd_order(scene_of(T).triangles))   # (the read-back waits for `side`)
        side.synchronize()                                # ... and the next frame behind the call
        frames(sub, want[3:], 4, "behind a re-sort on a side stream")
    finally:
        sub.close()


def test_two_shards():
    T = 777
    want = reference(T, "packed", SEED1, 6)
    assert all(above_guard(s["live"]) for s in want), "shards and oracle agree only while the frame-wide live count stays above 128"
    sub = subject(T, tile_world=2, band_rows=4)
    try:
        frames(sub, want[:3], 1, "two shards before the re-sort")
        resort(sub)
        probe = ptss.probe_kd_order(scene_of(T).triangles)
        assert all(np.array_equal(p, probe) for p in positions(sub, T))
        frames(sub, want[3:], 4, "two shards behind the re-sort")
    finally:
        sub.close()


def test_two_free_running_lanes():
    T = 777
    want = reference(T, "packed", SEED1, 6)
    sub = subject(T, frame_lanes=2, lanes_free_run=True)
    try:
        frames(sub, want[:3], 1, "two lanes before the re-sort")
        sub.synchronize()
        resort(sub)
        frames(sub, want[3:], 4, "two lanes behind the re-sort")
        assert sub.guard_timeouts() == 0
        assert np.array_equal(positions(sub, T)[0], ptss.probe_kd_order(scene_of(T).triangles))
    finally:
        sub.close()


# ---- images without a kd order ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bounded_padded", "bounded", "accel_300", "every_sphere_loop"])
def test_images_without_a_kd_order_are_left_alone(kind):
    """Plain (484 triangles), edge-classed, many-sphere (two images), and a mesh-sized scene under everySphereLoop."""
    if kind == "every_sphere_loop":
        scene, extra = scene_of(512), dict(every_sphere_loop=True)
    else:
        scene, extra = kind_scene(kind), {}
    if kind == "bounded_padded":
        assert scene.desc.numTriangles == 484
    r = ptss.Renderer(scene, 32, 24, max_iterations=2, **extra)
    try:
        r.generate_frame()
        kernels, acc = r.launched_kernels(), r.accumulator()
        assert r.triangle_leaves() == 0
        assert ptss.device_lib().ptss_resort_triangles(r._ctx, None) == 0
        assert r.resort_launches() == 0 and r.launched_kernels() == kernels
        assert np.array_equal(r.accumulator(), acc)
    finally:
        r.close()


def test_a_null_context_is_refused():
    L = ptss.device_lib()
    assert L.ptss_resort_triangles(None, None) == -1                       # PTSS_EINVAL
    assert L.ptss_resort_launches(None, C.byref(C.c_ulonglong())) == -1
