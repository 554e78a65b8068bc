"""Per-pixel motion and reprojection across moving triangles on the GPU (ptss_render_features_motion / ptss_reproject_motion;
DESIGN.md §3.20).

The features of the new call against ptss_render_features, byte for byte; its motion rows against the composition ptss_intersect
of every pixel-centre ray -> ptss_probe_motion (the host build of csrc/ptmotion.h), all four words; ptss_reproject_motion against
ptss_probe_reproject_motion on the read-back inputs, all four floats; with nothing moved, against ptss_reproject; frames untouched
by the three calls; bits 58/59 and 60 of ptss_launched_kernels; the refusals; and the point of it: after a mesh has moved, the first
frame merged with the history that followed the mesh is strictly closer to the converged image than that frame alone, over the
whole image and over the moved surface. The figures the last test prints are the ones quoted in DESIGN.md §3.20."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
from ptss_types import SURFACE_TRIANGLE, Triangle
from scene_update_common import GREEN, TableScene, grid_triangles, preset_triangles, triangles_of
from test_gpu_denoise import SCENE_MAKERS, far_camera, inverse_ticks, moved_camera, mse
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (250, 130)]


def grid_512():
    """A 16 x 16 grid of 512 triangles facing the camera, the smallest mesh image, before the spheres of the cornell preset."""
    return TableScene(grid_triangles((-3.0, -2.5, -6.0), (6.0, 0.0, 0.0), (0.0, 5.0, -0.8), 16, 16, GREEN))


SCENES = {"mixed": SCENE_MAKERS["mixed"], "in_place_484": SCENE_MAKERS["in_place_484"], "grid_512": grid_512}
UPDATABLE = {"in_place_484", "grid_512"}   # mixed stores its 16 triangles by edge class: ptss_update_triangles refuses it


def table_of(desc):
    return np.frombuffer(C.string_at(desc.triangles, desc.numTriangles * C.sizeof(Triangle)), dtype=ptss.TRIANGLE_DTYPE).copy()


def nudged(t, amount):
    """Another pose of a table: every vertex displaced by a smooth field of size `amount` (shared vertices stay shared)."""
    out = t.copy()
    for name in ("vertex0", "vertex1", "vertex2"):
        p = t[name].astype(np.float64)
        field = np.stack([np.sin(2.0 * p[:, 1] + 0.3), 0.5 * np.sin(3.0 * p[:, 0]), 0.3 * np.sin(p[:, 0] + p[:, 2])], axis=1)
        out[name] = (p + amount * field).astype(np.float32)
    return out


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


def triangle_ids(motion):
    s = motion["surface"]
    return s[(s >= SURFACE_TRIANGLE)] - SURFACE_TRIANGLE


def check(r, cam, w, h, T, prev, first, what, rows=None):
    """One ptss_render_features_motion: features = ptss_render_features, motion = ptss_intersect -> ptss_probe_motion."""
    feat, mot = r.features_motion(prev, first=first)
    assert same_bits(feat, r.features()), (what, "features")
    rays = ptss.camera_rays(cam, w, h)
    if rows is not None:
        rays = rays.reshape(h, w, 8)[rows].reshape(-1, 8)
    hits = r.intersect(rays)
    want = ptss.probe_motion(rays, hits, prev, first=first, num_triangles=T)
    assert same_bits(mot, want), (what, "motion", int((mot.view(np.uint32) != want.view(np.uint32)).sum()))
    assert ((mot["surface"] >= 0) == (feat["materialIdx"] >= 0)).all(), what
    return feat, mot, rays, hits


# ---- features equal, motion equals the composition --------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_features_are_equal_and_motion_is_the_composition(name, w, h, S):
    scene = SCENES[name]()
    T = scene.desc.numTriangles
    pose_a = table_of(scene.desc)
    r = ptss.Renderer(scene, w, h, max_iterations=2, samples_per_pass=S)
    cam = moved_camera() if name != "in_place_484" else ptss.default_camera()   # (the wall of 480 triangles lies ahead of the default pose)
    r.set_camera(cam)
    assert not r.launched_kernels() & ptss.motion_kernels()
    # nothing moved: count = 0 with a NULL pointer
    _, still, rays, hits = check(r, cam, w, h, T, None, 0, (name, "count = 0"))
    hit_ids = np.unique(triangle_ids(still))
    assert len(hit_ids) >= 3, name
    static_points = still["prevPoint"].copy()
    # the whole mesh has moved
    if name in UPDATABLE:
        pose_b = nudged(pose_a, 0.05)
        r.update_triangles(pose_b)
    else:
        pose_b, pose_a = pose_a, nudged(pose_a, 0.05)   # (no update of an edge-classed image: the previous pose is what differs)
    _, moved, _, hits = check(r, cam, w, h, T, pose_a, 0, (name, "whole mesh"))
    on_triangle = moved["surface"] >= SURFACE_TRIANGLE
    assert on_triangle.sum() > 0.1 * w * h
    here = ptss.probe_motion(rays, hits, None)["prevPoint"]
    assert (np.abs(moved["prevPoint"][on_triangle] - here[on_triangle]).max(axis=1) > 1e-4).mean() > 0.9   # they did move ...
    assert same_bits(moved["prevPoint"][~on_triangle], here[~on_triangle])                              # ... and nothing else
    if name not in UPDATABLE:
        assert same_bits(here, static_points)
    # a sub-range with hit triangles below, inside and above it
    hit_ids = np.unique(triangle_ids(moved))
    assert len(hit_ids) >= 3, name
    k = len(hit_ids) // 3
    first, last = int(hit_ids[k]), int(hit_ids[max(k, (2 * len(hit_ids)) // 3 - 1)])
    assert hit_ids[0] < first <= last < hit_ids[-1]
    _, part, _, _ = check(r, cam, w, h, T, pose_a[first:last + 1], first, (name, "sub-range"))
    ids = part["surface"] - SURFACE_TRIANGLE
    inside = on_triangle & (ids >= first) & (ids <= last)
    assert inside.any() and (on_triangle & (ids < first)).any() and (on_triangle & (ids > last)).any()   # both sides of both boundaries
    assert same_bits(part["prevPoint"][inside], moved["prevPoint"][inside]) and same_bits(part["prevPoint"][~inside], here[~inside])
    # one refused record: its triangle counts as static
    refused = pose_a.copy()
    victim = int(hit_ids[len(hit_ids) // 2])
    refused["vertex1"][victim, 1] = np.inf
    _, odd, _, _ = check(r, cam, w, h, T, refused, 0, (name, "a refused record"))
    on_victim = odd["surface"] == (SURFACE_TRIANGLE | victim)
    assert on_victim.any() and same_bits(odd["prevPoint"][on_victim], here[on_victim])
    assert same_bits(odd["prevPoint"][~on_victim], moved["prevPoint"][~on_victim])
    # a camera beyond 1e15
    far = far_camera()
    r.set_camera(far)
    check(r, far, w, h, T, pose_a, 0, (name, "camera beyond 1e15"))
    lds = {k[1] for k in r.launched_kernels() if k[0] == "features"}
    assert r.launched_kernels() & ptss.motion_kernels() == {("features_motion", l) for l in lds} and len(lds) == 1
    if name == "in_place_484":
        assert lds == {False}
    if name == "mixed":
        assert lds == {True}
    r.close()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_pixel_band_shard_is_served_for_its_own_pixels(name):
    scene = SCENES[name]()
    T = scene.desc.numTriangles
    pose_a = nudged(table_of(scene.desc), 0.05)
    w, h = 40, 36
    cam = moved_camera() if name != "in_place_484" else ptss.default_camera()
    seen = []
    for rank in range(2):
        r = ptss.Renderer(scene, w, h, max_iterations=2, tile_rank=rank, tile_world=2, band_rows=8)
        r.set_camera(cam)
        rows = r.rows()
        seen += rows.tolist()
        check(r, cam, w, h, T, pose_a, 0, (name, "shard", rank), rows=rows)
        check(r, cam, w, h, T, pose_a[T // 4:], T // 4, (name, "shard", rank, "sub-range"), rows=rows)
        with pytest.raises(ptss.PtssError, match="shard"):
            r.reproject(motion=True)
        assert ("reproject_motion",) not in r.launched_kernels()
        r.close()
    assert sorted(seen) == list(range(h))


# ---- ptss_reproject_motion: device = host --------------------------------------------------------------------------------------
def step(r, frames):
    for _ in range(frames):
        r.generate_frame()
    return r.accumulator()


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_reproject_motion_equals_the_host_build(name, w, h, S):
    scene = SCENES[name]()
    poses = [table_of(scene.desc)]
    poses += [nudged(poses[0], 0.04), nudged(poses[0], 0.09)]
    r = ptss.Renderer(scene, w, h, max_iterations=4, samples_per_pass=S)
    p = ptss.default_reproject_params()
    cam0 = moved_camera() if name != "in_place_484" else ptss.default_camera()
    r.set_camera(cam0)

    def move_to(k):
        """Pose k becomes the scene's (where the image can be updated in place) -> the previous pose's records."""
        if name in UPDATABLE:
            r.update_triangles(poses[k])
            return poses[k - 1]
        return poses[k]   # an edge-classed image keeps its geometry: any other table serves as "the previous pose"

    # three frames at pose 0 become the history
    acc0 = step(r, 3)
    f0, m0 = r.features_motion()
    h0 = r.reproject(motion=True)
    assert same_bits(h0, ptss.probe_reproject_motion(acc0, inverse_ticks(S, 3), 3 * S, cam0, None, w, h, f0, m0, None, None, p)), "no history"
    assert (h0["weight"] == 3 * S).all()
    # the mesh moves, the camera stands still; one frame
    prev = move_to(1)
    acc1 = step(r, 1)
    frames = 1 if name in UPDATABLE else 4   # an update resets the accumulation; without one the fourth frame joins the three
    f1, m1 = r.features_motion(prev)
    h1 = r.reproject(prev_camera=cam0, prev_features=f0, prev_history=h0, motion=True)
    want = ptss.probe_reproject_motion(acc1, inverse_ticks(S, frames), frames * S, cam0, cam0, w, h, f1, m1, f0, h0, p)
    assert same_bits(h1, want), (name, w, h, S, "mesh moved", int((h1.view(np.uint32) != want.view(np.uint32)).sum()))
    assert (h1["weight"] > frames * S).mean() > 0.2                                # the history did arrive ...
    on_moved = m1["surface"] >= SURFACE_TRIANGLE
    assert (h1["weight"][on_moved] > frames * S).any()                             # ... on the moved surface too
    # both move: a reprojected history is itself reprojected; two frames
    prev = move_to(2)
    cam2 = type(cam0).from_buffer_copy(cam0)
    for k in "ag":
        ptss.move_camera(cam2, k)
    r.set_camera(cam2)
    acc2 = step(r, 2)
    f2, m2 = r.features_motion(prev)
    h2 = r.reproject(prev_camera=cam0, prev_features=f1, prev_history=h1, motion=True)
    want = ptss.probe_reproject_motion(acc2, inverse_ticks(S, 2), 2 * S, cam2, cam0, w, h, f2, m2, f1, h1, p)
    assert same_bits(h2, want), (name, w, h, S, "both moved")
    assert (h2["weight"] > 3 * S).any()   # weight that has travelled through both steps
    # nothing moved: ptss_reproject_motion is ptss_reproject, bit for bit
    f3, m3 = r.features_motion()
    assert same_bits(f3, f2)
    with_rows = r.reproject(prev_camera=cam0, prev_features=f1, prev_history=h1, motion=True, dev_out=r.history_devptr(2))
    without = r.reproject(prev_camera=cam0, prev_features=f1, prev_history=h1)
    assert same_bits(with_rows, without), (name, w, h, S, "static identity")
    assert (without["weight"] > 2 * S).any()
    assert ("reproject_motion",) in r.launched_kernels()
    r.close()


# ---- no trace in frame state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_frames_are_untouched_by_the_motion_calls(S):
    torch = pytest.importorskip("torch")
    scene = ptss.Scene("cornell")
    prev_pose = nudged(table_of(scene.desc), 0.05)
    w, h, bounces = 40, 24, 4
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, samples_per_pass=S)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    cam = ptss.default_camera()
    side = torch.cuda.Stream()
    kept = None
    for tick in range(10):
        r.generate_frame()
        o.generate_frame()
        assert tick > 0 or not r.launched_kernels() & ptss.motion_kernels()   # only the calls below set bits 58..60
        f, _ = r.features_motion(prev_pose)
        args = {} if kept is None else dict(prev_camera=cam, prev_features=kept[0], prev_history=kept[1])
        hist = r.reproject(motion=True, **args)
        r.denoise_history(levels=1 + tick % 5)
        torch.cuda.synchronize()
        r.features_motion(prev_pose[3:9], first=3, stream=side.cuda_stream)   # and on a second stream
        r.reproject(motion=True, stream=side.cuda_stream, dev_out=r.history_devptr(2), **args)
        r.denoise_history(history=r.history_devptr(2).value, levels=5, stream=side.cuda_stream)
        kept = (f, hist)
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, ("ten frames with the motion calls after each", S), w, h, S)
    got = r.launched_kernels() & ptss.motion_kernels()
    assert ("reproject_motion",) in got and len(got) == 2 and not ptss.motion_kernels() & ptss.all_kernels()
    assert ("reproject",) not in r.launched_kernels()
    r.close()
    o.close()


def test_refusals_launch_nothing():
    scene = grid_512()
    T = scene.desc.numTriangles
    pose = table_of(scene.desc)
    r = ptss.Renderer(scene, 40, 36, max_iterations=2)
    r.generate_frame()
    L = ptss.device_lib()
    d_prev = r._device_buffer("prev", pose.nbytes)
    ptss._hip_check(ptss._hip_lib().hipMemcpy(d_prev, pose.ctypes.data, pose.nbytes, 1), "hipMemcpy")
    d_f, d_m = r.features_devptr(), r.motion_devptr()
    for first, count in ((T, 1), (T - 1, 2), (0, T + 1), (2 ** 40, 1), (1, 2 ** 40)):
        assert L.ptss_render_features_motion(r._ctx, d_prev, first, count, d_f, d_m, None) == -5, (first, count)   # PTSS_ERANGE
    assert L.ptss_render_features_motion(r._ctx, None, 0, 1, d_f, d_m, None) == -1
    assert L.ptss_render_features_motion(r._ctx, d_prev, 0, T, None, d_m, None) == -1
    assert L.ptss_render_features_motion(r._ctx, d_prev, 0, T, d_f, None, None) == -1
    r.features()
    with pytest.raises(ptss.PtssError, match="dev_history_prev"):
        r.reproject(prev_camera=ptss.default_camera(), prev_features=d_f.value, prev_history=r.history_devptr(1).value,
                    dev_out=r.history_devptr(1).value, motion=d_m.value)
    with pytest.raises(ptss.PtssError):
        r.reproject(motion=d_m.value, cosNormal=1.5)
    assert not r.launched_kernels() & ptss.motion_kernels()
    assert L.ptss_render_features_motion(r._ctx, d_prev, T - 1, 1, d_f, d_m, None) == 0   # the last triangle alone is a range
    r.synchronize()
    assert len(r.launched_kernels() & ptss.motion_kernels()) == 1
    r.close()


# ---- the point of it ------------------------------------------------------------------------------------------------------------
def panel(shift, turn_degrees):
    """A 16 x 16 grid panel (512 triangles) in the Cornell box, shifted sideways and turned about the vertical axis through its centre."""
    flat = grid_triangles((-1.5, -1.5, 0.0), (3.0, 0.0, 0.0), (0.0, 3.0, 0.0), 16, 16, GREEN)
    a = np.radians(turn_degrees)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    centre = np.array([-0.4 + shift, -1.0, -5.0])
    v = [flat[name].astype(np.float64) @ R.T + centre for name in ("vertex0", "vertex1", "vertex2")]
    return triangles_of(v[0], v[1], v[2], GREEN)


def test_history_that_follows_the_mesh_is_closer_to_the_converged_image():
    """64 samples at pose A; ptss_update_triangles to pose B (the panel 0.27 to the right, about 3.5 pixels, and turned by 3 degrees);
    one frame there; truth 1,024 spp at pose B after a reseed. Asserted: the display bytes of the motion-reprojected frame are strictly
    closer to the truth than the raw frame's, over the whole image and over the pixels of the moved surface. Measured (MI355X; the
    line this test prints, quoted in DESIGN.md §3.20): whole image 1690.71 -> 50.20 (ptss_reproject on the stale history: 63.65),
    the moved surface 574.38 -> 60.12 (stale: 230.24), 94.2 % of its pixels with history (stale: 67.2 %)."""
    box = preset_triangles()
    first, count = len(box), 512
    pose_a, pose_b = panel(0.0, 12.0), panel(0.27, 15.0)
    scene = TableScene(np.concatenate([box, pose_a]))
    r = ptss.Renderer(scene, 128, 128, max_iterations=8)
    cam = ptss.default_camera()
    ptss.move_camera(cam, "w")
    r.set_camera(cam)
    assert r.triangle_leaves() > 0   # a mesh image
    step(r, 64)
    f_a = r.features()
    r.reproject(dev_out=r.history_devptr(1), read=False)   # the history of pose A: (c, 64), kept on the device with its features
    d_fa = r._device_input("kept_features", f_a, ptss.FEATURE_DTYPE)
    r.update_triangles(pose_b, first=first)
    step(r, 1)
    raw = r.pixels().copy()
    f_b, m_b = r.features_motion(pose_a, first=first)
    kept = dict(prev_camera=cam, prev_features=d_fa.value, prev_history=r.history_devptr(1).value)
    merged = r.reproject(motion=True, **kept)
    shown = r.denoise_history(levels=0).copy()
    stale = r.reproject(dev_out=r.history_devptr(2), **kept)   # ptss_reproject misapplied: the history where the panel WAS
    shown_stale = r.denoise_history(history=r.history_devptr(2).value, levels=0).copy()
    r.reseed(0xC0FFEE)
    step(r, 1024)
    truth = r.pixels().copy()
    r.close()
    ids = m_b["surface"] - SURFACE_TRIANGLE
    on_panel = (m_b["surface"] >= SURFACE_TRIANGLE) & (ids >= first) & (ids < first + count)
    assert on_panel.sum() > 0.05 * 128 * 128
    whole = [mse(x, truth) for x in (raw, shown, shown_stale)]
    moved = [mse(x[on_panel], truth[on_panel]) for x in (raw, shown, shown_stale)]
    print(f"quality cornell + panel: whole image MSE raw {whole[0]:.2f}, motion-reprojected {whole[1]:.2f}, ptss_reproject on the stale history "
          f"{whole[2]:.2f}; moved surface ({int(on_panel.sum())} pixels) raw {moved[0]:.2f}, motion-reprojected {moved[1]:.2f}, stale {moved[2]:.2f}; "
          f"moved-surface pixels with history {100 * float((merged['weight'][on_panel] > 1).mean()):.1f} %, with the stale history "
          f"{100 * float((stale['weight'][on_panel] > 1).mean()):.1f} % (128x128, 8 bounces, truth 1,024 spp)")
    assert whole[1] < whole[0]
    assert moved[1] < moved[0]
