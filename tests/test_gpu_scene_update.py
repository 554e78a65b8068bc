"""Updating the scene of a live context: ptss_set_scene (whole scene, host path), ptss_update_triangles
(device-side vertex data, sceneUpdateKernel + meshRefitKernel), ptss_reseed and the read-backs. Frames are 48 x 32 at one sample
per tick, 3 frames per leg; "equals the oracle" means accumulator, display pixels, live counts and the RNG records of sampled
pixels are array_equal. Queries are compared with a FRESH context created on the updated scene with everySphereLoop = 1 (the
reference's loops over every primitive), in every field of every ray. Every context here is single-lane with one launch per bounce;
tests/test_gpu_live_context.py runs the same calls on live contexts of every other configuration, across changes of image kind."""
import numpy as np
import pytest

import oracle
import ptss
from scene_update_common import LIGHT, TableScene, deform, m1296, m530, p300, preset_triangles, seventy_spheres, stored

pytestmark = pytest.mark.gpu

W, H, BOUNCES, SEED2 = 48, 32, 4, 0xC0FFEE


def frames_equal_oracle(r, o, n=3):
    for _ in range(n):
        r.generate_frame()
        o.generate_frame()
        assert np.array_equal(r.live_counts(), o.live_counts())
    assert np.array_equal(r.accumulator(), o.accumulator())
    assert np.array_equal(r.pixels(), o.pixels())
    for p in (0, W * H // 3, W * H - 1):
        assert np.array_equal(r.rng_state(p), o.rng_state(p)), p


def renderer(scene, **kw):
    return ptss.Renderer(scene, W, H, max_iterations=BOUNCES, **kw)


def the_oracle(scene, seed=0x5EED):
    return oracle.Oracle(scene.desc, W, H, max_iterations=BOUNCES, seed=seed)


def query_rays(tris, seed=4):
    """4,096 rays: the pixel-centre camera rays, and rays leaving surface points in random directions, some not unit."""
    rng = np.random.default_rng(seed)
    cam = ptss.camera_rays(ptss.default_camera(), W, H)
    n = 4096 - len(cam)
    k = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    p = b[:, :1] * tris["vertex0"][k] + b[:, 1:2] * tris["vertex1"][k] + b[:, 2:] * tris["vertex2"][k]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::5] *= rng.uniform(0.3, 3.0, (len(d[::5]), 1))
    tmax = np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.1, 10.0, n))
    return np.concatenate([cam, ptss.make_rays(p, d.astype(np.float32), tmax)])


def queries_equal_fresh(r, scene_now, rays):
    fresh = renderer(scene_now, every_sphere_loop=True)
    try:
        assert r.intersect(rays).tobytes() == fresh.intersect(rays).tobytes()
        assert np.array_equal(r.occluded(rays), fresh.occluded(rays))
    finally:
        fresh.close()


def twelve_triangle_spheres():
    """70 spheres and 12 triangles: the many-sphere image (two images per context), its triangles edge-classed."""
    return seventy_spheres(preset_triangles()[:12], point_lights=LIGHT, keep_area_lights=False)


def kinds(r):
    k = r.launched_kernels()
    return {"mesh": any(x[:2] == ("bounce", "mesh") for x in k), "accel": any(x[:2] == ("bounce", "accel") for x in k)}


def test_set_scene_before_the_first_frame_changes_the_image_kind():
    cornell = ptss.Scene("cornell")
    spheres = twelve_triangle_spheres()
    mesh = m530()
    for before, after, leaves, kind in ((cornell, mesh, 34, "mesh"), (mesh, spheres, 0, "accel"), (spheres, cornell, 0, None)):
        r, o = renderer(before), the_oracle(after)
        try:
            r.set_scene(after)
            frames_equal_oracle(r, o)
            assert r.triangle_leaves() == leaves
            assert kinds(r) == {"mesh": kind == "mesh", "accel": kind == "accel"}
        finally:
            r.close()


def test_continuity_across_two_replacements():
    a, b = ptss.Scene("cornell"), m530()
    r, o = renderer(a), the_oracle(a)
    try:
        for _ in range(3):
            r.generate_frame()
            o.generate_frame()
        r.set_scene(b)
        r.set_scene(a)
        o.request_reset()
        frames_equal_oracle(r, o)
    finally:
        r.close()


def test_reseed_gives_the_streams_of_a_fresh_context():
    a, b = ptss.Scene("cornell"), m530()
    r = renderer(a)
    try:
        r.generate_frame()
        r.generate_frame()
        r.set_scene(b)
        r.reseed(SEED2)
        frames_equal_oracle(r, the_oracle(b, seed=SEED2))
    finally:
        r.close()


@pytest.mark.parametrize("make", [m530, m1296])
def test_refit_bytes_equal_the_host_probe(make):
    scene = make()
    new = deform(scene.triangles)
    n = len(new)
    r = renderer(scene)
    try:
        leaves, pos = r.triangle_leaves(), r.triangle_positions(n)
        r.update_triangles(new)
        assert r.launched_kernels() >= {("update",), ("refit",)}
        assert np.array_equal(r.triangle_positions(n), pos) and r.triangle_leaves() == leaves == (n + 15) // 16
        order = np.empty(n, dtype=np.int64)
        order[pos] = np.arange(n)   # stored position -> original index
        want = ptss.probe_mesh_refit(stored(new)[order])
        got = r.triangle_bounds()
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert r.update_rejected() == 0
    finally:
        r.close()


@pytest.mark.parametrize("make", [m530, m1296])
def test_refit_image_equals_a_fresh_context_and_the_oracle(make):
    scene = make()
    new = deform(scene.triangles)
    moved = scene.with_triangles(new)
    r = renderer(scene)
    try:
        r.update_triangles(new)   # before the first frame
        queries_equal_fresh(r, moved, query_rays(new))
        frames_equal_oracle(r, the_oracle(moved))
    finally:
        r.close()
    r = renderer(scene)
    try:
        r.generate_frame()
        r.generate_frame()
        r.update_triangles(new)
        r.reseed(SEED2)
        frames_equal_oracle(r, the_oracle(moved, seed=SEED2))
    finally:
        r.close()


def test_partial_range():
    scene = m530()
    new = deform(scene.triangles)
    part = scene.triangles.copy()
    part[17:117] = new[17:117]
    r = renderer(scene)
    try:
        r.update_triangles(new[17:117], first=17)
        queries_equal_fresh(r, scene.with_triangles(part), query_rays(part))
        L = ptss.device_lib()
        assert L.ptss_update_triangles(r._ctx, r._buffers["triangles_upload"], 500, 31, None) == -5   # PTSS_ERANGE
        assert L.ptss_update_triangles(r._ctx, r._buffers["triangles_upload"], 530, 1, None) == -5
        assert L.ptss_update_triangles(r._ctx, None, 0, 1, None) == -1
        assert L.ptss_update_triangles(r._ctx, None, 0, 0, None) == 0
    finally:
        r.close()


def test_images_without_a_hierarchy_are_updated_and_never_refitted():
    scene = p300()
    new = deform(scene.triangles)
    r = renderer(scene)
    try:
        r.update_triangles(new)
        k = r.launched_kernels()
        assert ("update",) in k and ("refit",) not in k
        with pytest.raises(ptss.PtssError):
            r.triangle_bounds()
        frames_equal_oracle(r, the_oracle(scene.with_triangles(new)))
    finally:
        r.close()


def test_both_images_of_a_many_sphere_context_are_updated():
    scene = seventy_spheres(p300().triangles)
    new = deform(scene.triangles)
    moved = scene.with_triangles(new)
    r = renderer(scene)
    try:
        r.update_triangles(new)
        k = r.launched_kernels()
        assert ("update",) in k and ("refit",) not in k
        frames_equal_oracle(r, the_oracle(moved))          # images[0], the chunked image
        assert kinds(r)["accel"]
        far = ptss.default_camera()
        far.position.x = 2e15                               # outside the chunked image's range: images[1]
        o = the_oracle(moved)
        r.set_camera(far)
        o.set_camera(far)
        r.reseed(0x5EED)
        frames_equal_oracle(r, o)
    finally:
        r.close()


def test_an_edge_classed_scene_refuses_the_device_path():
    for scene in (ptss.Scene("cornell"), twelve_triangle_spheres()):
        n = scene.desc.numTriangles
        tris = scene.triangles if isinstance(scene, TableScene) else preset_triangles()
        r = renderer(scene)
        try:
            with pytest.raises(ptss.PtssError, match="ptss_set_scene"):
                r.update_triangles(deform(tris[:n]))
            assert ("update",) not in r.launched_kernels()
            frames_equal_oracle(r, the_oracle(scene))
        finally:
            r.close()


def test_rejected_records_keep_their_old_geometry():
    scene = m530()
    new = deform(scene.triangles)
    new["vertex1"][5, 1] = np.nan
    new["vertex2"][40, 0] = 2.0 ** 41
    applied = new.copy()
    applied[[5, 40]] = scene.triangles[[5, 40]]
    r = renderer(scene)
    try:
        r.update_triangles(new)
        assert r.update_rejected() == 2
        queries_equal_fresh(r, scene.with_triangles(applied), query_rays(applied))
        at = np.full(1, 2.0 ** 40, dtype=np.float32)      # the limit itself is inside
        edge = applied[:1].copy()
        edge["vertex0"][0, 2] = -at[0]
        r.update_triangles(edge, first=0)
        assert r.update_rejected() == 2
    finally:
        r.close()


def test_update_features_and_denoise_in_stream_order_and_counters_survive():
    scene = m530()
    new = deform(scene.triangles)
    moved = scene.with_triangles(new)
    r = renderer(scene, sync_each_frame=False)
    try:
        r.generate_frame()
        r.generate_frame()
        before = r.total_ray_bounces()
        r.update_triangles(new)
        r.generate_frame()
        feat = r.features()
        out = r.denoise(levels=2)
        assert out.shape == (W * H, 4)
        fresh = renderer(moved, every_sphere_loop=True)
        try:
            hits = fresh.intersect(ptss.camera_rays(ptss.default_camera(), W, H))
        finally:
            fresh.close()
        assert feat["normal"].tobytes() == hits["normal"].tobytes()
        assert feat["depth"].tobytes() == hits["distance"].tobytes()
        assert np.array_equal(feat["materialIdx"], hits["materialIdx"])
        mid = r.total_ray_bounces()
        assert mid >= before + W * H
        r.set_scene(ptss.Scene("cornell"))
        r.generate_frame()
        assert r.total_ray_bounces() >= mid + W * H
        assert ("update",) in r.launched_kernels()         # cumulative across set_scene
    finally:
        r.close()


def test_a_device_tensor_is_taken_in_place():
    torch = pytest.importorskip("torch")
    scene = m530()
    new = deform(scene.triangles)
    r = renderer(scene)
    try:
        t = torch.from_numpy(new.view(np.float32).reshape(-1, 19).copy()).cuda()
        r.update_triangles(t)
        torch.cuda.synchronize()
        want = renderer(scene)
        try:
            want.update_triangles(new)
            assert np.array_equal(r.triangle_bounds().view(np.uint32), want.triangle_bounds().view(np.uint32))
        finally:
            want.close()
    finally:
        r.close()


def test_the_uploaded_image_is_the_one_the_host_probe_packs():
    """libptss.so uploads what ptss.probe_pack_scene reports (csrc/ptpack.h compiled twice): positions, bounds and leaves, bit for bit."""
    scene = m530()
    L, blob, in_lds = ptss.probe_pack_scene(scene)
    r = ptss.Renderer(scene, 64, 64, max_iterations=1)
    try:
        leaves, groups = L["numLeaves"], L["numGroups"]
        assert in_lds and r.triangle_leaves() == leaves == 34
        positions = blob.view(np.int32).reshape(-1)[4 * L["offTriPos"]:4 * L["offTriPos"] + 530]
        assert np.array_equal(r.triangle_positions(530), positions)
        bounds = np.concatenate([blob[L["offLeaf"]:L["offLeaf"] + 3 * leaves], blob[L["offGroup"]:L["offGroup"] + 3 * groups]]).reshape(-1, 12)
        assert r.triangle_bounds().tobytes() == bounds.tobytes()
    finally:
        r.close()
