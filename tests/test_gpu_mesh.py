"""The mesh image: scenes of 512 .. 2^20 triangles and fewer than 64 spheres are traced through a two-level
hierarchy of triangle leaves and groups. Each case loads procedural OBJ models into a preset (Scene.add_obj), renders on the
GPU and compares with the oracle the way the other parity tests do — live counts every tick; accumulator, display pixels, float
sums, ray-bounce total and RNG states at the end — and checks which bounce kernels ran (Renderer.launched_kernels). The 64k-triangle
frame is too slow for the oracle: there the chunked image is compared with the every-triangle loop (cfg.everySphereLoop)."""
import numpy as np
import pytest

import oracle
import ptss
from meshgen import grid_obj, icosphere_obj, strip_obj, translate_scale, write
from ptss_types import Material

pytestmark = pytest.mark.gpu

# materials of the "cornell" preset: 0 red Phong, 1 glass, 2 white, 3 red, 4 green, 5 emitter, 6 mirror
PHONG, GLASS, WHITE, RED, GREEN, MIRROR = 0, 1, 2, 3, 4, 6


def mesh_kernels_of(lds, bounces, mode):
    out = set()
    if mode in ("path", "both"):
        out |= {("bounce", "mesh", i == bounces - 1, lds, i == 0) for i in range(bounces)}
    if mode in ("ray", "both"):
        out.add(("bounce", "mesh", True, lds, True))
    return out


def compare(r, o, what, w, h, S):
    assert np.array_equal(r.accumulator(), o.accumulator()), what
    assert np.array_equal(r.pixels(), o.pixels()), what
    assert np.array_equal(r.float_accumulator(), o.float_sum()), what
    assert r.total_ray_bounces() == o.total_ray_bounces(), what
    for p in (0, w * h // 3, w * h - 1):
        for lane in {0, S - 1}:
            assert np.array_equal(r.rng_state(p, lane), o.rng_state(p, lane)), (what, p, lane)
    assert r.guard_timeouts() == 0, what


def run(scene, w, h, bounces, ticks=2, S=1, camera=None, mode="path", frame_lanes=0, expect_mesh=True, lds=True):
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, samples_per_pass=S, frame_lanes=frame_lanes)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    try:
        if camera is not None:
            cam = ptss.default_camera()
            cam.position.x, cam.position.y, cam.position.z = camera
            r.set_camera(cam)
            o.set_camera(cam)
        if mode in ("path", "both"):
            for t in range(ticks):
                r.generate_frame()
                o.generate_frame()
                assert np.array_equal(r.live_counts(), o.live_counts()), t
            compare(r, o, "path-traced frames", w, h, S)
        if mode in ("ray", "both"):
            r.set_mode(0)
            o.set_mode(0)
            r.generate_frame()
            o.generate_frame()
            compare(r, o, "ray-traced frame", w, h, S)
        n = scene.desc.numTriangles
        if expect_mesh:
            assert r.triangle_leaves() == (n + 15) // 16
            assert r.launched_kernels() == mesh_kernels_of(lds, bounces, mode)
        else:
            assert r.triangle_leaves() == 0
            assert not (r.launched_kernels() & ptss.mesh_kernels())
    finally:
        r.close()


def cornell_with(tmp_path, *models):
    """The 'cornell' preset with OBJ models: (obj text, transform or None, material)."""
    s = ptss.Scene("cornell")
    for k, (text, m, mat) in enumerate(models):
        s.add_obj(write(tmp_path, f"m{k}.obj", text), transform=m, material=mat)
    return s


def test_cornell_walls_tessellated_into_ten_thousand_triangles(tmp_path):
    # floor, back and left wall again, as 3 x 3,200 triangles lying exactly on the preset's own walls: exact ties everywhere
    s = cornell_with(tmp_path, (grid_obj((-4, -4, 0), (8, 0, 0), (0, 0, -8), 40, 40), None, WHITE),
                     (grid_obj((-4, -4, -8), (8, 0, 0), (0, 8, 0), 40, 40), None, WHITE),
                     (grid_obj((-4, -4, 0), (0, 0, -8), (0, 8, 0), 40, 40, normals=False), None, RED))
    assert s.desc.numTriangles == 14 + 9600
    run(s, 48, 40, 5)


@pytest.mark.parametrize("material", [GLASS, PHONG])
def test_icosphere_of_five_thousand_triangles(tmp_path, material):
    s = cornell_with(tmp_path, (icosphere_obj(4), translate_scale(0.3, -2.2, -5.0, 1.6), material))
    run(s, 40, 40, 6)


def test_mesh_preset_cook_torrance_and_ray_tracing_mode():
    run(ptss.Scene("mesh"), 44, 36, 5, mode="both")


def test_floor_seen_from_a_camera_in_its_plane(tmp_path):
    # a tessellated shelf at y = -1 and the camera at y = -1: grazing rays, |det| near the 1e-7 floor
    s = cornell_with(tmp_path, (grid_obj((-3, -1, -1), (6, 0, 0), (0, 0, -6), 20, 20), None, WHITE))
    run(s, 48, 32, 4, camera=(0.0, -1.0, 0.0))


def test_duplicated_mesh_with_a_second_material_ties_to_the_higher_index(tmp_path):
    m = translate_scale(-0.5, -2.5, -5.0, 1.4)
    s = cornell_with(tmp_path, (icosphere_obj(3), m, GREEN), (icosphere_obj(3), m, PHONG))
    run(s, 40, 32, 4)


def test_camera_inside_a_group_bound():
    run(ptss.Scene("mesh"), 32, 32, 4, camera=(0.5, -2.5, -5.5))


def test_several_samples_per_pass_and_two_frame_lanes(tmp_path):
    s = cornell_with(tmp_path, (icosphere_obj(4), translate_scale(0.0, -2.0, -5.0, 1.5), PHONG))
    run(s, 36, 28, 5, S=3)
    run(s, 64, 48, 5, frame_lanes=2)


def test_image_read_in_place(tmp_path):
    # 700 extra materials push the staged part of the image past 64 KiB: the mesh kernels read it in place
    s = cornell_with(tmp_path, (icosphere_obj(4), translate_scale(0.0, -2.0, -5.0, 1.5), GREEN))
    mats = (Material * (s.desc.numMaterials + 700))(*s.materials, *([s.materials[WHITE]] * 700))
    s.desc.materials, s.desc.numMaterials = mats, len(mats)
    s._keep = mats
    run(s, 32, 24, 4, mode="both", lds=False)


@pytest.mark.parametrize("total", [255, 256, 511, 512])
def test_threshold_between_the_old_paths_and_the_mesh_image(tmp_path, total):
    # 255: the edge-classed image; 256 .. 511: the caller's order (the older suites' largest scene has 484 triangles); 512: mesh
    s = cornell_with(tmp_path, (strip_obj(total - 14), None, GREEN))
    assert s.desc.numTriangles == total
    run(s, 40, 30, 4, expect_mesh=total >= 512)


def test_64k_triangles_match_the_every_triangle_loop(tmp_path):
    s = cornell_with(tmp_path, *[(icosphere_obj(5), translate_scale(x, -2.6, -5.5, 1.1), mat) for x, mat in ((-2.2, GLASS), (0.0, PHONG), (2.2, GREEN))])
    assert s.desc.numTriangles == 14 + 3 * 20480
    out = []
    for every in (False, True):
        r = ptss.Renderer(s, 640, 360, max_iterations=8, float_accumulator=True, every_sphere_loop=every)
        try:
            r.generate_frame()
            out.append((r.accumulator(), r.live_counts(), r.total_ray_bounces(), r.triangle_leaves(), r.launched_kernels()))
        finally:
            r.close()
    (a, lc, tb, leaves, kern), (b, lc2, tb2, leaves2, kern2) = out
    assert leaves == (s.desc.numTriangles + 15) // 16 and leaves2 == 0
    assert kern == mesh_kernels_of(True, 8, "path") and not (kern2 & ptss.mesh_kernels())
    assert np.array_equal(a, b)
    assert np.array_equal(lc, lc2) and tb == tb2
