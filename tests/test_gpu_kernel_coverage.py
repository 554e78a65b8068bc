"""Every traced kernel instantiation against the oracle. The frame driver picks one of 32 bounceKernel instantiations (scene
variant x last bounce x scene image in LDS x first bounce) and one of 4 frameKernels (ptss_kernels.hip bounceTable /
frameTable); ptss_launched_kernels records on the host which ones a context has launched. Each case below is a scene, a
frame and a configuration chosen to reach a known set of them; it is compared with the oracle the way the other parity
tests compare (live counts every tick; accumulator, display pixels, float sums, ray-bounce total, RNG states and no guard
timeout after the path-traced frames, and again after the ray-traced one, whose mode switch resets the sums) and asserts
that it launched exactly that set. The last test asserts that the cases together reach all 36.

The variants (ptss_kernels.hip sceneVariant): accel = the chunked many-sphere image; bounded+pairs = bounded geometry
(SceneLayout::sphereBounded) and a camera in range, at least two lights and four in five primitives diffuse
(SceneLayout::neePairs); bounded = the same without pairs; plain = everything else (a sphere radius below 1e-12, or a camera
out of range). The image is staged in LDS when it fits 64 KiB with the work area, else read in place (ptss_create); the
cases stay far from that edge on both sides (a few KiB against 75-90 KiB), so that builds with another tile size keep the
same choice. first + last in one launch: one bounce, i.e. the ray-tracing mode ("both" below: path frames, then one
ray-tracing frame).

Under tests/test_gpu_build_variants.py this module runs against other builds of the library. Only one of them changes
which instantiation runs: the `knobs` build with PTSS_SCENE_PATH=scalar reads every image in place, so there every expected
bounce instantiation is mapped to its in-place twin (the one-launch frame kernel always stages the image in LDS, and
whether a frame qualifies for it is decided before the override, so the frame cases keep theirs). Every oracle comparison
holds under every build."""
import os

import numpy as np
import pytest

import oracle
import ptss
from test_gpu_edge_scenes import COOK, CREAM, GLASS, GREEN, LAMP, FLOOR, MIRROR, PHONG, RED, build
from test_gpu_build_variants import build_variants_module
from test_gpu_fuzz_scenes import random_scene

pytestmark = pytest.mark.gpu

LIBNAME = os.path.basename(ptss.DEVICE_LIB)
ALL_IN_PLACE = LIBNAME == "libptss_knobs.so" and os.environ.get("PTSS_SCENE_PATH") == "scalar"

ONE_LIGHT = dict(area=[((50, 50, 50), 2)])                                          # LAMP = triangles 2 and 3
TWO_LIGHTS = dict(area=[((50, 50, 50), 2)], point=[((-2.5, 2.0, -2.0), (30, 30, 30))])
GLOSSY = [((0, 0, -3), 0.8, COOK), ((-1.6, -0.2, -4), 0.7, GLASS), ((1.5, 0.1, -3.5), 0.6, MIRROR), ((0.6, 0.9, -5), 0.5, PHONG)]
DIFFUSE = [((-1.8, -0.3, -4.2), 0.7, CREAM), ((0.1, -0.4, -3.4), 0.6, RED), ((1.7, -0.2, -4.6), 0.8, GREEN), ((0.2, 0.9, -5.5), 0.5, CREAM),
           ((-0.9, 1.6, -4.8), 0.4, GREEN), ((1.1, 1.4, -3.9), 0.35, RED), ((0, -0.7, -2.2), 0.3, CREAM)]
TINY = ((0.5, -0.5, -2.0), 1e-13, RED)   # a radius below 1e-12: the geometry is not bounded, the plain variant runs


def back_wall(cols=24, rows=10):
    """480 small diffuse triangles tiling the wall behind the scene (z = -8.9): 4,800 rows of the scene image, 77 KiB, so that a
    scene carrying them is read in place; the rays hit them, so those reads decide the image."""
    tris = []
    for i in range(cols):
        for j in range(rows):
            x0, x1 = -4 + 8 * i / cols, -4 + 8 * (i + 1) / cols
            y0, y1 = -1 + 4 * j / rows, -1 + 4 * (j + 1) / rows
            m = (CREAM, GREEN, RED)[(i + j) % 3]
            tris += [((x0, y0, -8.9), (x1, y0, -8.9), (x1, y1, -8.9), m), ((x0, y0, -8.9), (x1, y1, -8.9), (x0, y1, -8.9), m)]
    return tris


def sphere_grid(n):
    """n spheres on a grid, a third of them glossy (no pairs with one light anyway): with cfg.everySphereLoop the plain image
    holds 2.25 rows per sphere, 86 KiB at 2,400."""
    return [((-3.5 + 0.3 * (i % 24), -0.9 + 0.3 * ((i // 24) % 10), -4.0 - 0.3 * (i // 240)), 0.12, (CREAM, MIRROR, GREEN)[i % 3])
            for i in range(n)]


SCENES = {
    "bounded": lambda: build(spheres=GLOSSY, triangles=FLOOR + LAMP, **ONE_LIGHT),
    "pairs": lambda: build(spheres=DIFFUSE, triangles=FLOOR + LAMP, **TWO_LIGHTS),
    "plain": lambda: build(spheres=GLOSSY + [TINY], triangles=FLOOR + LAMP, **TWO_LIGHTS),
    "bounded_padded": lambda: build(spheres=GLOSSY, triangles=FLOOR + LAMP + back_wall(), **ONE_LIGHT),
    "pairs_padded": lambda: build(spheres=DIFFUSE, triangles=FLOOR + LAMP + back_wall(), **TWO_LIGHTS),
    "plain_padded": lambda: build(spheres=GLOSSY + [TINY], triangles=FLOOR + LAMP + back_wall(), **TWO_LIGHTS),
    "sphere_grid": lambda: build(spheres=sphere_grid(2400), triangles=FLOOR + LAMP, **ONE_LIGHT),
    "accel_300": lambda: random_scene(7301, ns=300, nt=6)[0],
    "accel_4500": lambda: random_scene(7302, ns=4500, nt=8)[0],
}
FAR = (0.0, 0.0, 4e15)   # beyond the 1e15 range: a bounded image runs the plain variant for these frames


def bounces_of(variant, lds, bounces, mode):
    """The bounce instantiations a bounce-by-bounce context launches: first / middle / last of `bounces`, and with "ray" or "both"
    the first-and-last one of the one-bounce ray-tracing frame."""
    out = set()
    if mode in ("path", "both"):
        for i in range(bounces):
            out.add(("bounce", variant, i == bounces - 1, lds, i == 0))
    if mode in ("ray", "both"):
        out.add(("bounce", variant, True, lds, True))
    return out


# name: scene, w, h, bounces, S, camera, mode, one_launch_frames, every_sphere_loop, expected instantiations
CASES = {
    "bounded_lds": ("bounded", 37, 23, 4, 2, (0.3, 0.2, 0.5), "both", 0, False, bounces_of("bounded", True, 4, "both")),
    "pairs_lds": ("pairs", 40, 24, 5, 1, None, "both", 0, False, bounces_of("bounded+pairs", True, 5, "both")),
    "plain_lds": ("plain", 29, 31, 4, 3, None, "both", 0, False, bounces_of("plain", True, 4, "both")),
    "bounded_in_place": ("bounded_padded", 45, 27, 4, 2, None, "both", 0, False, bounces_of("bounded", False, 4, "both")),
    "pairs_in_place": ("pairs_padded", 33, 19, 5, 1, None, "both", 0, False, bounces_of("bounded+pairs", False, 5, "both")),
    "plain_in_place": ("plain_padded", 41, 17, 4, 2, None, "both", 0, False, bounces_of("plain", False, 4, "both")),
    "bounded_spheres_in_place": ("sphere_grid", 23, 13, 3, 1, None, "path", 0, True, bounces_of("bounded", False, 3, "path")),
    "accel_lds": ("accel_300", 39, 21, 5, 2, None, "both", 0, False, bounces_of("accel", True, 5, "both")),
    "accel_in_place": ("accel_4500", 25, 15, 4, 1, None, "both", 0, False, bounces_of("accel", False, 4, "both")),
    "frame_accel": ("accel_300", 41, 23, 5, 1, None, "both", 1, False, {("frame", "accel")}),
    "frame_pairs": ("pairs", 35, 21, 6, 2, None, "both", 1, False, {("frame", "bounded+pairs")}),
    "frame_bounded": ("bounded", 48, 27, 5, 3, None, "both", 1, False, {("frame", "bounded")}),
    "frame_plain": ("plain", 31, 29, 5, 1, None, "path", 1, False, {("frame", "plain")}),
    "frame_plain_camera_far": ("bounded", 36, 20, 4, 1, FAR, "path", 1, False, {("frame", "plain")}),
}
_REACHED = {}   # case name -> instantiations it launched (test_every_instantiation_is_reached)


def expected(case):
    want = CASES[case][-1]
    if ALL_IN_PLACE:
        want = {k[:3] + (False,) + k[4:] if k[0] == "bounce" else k for k in want}
    return want


def compare(r, o, what, w, h, S):
    """Everything the frames so far have left: accumulator, display pixels, float sums, ray-bounce total, RNG states, no timeout."""
    assert np.array_equal(r.accumulator(), o.accumulator()), what
    assert np.array_equal(r.pixels(), o.pixels()), what
    assert np.array_equal(r.float_accumulator(), o.float_sum(), equal_nan=True), what
    assert r.total_ray_bounces() == o.total_ray_bounces(), what
    for p in (0, w * h // 2, w * h - 1):
        for lane in {0, S - 1}:
            assert np.array_equal(r.rng_state(p, lane), o.rng_state(p, lane)), (what, p, lane)
    assert r.guard_timeouts() == 0, what


def run_case(name):
    scene_name, w, h, bounces, S, camera, mode, one_launch, every_sphere_loop, _ = CASES[name]
    scene = SCENES[scene_name]()
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, samples_per_pass=S, one_launch_frames=one_launch,
                      every_sphere_loop=every_sphere_loop, seed=0x5EED + len(name))
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S, seed=0x5EED + len(name))
    assert r.one_launch_frames == bool(one_launch), name
    if camera is not None:
        cam = ptss.default_camera()
        cam.position.x, cam.position.y, cam.position.z = camera
        r.set_camera(cam)
        o.set_camera(cam)
    ticks = ["path"] * 2 if mode in ("path", "both") else []
    ticks += ["ray"] if mode in ("ray", "both") else []
    for t, kind in enumerate(ticks):
        if kind == "ray":             # one-bounce ray tracing from here on: a reset (CudaTracer.cu:760-765) clears the sums
            compare(r, o, (name, "path frames"), w, h, S)
            r.set_mode(False)
            o.set_mode(False)
        r.generate_frame()
        o.generate_frame()
        assert np.array_equal(r.live_counts(), o.live_counts()), (name, t)
    compare(r, o, (name, ticks[-1] + " frames"), w, h, S)
    launched = r.launched_kernels()
    r.close()
    o.close()
    return launched


@pytest.mark.parametrize("name", list(CASES))
def test_instantiation_matches_the_oracle(name):
    launched = run_case(name)
    _REACHED[name] = launched
    assert launched == expected(name), sorted(launched ^ expected(name))


def test_every_instantiation_is_reached():
    """The union over the cases: all 36 instantiations (every in-place one twice, under PTSS_SCENE_PATH=scalar)."""
    missing_cases = sorted(set(CASES) - set(_REACHED))
    assert not missing_cases, f"cases that did not run or failed: {missing_cases}"
    union = set().union(*_REACHED.values())
    want = set().union(*(expected(c) for c in CASES))
    print(f"kernel instantiations reached: {len(union)}/{len(ptss.all_kernels())}")
    assert union == want
    if not ALL_IN_PLACE:
        assert union == ptss.all_kernels() and len(union) == 36


def _diag_bits():
    """PTSS_DIAG of the library under test: that of its tools/build_variants.py entry (0 for the shipped library)."""
    bv = build_variants_module()
    tag = LIBNAME[len("libptss_"):-len(".so")] if LIBNAME.startswith("libptss_") else None
    for d in bv.VARIANTS.get(tag, []):
        if d.startswith("PTSS_DIAG="):
            return int(d.split("=")[1])
    return 0


# counter words that a frame of the "pairs" scene and one of "accel_300" must move, by PTSS_DIAG bit (csrc/ptss_diag.h)
DIAG_WORDS = {1: [2, 6],            # sphere candidates: waves through the closest-hit and the dense any-hit candidate pass
              2: [0],               # scatter: waves in scatter() at all
              4: [2],               # chunk culling: rays through the chunk bounds (the many-sphere scene)
              8: [7],               # shadow-segment pairs: NEE rounds of the paired kernels (the pairs scene)
              16: list(range(8))}   # shadow-queue lengths: one histogram bin per wave and NEE round (their sum)


def test_debug_counters_only_in_diagnostic_builds():
    """The shipped library carries no counter (ptss_debug_counters reads zeros); a diagnostic build's counters are device-wide
    and never reset, so the words of its own bit are read before and after this test's frames — a pairs scene (candidates,
    scatter, paired shadow segments, queues) and a chunked one (chunk culling) — and must have grown."""
    bits = _diag_bits()
    before = after = None
    for scene_name in ("pairs", "accel_300"):
        scene = SCENES[scene_name]()
        r = ptss.Renderer(scene, 64, 48, max_iterations=4)
        if before is None:
            before = np.asarray(r.debug_counters(), dtype=np.uint64)
        for _ in range(2):
            r.generate_frame()
        after = np.asarray(r.debug_counters(), dtype=np.uint64)
        r.close()
    if not bits:
        assert not before.any() and not after.any(), f"{LIBNAME} is not a diagnostic build but reports counters {after}"
        return
    assert bits & ~sum(DIAG_WORDS) == 0, f"PTSS_DIAG={bits} has bits this test does not know"
    for b, words in DIAG_WORDS.items():
        if bits & b:
            grown = int(after[words].sum()) - int(before[words].sum())
            assert grown > 0, f"{LIBNAME}: PTSS_DIAG bit {b}: words {words} did not move ({before} -> {after})"
