"""Cases and expected values shared by tests/test_path_query_cpu.py and tests/test_gpu_path_query.py (ptss_seed_path_rng /
ptss_trace_paths).

The main pin is an identity: a path query fed a frame's own eye rays and random streams reproduces that frame's linear radiance and
final stream states bit for bit — as long as the frame's loop guard (`numRays > 128`, CudaTracer.cu:622) never fires, because a path
query has no such guard. So every case here must keep more than 128 rays alive in every iteration on the oracle
(test_path_query_cpu.py checks that without a GPU); a case that does not is replaced here, never skipped.

A scene is read in place instead of staged in LDS once its image passes 64 KiB. `in_place(scene)` gets there by appending materials
nothing refers to: geometry, lights and therefore the oracle's answer stay the same, so the two placements share one expectation."""
import ctypes as C

import numpy as np

import oracle
import ptss
from ptss_types import Material, SceneDesc
from scene_update_common import LIGHT, TableScene, deform, icosphere_triangles, preset_triangles, seventy_spheres

W, H = 64, 48
N = W * H
ITERATIONS = (1, 2, 4, 8)
SEED = 0x5EED
COOK, PHONG, GLASS = 0, 6, 7   # materials of the "mixed" preset: Cook-Torrance, Phong, glass (specAvg 0.9, refrAvg 0.9, index 1.55)


def _camera(position=None):
    cam = ptss.default_camera()
    if position is not None:
        cam.position.x, cam.position.y, cam.position.z = position
    return cam


def _mixed(**kw):
    """The "mixed" preset's box (mirror walls, its 22 spheres unless replaced, its two area lights) around more: paths live long in it."""
    extra = kw.pop("extra_triangles", None)
    t = preset_triangles("mixed")
    if extra is not None:
        t = np.concatenate([t, extra])
    return TableScene(t, preset="mixed", **kw)


# name: (scene maker, cfg.everySphereLoop, camera position or None, seed). The Cornell box absorbs 38 % of its rays per bounce: from
# the default camera 64 x 48 rays do not last eight iterations, from beside its glass sphere they do.
SCENES = {
    "cornell": (lambda: ptss.Scene("cornell"), False, (-0.5, -3.0, -3.5), SEED),
    "mixed": (lambda: ptss.Scene("mixed"), False, None, 0xABCDEF),
    "default": (lambda: ptss.Scene("default"), False, None, 7),
    # a point light as well as the two area lights: point lights come first in shade()'s sum
    "point_light": (lambda: _mixed(point_lights=LIGHT), False, (0.4, -0.3, -0.2), SEED),
    # 16 + 1,280 triangles, an icosphere of tests/meshgen.py: the mesh image
    "mesh": (lambda: _mixed(extra_triangles=icosphere_triangles(3, (0.5, -2.2, -4.8), 1.5, PHONG)), False, None, 0x1234567),
    # 70 spheres: the many-sphere image (and the plain one beside it, which queries do not use)
    "many_spheres": (lambda: seventy_spheres(preset_triangles("mixed"), preset="mixed"), False, None, SEED),
    # the same scene through the every-primitive loops
    "every_sphere_loop": (lambda: seventy_spheres(preset_triangles("mixed"), preset="mixed"), True, (0.2, 0.1, -0.3), 99),
    # the camera (at the origin) inside a glass sphere: bounce 0 hits from inside, Beer-Lambert and total internal reflection
    "inside_glass": (lambda: _mixed(spheres=[(0.0, 0.0, -0.2, 1.0, GLASS), (1.0, -3.0, -5.6, 1.0, PHONG), (-2.0, -2.5, -5.2, 1.5, COOK)]), False, None,
                     31337),
}
CASES = [(name, iterations) for name in SCENES for iterations in ITERATIONS]
PADDING_MATERIALS = 900   # 5 rows of 16 B each: 72 KB on top of any image


class _Wrapped:
    pass


def in_place(scene):
    """`scene` with PADDING_MATERIALS unused materials behind its own: the image no longer fits the 64 KiB LDS window."""
    d = scene.desc
    mats = (Material * (d.numMaterials + PADDING_MATERIALS))(*[d.materials[k] for k in range(d.numMaterials)],
                                                                *([d.materials[0]] * PADDING_MATERIALS))
    out = _Wrapped()
    out.desc = SceneDesc()
    C.memmove(C.byref(out.desc), C.byref(d), C.sizeof(SceneDesc))
    out.desc.materials, out.desc.numMaterials = mats, len(mats)
    out.keep = (scene, mats)
    return out


def make_scene(name, placement="lds"):
    scene = SCENES[name][0]()
    return in_place(scene) if placement == "in_place" else scene


def camera_of(name):
    return _camera(SCENES[name][2])


_JITTER = {}


def jitter(seed, n=N):
    """(n, 2) float32: the two uniforms computeEyeRaysKernel draws for pixel p, stream curand_init(seed, p, 0)."""
    if (seed, n) not in _JITTER:
        _JITTER[(seed, n)] = np.array([oracle.probe_rng(seed, p, 2)[2] for p in range(n)], dtype=np.float32)
    return _JITTER[(seed, n)]


def eye_rays(cam, seed, width=W, height=H, rows=None):
    """The frame's own eye rays: ptss_camera_ray of every pixel with the pixel's two jitter draws, (pixels, 8) float32 in pixel order.
    rows: only these global rows (a shard's)."""
    jit = jitter(seed, width * height)
    q = ptss.RayQuery()
    buf = (C.c_float * 8).from_buffer(q)
    fn = ptss.host_lib().ptss_camera_ray
    ys = range(height) if rows is None else [int(y) for y in rows]
    out = np.empty((len(ys) * width, 8), dtype=np.float32)
    k = 0
    for y in ys:
        for x in range(width):
            p = y * width + x
            assert fn(C.byref(cam), width, height, x, y, C.c_float(jit[p, 0]), C.c_float(jit[p, 1]), C.byref(q)) == 0
            out[k] = buf
            k += 1
    return out


class Expected:
    """One frame of the oracle: radiance0 per pixel, every stream's state afterwards, the live counts."""

    def __init__(self, desc, cam, iterations, seed, width=W, height=H):
        o = oracle.Oracle(desc, width, height, max_iterations=iterations, seed=seed)
        o.set_camera(cam)
        o.generate_frame()
        self.radiance = o.last_radiance0()
        self.states = np.array([o.rng_state(p) for p in range(width * height)], dtype=np.uint32)
        self.live_counts = o.live_counts()
        o.close()


_EXPECTED = {}


def expected(name, iterations):
    """The oracle's frame for case (name, iterations); computed once per process (both placements share it)."""
    if (name, iterations) not in _EXPECTED:
        scene = make_scene(name)
        _EXPECTED[(name, iterations)] = Expected(scene.desc, camera_of(name), iterations, SCENES[name][3])
    return _EXPECTED[(name, iterations)]


def satisfies_identity_condition(live_counts, iterations):
    """The frame's loop guard never fired: every iteration ran, each entered by more than 128 rays."""
    return len(live_counts) == iterations and bool((np.asarray(live_counts) > 128).all())


# ---- the mesh case in a new pose (ptss_update_triangles + ptss_resort_triangles) ------------------------------------------------------
MOVED_FIRST = 16   # the icosphere's triangles follow the box's sixteen


def moved_mesh():
    """(the "mesh" case's scene, its icosphere's triangles in a new pose: rotated, scaled and wobbled by scene_update_common.deform)."""
    scene = make_scene("mesh")
    return scene, deform(scene.triangles[MOVED_FIRST:])


def expected_moved(iterations):
    """The oracle's frame of the "mesh" case built on the new pose."""
    if ("moved", iterations) not in _EXPECTED:
        scene, moved = moved_mesh()
        posed = scene.with_triangles(np.concatenate([scene.triangles[:MOVED_FIRST], moved]))
        _EXPECTED[("moved", iterations)] = Expected(posed.desc, camera_of("mesh"), iterations, SCENES["mesh"][3])
    return _EXPECTED[("moved", iterations)]
