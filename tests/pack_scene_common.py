"""The scenes tests/test_pack_scene.py packs (csrc/ptpack.h through ptss.probe_pack_scene), by name; tests/golden/pack_scene.json
holds a digest for every (scene, everySphereLoop, image) of them."""
import functools
import pathlib
import tempfile

import numpy as np

import ptss
from meshgen import strip_obj, write
from scene_update_common import GREEN, LIGHT, MIRROR, RED, WHITE, TableScene, m1296, m530, p300, preset_triangles, seventy_spheres

PRESETS = ("default", "cornell", "lambert", "mixed", "stress", "mesh", "pointlight")
THRESHOLDS = (255, 256, 511, 512)


def strip_scene(total):
    """The 'cornell' preset (14 triangles) and a strip across the back of the box: `total` triangles, as tests/test_gpu_mesh.py's
    threshold cases build them."""
    s = ptss.Scene("cornell")
    with tempfile.TemporaryDirectory() as tmp:
        s.add_obj(write(pathlib.Path(tmp), "strip.obj", strip_obj(total - 14)), material=GREEN)
    assert s.desc.numTriangles == total
    return s


def random_spheres(n=1024, seed=1024):
    """n spheres drawn inside the Cornell box's volume around the preset's triangles: 64 chunks, so the pairwise refinement runs."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform((-3.6, -3.6, -7.6), (3.6, 3.6, -0.4), size=(n, 3)).astype(np.float32)
    rad = rng.uniform(0.05, 0.25, size=n).astype(np.float32)
    sph = [(float(p[0]), float(p[1]), float(p[2]), float(r), (WHITE, RED, GREEN, MIRROR)[k % 4]) for k, (p, r) in enumerate(zip(pos, rad))]
    return TableScene(preset_triangles(), spheres=sph)


def m530_with_vertex(value):
    """m530 with one coordinate replaced: 530 triangles that fail the bounded-geometry and the mesh gates."""
    t = m530().triangles.copy()
    t["vertex1"][77, 1] = value
    return TableScene(t, point_lights=LIGHT, keep_area_lights=False)


def mesh_with_materials(extra):
    """The 'mesh' preset with `extra` more materials: 400 leave room in LDS for everything staged but the leaf bounds."""
    from ptss_types import Material
    s = ptss.Scene("mesh")
    mats = (Material * (s.desc.numMaterials + extra))(*s.materials, *([s.materials[WHITE]] * extra))
    s.desc.materials, s.desc.numMaterials = mats, len(mats)
    s._keep = mats
    return s


_BUILDERS = {p: functools.partial(ptss.Scene, p) for p in PRESETS}
_BUILDERS.update({"m530": m530, "m1296": m1296, "p300": p300, "s70": lambda: seventy_spheres(preset_triangles())})
_BUILDERS.update({f"t{n}": functools.partial(strip_scene, n) for n in THRESHOLDS})
_BUILDERS.update({"rand1024": random_spheres, "nan_vertex": lambda: m530_with_vertex(np.nan), "huge_vertex": lambda: m530_with_vertex(2e15),
                  "mesh_400mat": lambda: mesh_with_materials(400)})
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return _BUILDERS[name]()


def triangle_table(desc):
    """(T,) ptss.TRIANGLE_DTYPE copy of a description's triangles."""
    import ctypes as C
    from ptss_types import Triangle
    return np.frombuffer(C.string_at(desc.triangles, desc.numTriangles * C.sizeof(Triangle)), dtype=ptss.TRIANGLE_DTYPE).copy()
