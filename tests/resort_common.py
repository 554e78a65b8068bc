"""Scenes and poses shared by tests/test_resort_cpu.py and tests/test_gpu_resort.py (ptss_resort_triangles): triangle
tables of given sizes, the hand-built tables whose centroids tie, and the pose that scatters every triangle."""
import numpy as np

import ptss
from scene_update_common import GREEN, LIGHT, MIRROR, RED, WHITE, TableScene, grid_triangles, icosphere_triangles, preset_triangles, triangles_of


def wavy_grid(nu, nv, material=WHITE):
    """2 nu nv triangles: a floor-sized rectangle inside the Cornell box's volume with a sinusoidal height."""
    t = grid_triangles((-4, -3.0, -1), (8, 0, 0), (0, 0, -7), nu, nv, material)
    for name in ("vertex0", "vertex1", "vertex2"):
        p = t[name]
        p[:, 1] += (np.float32(0.4) * np.sin(np.float32(2.5) * p[:, 0]) * np.cos(np.float32(1.7) * p[:, 2])).astype(np.float32)
        t[name] = p
    return triangles_of(t["vertex0"], t["vertex1"], t["vertex2"], material)


def table(T):
    """T triangles (T >= 512): the Cornell box's 14 — the area light's two are original indices 12 and 13 —, an icosphere, and a wavy
    grid cut to size."""
    parts = [preset_triangles(), icosphere_triangles(2, (0.5, -1.5, -4.8), 1.3, MIRROR)]
    have = sum(len(p) for p in parts)
    assert T >= have + 2
    nv = 12 if T < 6000 else 100
    nu = -(-(T - have) // (2 * nv))
    parts.append(wavy_grid(nu, nv, GREEN)[:T - have])
    t = np.concatenate(parts)
    assert len(t) == T
    return t


def mesh_scene(T):
    """The table with the Cornell preset's spheres, materials and box light (whose triangles belong to the mesh)."""
    return TableScene(table(T))


def point_lit(triangles):
    return TableScene(triangles, spheres=[], point_lights=LIGHT, keep_area_lights=False)


def lattice_through_zero(seed=3):
    """576 triangles whose centroids are the points of an 8 x 8 x 9 lattice, x = -30, -20, .., 40: every coordinate ties many times.
    Each triangle lies in its plane x = const, so its centroid's x is exactly that constant — and in the plane x = 0 the 36 triangles
    of highest original index carry x = -0.0, the other 36 x = +0.0. Sorted along x the cut at 256 of the 512-member segment falls
    inside that plane (members 216 .. 287), where the packer's comparator ties all 72 and lets the original index decide."""
    rng = np.random.default_rng(seed)
    ix, iy, iz = (a.reshape(-1) for a in np.meshgrid(np.arange(8), np.arange(8), np.arange(9), indexing="ij"))
    perm = rng.permutation(len(ix))
    c = np.stack([10.0 * (ix[perm] - 3), 1.0 * iy[perm], -1.0 * iz[perm] - 2.0], axis=1).astype(np.float32)
    zero = np.flatnonzero(c[:, 0] == 0)
    assert len(zero) == 72
    c[zero[36:], 0] = np.float32(-0.0)
    off = np.array([[0, 0.25, 0], [0, -0.25, 0.25], [0, 0, -0.25]], dtype=np.float32)
    v = [c + o for o in off]
    for p in v:   # (c + 0 turned -0.0 into +0.0)
        p[zero[36:], 0] = np.float32(-0.0)
    return triangles_of(v[0], v[1], v[2], WHITE)


def identical(n=600):
    one = np.array([[0.5, -1.0, -4.0], [1.5, -1.0, -4.0], [0.5, 0.0, -4.5]], dtype=np.float32)
    return triangles_of(*(np.repeat(one[k][None], n, axis=0) for k in range(3)), RED)


def flat(nu=20, nv=15):
    return grid_triangles((-4, -3.9, -1), (8, 0, 0), (0, 0, -7), nu, nv, WHITE)


def scatter(t, seed=11, keep=()):
    """The pose that permutes the triangles' places: triangle i takes the place (vertices and normals) of triangle perm[i], its
    material staying. `keep`: original indices that stay where they are."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(t))
    out = t[perm].copy()
    out["materialIdx"] = t["materialIdx"]
    for i in keep:
        out[i] = t[i]
    return out


def leaf_of(position):
    """Leaf number of every original index."""
    return np.asarray(position) // 16


def packer_positions(scene):
    L, blob, _ = ptss.probe_pack_scene(scene)
    assert L["numLeaves"] > 0, "not a mesh image"
    n = scene.desc.numTriangles
    return blob.view(np.int32).reshape(-1)[4 * L["offTriPos"]:4 * L["offTriPos"] + n].copy()
