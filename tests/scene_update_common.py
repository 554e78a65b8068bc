"""Scenes and the deformation shared by tests/test_scene_update_cpu.py and tests/test_gpu_scene_update.py: triangle tables built
with numpy (ptss.TRIANGLE_DTYPE) and wrapped as scene descriptions on top of a preset's materials."""
import ctypes as C

import numpy as np

import ptss
from meshgen import icosphere
from ptss_types import PointLight, SceneDesc, Sphere, Triangle

WHITE, RED, GREEN, MIRROR = 2, 3, 4, 6   # materials of the "cornell" preset


def triangles_of(v0, v1, v2, material, normals=None):
    """(n,) TRIANGLE_DTYPE from three (n, 3) vertex arrays; normals: (n, 3, 3) or None for the face normal."""
    v0, v1, v2 = (np.asarray(x, dtype=np.float32).reshape(-1, 3) for x in (v0, v1, v2))
    t = np.zeros(len(v0), dtype=ptss.TRIANGLE_DTYPE)
    t["vertex0"], t["vertex1"], t["vertex2"] = v0, v1, v2
    if normals is None:
        n = np.cross((v1 - v0).astype(np.float64), (v2 - v0).astype(np.float64))
        n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
        normals = np.repeat(n[:, None, :], 3, axis=1)
    normals = np.asarray(normals, dtype=np.float32)
    t["normal0"], t["normal1"], t["normal2"] = normals[:, 0], normals[:, 1], normals[:, 2]
    t["materialIdx"] = material
    return t


def icosphere_triangles(level, centre, radius, material):
    v, f = icosphere(level)
    p = (np.asarray(centre) + radius * v).astype(np.float32)
    return triangles_of(p[f[:, 0]], p[f[:, 1]], p[f[:, 2]], material, normals=v[f])


def grid_triangles(corner, u, v, nu, nv, material):
    corner, u, v = (np.asarray(x, dtype=np.float64) for x in (corner, u, v))
    a, b, c = [], [], []
    for j in range(nv):
        for i in range(nu):
            p00, p10 = corner + u * (i / nu) + v * (j / nv), corner + u * ((i + 1) / nu) + v * (j / nv)
            p11, p01 = corner + u * ((i + 1) / nu) + v * ((j + 1) / nv), corner + u * (i / nu) + v * ((j + 1) / nv)
            a += [p00, p00]
            b += [p10, p11]
            c += [p11, p01]
    return triangles_of(a, b, c, material)


def preset_triangles(preset="cornell"):
    s = ptss.Scene(preset)
    return np.frombuffer(C.string_at(s.desc.triangles, s.desc.numTriangles * C.sizeof(Triangle)), dtype=ptss.TRIANGLE_DTYPE).copy()


class TableScene:
    """A scene description over numpy tables: the materials (and, unless replaced, spheres and lights) of a preset."""

    def __init__(self, triangles, preset="cornell", spheres=None, point_lights=None, keep_area_lights=True):
        self._base = ptss.Scene(preset)
        b = self._base.desc
        self.triangles = np.ascontiguousarray(triangles, dtype=ptss.TRIANGLE_DTYPE)
        self._tri = (Triangle * len(self.triangles)).from_buffer_copy(self.triangles.tobytes())
        d = SceneDesc()
        d.materials, d.numMaterials, d.defaultColor = b.materials, b.numMaterials, b.defaultColor
        d.triangles, d.numTriangles = self._tri, len(self.triangles)
        if spheres is None:
            d.spheres, d.numSpheres = b.spheres, b.numSpheres
        else:
            self._sph = (Sphere * len(spheres))()
            for k, (x, y, z, r, m) in enumerate(spheres):
                self._sph[k].position.x, self._sph[k].position.y, self._sph[k].position.z = x, y, z
                self._sph[k].radius, self._sph[k].materialIdx = r, m
            d.spheres, d.numSpheres = self._sph, len(spheres)
        if point_lights is None:
            d.pointLights, d.numPointLights = b.pointLights, b.numPointLights
        else:
            self._pl = (PointLight * len(point_lights))()
            for k, (pos, power) in enumerate(point_lights):
                self._pl[k].position.x, self._pl[k].position.y, self._pl[k].position.z = pos
                self._pl[k].power.x, self._pl[k].power.y, self._pl[k].power.z = power
            d.pointLights, d.numPointLights = self._pl, len(point_lights)
        if keep_area_lights:
            d.areaLights, d.numAreaLights = b.areaLights, b.numAreaLights
        self.desc = d

    def with_triangles(self, triangles):
        """The same scene around another triangle table."""
        s = TableScene.__new__(TableScene)
        s.__dict__.update(self.__dict__)
        s.triangles = np.ascontiguousarray(triangles, dtype=ptss.TRIANGLE_DTYPE)
        s._tri = (Triangle * len(s.triangles)).from_buffer_copy(s.triangles.tobytes())
        d = SceneDesc()
        C.memmove(C.byref(d), C.byref(self.desc), C.sizeof(SceneDesc))
        d.triangles, d.numTriangles = s._tri, len(s.triangles)
        s.desc = d
        return s


LIGHT = [((0.0, 3.0, -4.0), (300.0, 300.0, 300.0))]


def m530():
    """Icosphere level 2 (320) + a 15 x 7 grid (210), inside the Cornell box's volume: 34 leaves, the last of 2 triangles, and 3
    groups, the last of 18 triangles (one padded row in the group trip). Lit by a point light (the box's own emitter is not there)."""
    t = np.concatenate([icosphere_triangles(2, (0.3, -2.0, -5.0), 1.6, GREEN), grid_triangles((-4, -3.9, -1), (8, 0, 0), (0, 0, -7), 15, 7, WHITE)])
    assert len(t) == 530
    return TableScene(t, point_lights=LIGHT, keep_area_lights=False)


def m1296():
    """The Cornell box's 14 triangles and one more rectangle (16), then an icosphere of level 3 (1,280): 6 groups, two trips of
    the group mask. The box's area light keeps its triangle indices (12, 13)."""
    shelf = grid_triangles((-3, -1, -6), (2, 0, 0), (0, 0, -1.5), 1, 1, RED)
    t = np.concatenate([preset_triangles(), shelf, icosphere_triangles(3, (0.5, -2.2, -4.8), 1.5, MIRROR)])
    assert len(t) == 1296
    return TableScene(t)


def p300():
    """300 triangles: neither edge-classed (T > 255) nor a mesh image (T < 512) — the caller's order."""
    t = np.concatenate([preset_triangles(), grid_triangles((-3, -2, -2), (6, 0, 0), (0, 1, -5), 11, 13, GREEN)])
    assert len(t) == 300
    return TableScene(t)


def seventy_spheres(triangles, **kw):
    """70 spheres in a lattice (the many-sphere image, two images per context) around a triangle table."""
    sph = [(-3.0 + 0.9 * (k % 7), -3.2 + 0.8 * ((k // 7) % 5), -3.0 - 1.2 * (k // 35), 0.3, (WHITE, RED, GREEN, MIRROR)[k % 4]) for k in range(70)]
    return TableScene(triangles, spheres=sph, **kw)


def deform(t, phase=0.7):
    """Deformation D, in float32: a rotation about y, a non-uniform scale and a per-vertex sinusoidal wobble about the table's
    centre; the normals are rotated. Returns a new table."""
    out = t.copy()
    c, s = np.float32(np.cos(phase)), np.float32(np.sin(phase))
    centre = np.float32(0.5) * (t["vertex0"].min(axis=0) + t["vertex0"].max(axis=0))
    scale = np.array([1.1, 0.85, 1.05], dtype=np.float32)
    for name in ("vertex0", "vertex1", "vertex2"):
        p = t[name] - centre
        q = np.stack([c * p[:, 0] + s * p[:, 2], p[:, 1], c * p[:, 2] - s * p[:, 0]], axis=1) * scale
        q[:, 1] += np.float32(0.08) * np.sin(np.float32(3.0) * q[:, 0] + np.float32(phase)).astype(np.float32)
        out[name] = (q + centre).astype(np.float32)
    for name in ("normal0", "normal1", "normal2"):
        n = t[name]
        out[name] = np.stack([c * n[:, 0] + s * n[:, 2], n[:, 1], c * n[:, 2] - s * n[:, 0]], axis=1).astype(np.float32)
    return out


def stored(t):
    """(n, 9) float32 {v0, e1, e2} of a triangle table, as the image stores them (the same float subtractions)."""
    return np.concatenate([t["vertex0"], t["vertex1"] - t["vertex0"], t["vertex2"] - t["vertex0"]], axis=1).astype(np.float32)
