"""Scenes for the range-guard tests (test_guard_ranges.py on the CPU, test_gpu_guard_scenes.py on the GPU): the 'mixed' preset's
materials with chosen overrides, a floor, two blockers and lights whose powers and positions are the test's to pick."""
import ctypes as C

import numpy as np

import ptss
from ptss_types import AreaLight, Material, PointLight, SceneDesc, Sphere, Triangle

CREAM, RED, GREEN, EMIT, MIRROR, GLASS, COOK, PHONG = 8, 9, 10, 11, 12, 3, 0, 6  # material classes of the 'mixed' preset
GUARD_POWERS, GUARD_REFRACTION, GUARD_EXPONENT = 1, 2, 4                          # bits of ptss_guard_flags


def _set3(v, xyz):
    v.x, v.y, v.z = (float(t) for t in xyz)


def build(spheres=(), triangles=(), area=(), point=(), ior=None, exponent=None):
    """spheres: (centre, radius, material); triangles: (v0, v1, v2, material); area: (power, firstTriangle); point: (position,
    power). ior / exponent: {material index: value} written over the 'mixed' preset's materials."""
    base = ptss.Scene("mixed")
    mats = (Material * base.desc.numMaterials)(*base.materials)
    for m, v in (ior or {}).items():
        mats[m].indexOfRefraction = float(v)
    for m, v in (exponent or {}).items():
        mats[m].specularExponent = float(v)
    sph = (Sphere * max(1, len(spheres)))()
    for i, (c, r, m) in enumerate(spheres):
        _set3(sph[i].position, c)
        sph[i].radius, sph[i].materialIdx = float(r), m
    tri = (Triangle * max(1, len(triangles)))()
    for i, (a, b, c, m) in enumerate(triangles):
        a, b, c = (np.asarray(t, np.float32) for t in (a, b, c))
        with np.errstate(all="ignore"):
            n = np.cross(b - a, c - a).astype(np.float32)
            ln = np.float32(np.sqrt(np.dot(n, n)))
            n = n / ln if 0 < ln < np.inf else np.asarray([0, 1, 0], np.float32)
        for dst, src in ((tri[i].vertex0, a), (tri[i].vertex1, b), (tri[i].vertex2, c), (tri[i].normal0, n),
                         (tri[i].normal1, n), (tri[i].normal2, n)):
            _set3(dst, src)
        tri[i].materialIdx = m
    al = (AreaLight * max(1, len(area)))()
    for i, (p, first) in enumerate(area):
        _set3(al[i].power, p)
        al[i].area, al[i].triangleIdx, al[i].numTriangles = 1.0, first, 2
    pl = (PointLight * max(1, len(point)))()
    for i, (pos, p) in enumerate(point):
        _set3(pl[i].position, pos)
        _set3(pl[i].power, p)
    d = SceneDesc()
    d.spheres, d.numSpheres = (sph if spheres else None), len(spheres)
    d.triangles, d.numTriangles = (tri if triangles else None), len(triangles)
    d.materials, d.numMaterials = mats, len(mats)
    d.areaLights, d.numAreaLights = (al if area else None), len(area)
    d.pointLights, d.numPointLights = (pl if point else None), len(point)

    class Holder:
        pass
    h = Holder()
    h.desc, h.keep = d, (sph, tri, mats, al, pl, base)
    return h


def quad(p0, p1, p2, p3, m):
    return [(p0, p1, p2, m), (p0, p2, p3, m)]


def host_guard_flags(scene):
    """What ptss_create will decide for this scene (the classifier itself, no GPU)."""
    out = C.c_uint()
    assert ptss.host_lib().ptss_probe_scene_guard_flags(C.byref(scene.desc), C.byref(out)) == 0
    return out.value


# a room every guard scene shares: floor, back wall, a lamp quad (area lights sample it), one sphere of each scattering class
FLOOR = quad((-4, -1, 0), (4, -1, 0), (4, -1, -9), (-4, -1, -9), CREAM)
WALL = quad((-4, -1, -9), (4, -1, -9), (4, 4, -9), (-4, 4, -9), GREEN)
LAMP = quad((-1, 3, -3), (1, 3, -3), (1, 3, -5), (-1, 3, -5), EMIT)
BALLS = [((-2.2, -0.3, -5.0), 0.7, GLASS), ((-0.7, -0.4, -4.2), 0.6, PHONG), ((0.8, -0.4, -5.2), 0.6, COOK),
         ((2.2, -0.3, -4.4), 0.7, MIRROR), ((0.1, -0.6, -3.0), 0.4, RED)]


def room(area_powers=((60, 60, 60),), point=(), **materials):
    """LAMP comes first (triangles 0 and 1): every area light samples it."""
    return build(spheres=BALLS, triangles=LAMP + FLOOR + WALL, area=[(p, 0) for p in area_powers], point=point, **materials)
