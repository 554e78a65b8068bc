"""The host mirror's scene presets (cuda-path-tracer-ss_amd/host/Scene.cpp) against the reference's own Scene class, compiled for
the CPU and run: Scene::build() as committed against the preset "default", and addDefinedSpheres(4) + addCornellBox(8) (the scene of
the reference's image.tga) against "cornell". Every material, sphere, triangle, area light and point light: integers and flags
equal, floats under the rule of tests/reference_common.py with a float64 model of the reference's construction.

The order in which a C++ compiler draws the three rand() coordinates of a random sphere is unspecified (they are arguments of one
constructor call, Scene.cpp:161, 219). The g++ build of the reference draws them RIGHT TO LEFT: its spheres are the preset
"default@rtl", not "default". That is a fact about g++; it pins nothing about the compiler the reference was built with."""
import numpy as np
import pytest

import ptss
import refprobe
from reference_common import check_floats, dot, f64, norm, require_reference

GPP_DRAWS_RIGHT_TO_LEFT = True   # what this test finds, stated: g++ evaluates vec3(rnd, rnd, rnd)'s arguments last to first


@pytest.fixture(scope="module")
def ref():
    return require_reference()


def _host(preset):
    sc = ptss.Scene(preset)
    return refprobe.scene_tables(sc.desc)


# ---- float64 model of the construction ------------------------------------------------------------------------------------------
def _lcg():
    state = 1
    while True:
        state = (state * 214013 + 2531011) & 0xFFFFFFFF
        yield (state >> 16) & 0x7FFF


def _sphere_model(right_to_left):
    """addRandomSpheres(5) then addRandomGlassSpheres(15), Scene.cpp:213-224, 155-166: rnd(x) = x * rand() / 32767 on an unseeded
    Microsoft rand(); two, then three draws thrown away per sphere; position arguments in either order; then the radius."""
    g = _lcg()
    out = []
    for count, burn in ((5, 2), (15, 3)):
        for _ in range(count):
            for _ in range(burn):
                next(g)
            d = [next(g) for _ in range(3)]
            if right_to_left:
                z, y, x = d
            else:
                x, y, z = d
            r = next(g)
            out.append((5.0 * x / 32767 - 2.5, 5.0 * y / 32767 - 2.5, 7.0 * z / 32767 - 9.0, 1.0 * r / 32767 + 0.2))
    return np.array(out)


def _mat(shift, degrees, axis, edge):
    """translate(shift) * rotate(degrees, axis) * scale(edge), glm's definitions, the angle through float32 radians."""
    t = np.eye(4)
    t[:3, 3] = shift
    r = np.eye(4)
    if degrees != 0.0:
        a = float(np.float32(degrees) * np.float32(0.01745329251994329576923690768489))
        c, s = np.cos(a), np.sin(a)
        x, y, z = axis
        r[:3, :3] = np.array([[c + (1 - c) * x * x, (1 - c) * x * y - s * z, (1 - c) * x * z + s * y],
                              [(1 - c) * y * x + s * z, c + (1 - c) * y * y, (1 - c) * y * z - s * x],
                              [(1 - c) * z * x - s * y, (1 - c) * z * y + s * x, c + (1 - c) * z * z]])
    return t @ r @ np.diag([edge, edge, edge, 1.0])


def _rectangle_model(m):
    """addRectangularModel, Scene.cpp:63-96: corners (i - .5, j - .5, 0, 1), triangles (0, 1, 2) and (3, 1, 2), one normal."""
    corner = [(m @ np.array([i - 0.5, j - 0.5, 0.0, 1.0]))[:3] for i in (0, 1) for j in (0, 1)]
    n = (np.linalg.inv(m.T) @ np.array([0.0, 0.0, 1.0, 0.0]))[:3]
    n = n / np.sqrt(n @ n)
    return [(corner[0], corner[1], corner[2], n), (corner[3], corner[1], corner[2], n)]


X, Y = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
F = lambda v: float(np.float32(v))   # noqa: E731  a float literal of the reference


def _walls(name):
    """(shift, degrees, axis, edge) per rectangle, lights last: the placements of Scene.cpp:252-293 (addCornellBox(8)) and
    Scene.cpp:323-370 (addMirrorBox(10))."""
    if name == "cornell":
        w, h = 8.0, 4.0
        return [((0, -h, -h), -90, X, w), ((0, h, -h), 90, X, w), ((-h, 0, -h), 90, Y, w), ((h, 0, -h), -90, Y, w),
                ((F(h - F(0.02)), 0, -h), -90, Y, w - 2), ((0, 0, -w), 0, Y, w), ((0, F(h - F(0.01)), -h), 90, X, 2.5)]
    w, h = 10.0, 5.0
    return [((0, -h, -h), -90, X, w), ((0, h, -h), 90, X, w), ((F(-h + 0.2 * h), 0, -h), 88, Y, w), ((h, 0, -h), -90, Y, w),
            ((0, 0, -w), 0, Y, w), ((0, 0, 0), 180, Y, w), ((0, F(h - F(0.01)), -h), 90, X, 2.5), ((0, F(-h + F(0.01)), -h), -90, X, 1.5)]


def _triangle_model(name):
    tris = []
    for shift, deg, axis, edge in _walls(name):
        tris += _rectangle_model(_mat(shift, deg, axis, edge))
    return tris


@pytest.mark.parametrize("kind,name", [(0, "default"), (1, "cornell")])
def test_scene_tables(ref, kind, name):
    r = ref.build_scene(kind)
    plain, rtl = _host(name), _host(name + "@rtl")

    # ---- counts, integers, flags: equal ------------------------------------------------------------------------------------------
    for table in ("spheres", "triangles", "materials", "pointLights", "areaLights"):
        assert len(r[table]) == len(plain[table]) == len(rtl[table]), table
    assert (len(r["spheres"]), len(r["triangles"]), len(r["materials"]), len(r["pointLights"]), len(r["areaLights"])) == \
        {"default": (20, 16, 12, 0, 2), "cornell": (2, 14, 7, 0, 1)}[name]
    assert np.array_equal(r["spheres"]["materialIdx"], plain["spheres"]["materialIdx"])
    assert np.array_equal(r["triangles"]["materialIdx"], plain["triangles"]["materialIdx"])
    assert np.array_equal(r["materials"]["flags"], plain["materials"]["flags"])
    assert np.array_equal(r["areaLights"]["triangleIdx"], plain["areaLights"]["triangleIdx"])
    assert np.array_equal(r["areaLights"]["numTriangles"], plain["areaLights"]["numTriangles"])

    # ---- materials: constants of the source, so bit for bit. roughness only where the reference's scene code assigns it (the
    # Cook-Torrance materials, Scene.cpp:199-210); elsewhere the reference leaves it unset and the mirror has 0
    for field in ("diffuseColor", "specularColor", "absorption", "emmitance", "specularExponent", "indexOfRefraction", "diffAvg", "specAvg",
                  "refrAvg"):
        assert np.array_equal(r["materials"][field].view(np.uint32), plain["materials"][field].view(np.uint32)), field
    assigned = (r["materials"]["flags"] & 3) == 3
    assert np.array_equal(r["materials"]["roughness"][assigned], plain["materials"]["roughness"][assigned])
    assert assigned.sum() == (3 if name == "default" else 0) and not plain["materials"]["roughness"][~assigned].any()
    assert np.array_equal(r["areaLights"]["power"].view(np.uint32), plain["areaLights"]["power"].view(np.uint32))

    # ---- spheres: one of the two argument orders, and this test says which ---------------------------------------------------------
    def sph4(t):
        return np.concatenate([t["spheres"]["position"], t["spheres"]["radius"][:, None]], axis=1)
    if name == "default":
        model_plain, model_rtl = _sphere_model(False), _sphere_model(True)
        assert not np.allclose(model_plain, model_rtl)
        is_rtl = np.allclose(sph4(r), model_rtl, atol=1e-5)
        is_plain = np.allclose(sph4(r), model_plain, atol=1e-5)
        assert is_rtl != is_plain, "the g++ build of the reference matches neither argument order"
        assert is_rtl == GPP_DRAWS_RIGHT_TO_LEFT
        host, model = (rtl, model_rtl) if is_rtl else (plain, model_plain)
        # the other preset is the same set of draws with x and z's draws exchanged: y and radius are shared
        other = plain if is_rtl else rtl
        assert np.array_equal(sph4(other)[:, [1, 3]], sph4(host)[:, [1, 3]]) and not np.array_equal(sph4(other), sph4(host))
        check_floats("Scene spheres [default]", sph4(r), sph4(host), model, floor=1.0)
    else:
        # addDefinedSpheres(4), Scene.cpp:107-108: no draws
        model = np.array([(-2, -(4 - 1.5), -(4 * F(1.3)), 1.5), (1, -(4 - 1.0), -(4 * F(1.4)), 1.0)])
        assert np.array_equal(sph4(plain), sph4(rtl))
        check_floats("Scene spheres [cornell]", sph4(r), sph4(plain), model, floor=1.0)

    # ---- triangles and lights ---------------------------------------------------------------------------------------------------------
    assert plain["triangles"].tobytes() == rtl["triangles"].tobytes()
    tris = _triangle_model(name)
    assert len(tris) == len(r["triangles"])
    verts = np.array([np.concatenate(t[:3]) for t in tris])
    normals = np.array([np.concatenate([t[3]] * 3) for t in tris])

    def cat(t, fields):
        return np.concatenate([t["triangles"][f] for f in fields], axis=1)
    # a vertex is a sum of products the size of the box: the floor is its half edge
    check_floats(f"Scene triangle vertices [{name}]", cat(r, ("vertex0", "vertex1", "vertex2")), cat(plain, ("vertex0", "vertex1", "vertex2")),
                 verts, floor=4.0 if name == "cornell" else 5.0)
    check_floats(f"Scene triangle normals [{name}]", cat(r, ("normal0", "normal1", "normal2")), cat(plain, ("normal0", "normal1", "normal2")),
                 normals, floor=1.0)
    # every normal is a unit vector that faces into the box; the three of a triangle are one vector
    n0 = f64(r["triangles"]["normal0"])
    assert np.abs(norm(n0) - 1).max() < 1e-6
    assert np.array_equal(r["triangles"]["normal0"], r["triangles"]["normal1"]) and np.array_equal(r["triangles"]["normal0"], r["triangles"]["normal2"])
    centre = np.array([0.0, 0.0, -4.0 if name == "cornell" else -5.0])
    mid = (f64(r["triangles"]["vertex0"]) + f64(r["triangles"]["vertex1"]) + f64(r["triangles"]["vertex2"])) / 3
    assert (dot(n0, centre - mid) > 0).all()
    # AreaLight::area, Scene.cpp:48-51: |e1 x e2| of the light's first triangle
    area = []
    for first in r["areaLights"]["triangleIdx"]:
        v0, v1, v2 = tris[first][:3]
        area.append(norm(np.cross(v1 - v2, v2 - v0)))
    check_floats(f"Scene light areas [{name}]", r["areaLights"]["area"], plain["areaLights"]["area"], np.array(area), floor=1.0, vector=False)


def test_g_plus_plus_order_is_stated(ref):
    """The sentence in this file's docstring, checked: the g++ build's spheres are bit for bit neither preset's or exactly one's."""
    r = ref.build_scene(0)
    plain, rtl = _host("default"), _host("default@rtl")
    same_plain = r["spheres"].tobytes() == plain["spheres"].tobytes()
    same_rtl = r["spheres"].tobytes() == rtl["spheres"].tobytes()
    print(f"[reference] g++ build of Scene::build(): spheres bit-equal to 'default': {same_plain}, to 'default@rtl': {same_rtl}")
    assert not same_plain
    assert same_rtl == GPP_DRAWS_RIGHT_TO_LEFT
