"""Scene::addObjModel (ptss_scene_add_obj, ptss.Scene.add_obj) against an independent numpy reading of the same OBJ text, its
error handling, and the "mesh" preset. No GPU."""
import json
import os

import numpy as np
import pytest

import ptss
from meshgen import icosphere_obj

HERE = os.path.dirname(os.path.abspath(__file__))

OBJ = """# every face form, comments, ignored statements
mtllib scene.mtl
o thing
g part
s 1
usemtl gold
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 0.5 1.5
v -1 -0.5 0.25 1.0
vt 0 0
vt 1 0
vt 1 1
vn 0 0 1
vn 0 1 0
vn 1 0 0
f 1 2 3
f 1/1 3/2 4/3
f 1//1 2//2 5//3
f 2/1/1 3/2/2 5/3/3
f -6 -5 -2            # relative indices: vertices 1 2 5
f -4//-3 -3//-2 -2//-1  # 3 4 5 with normals 1 2 3
f 1 2 3 4             # a quad: fan (1 2 3) (1 3 4)
f 6 1 2 3 5 4         # a hexagon: four triangles
"""


def numpy_parse(text, m):
    """An independent reading: positions by m, normals by inverse(m)^T, fan order, face normal where a face lacks normals."""
    v, vn, tris = [], [], []
    m = np.asarray(m, dtype=np.float64)
    nm = np.linalg.inv(m).T
    for line in text.replace("\r\n", "\n").split("\n"):
        line = line.split("#")[0].split()
        if not line:
            continue
        if line[0] == "v":
            v.append([float(x) for x in line[1:4]])
        elif line[0] == "vn":
            vn.append([float(x) for x in line[1:4]])
        elif line[0] == "f":
            idx = []
            for tok in line[1:]:
                parts = tok.split("/")
                i = int(parts[0])
                i = i - 1 if i > 0 else len(v) + i
                k = None
                if len(parts) == 3 and parts[2]:
                    k = int(parts[2])
                    k = k - 1 if k > 0 else len(vn) + k
                idx.append((i, k))
            for j in range(1, len(idx) - 1):
                c = [idx[0], idx[j], idx[j + 1]]
                p = [(m @ np.append(v[i], 1.0))[:3] for i, _ in c]
                if all(k is not None for _, k in c):
                    ns = []
                    for _, k in c:
                        n = (nm @ np.append(vn[k], 0.0))[:3]
                        ns.append(n / np.linalg.norm(n))
                else:
                    n = np.cross(p[1] - p[0], p[2] - p[0])
                    ns = [n / np.linalg.norm(n)] * 3
                tris.append((p, ns))
    return tris


def tri_arrays(scene, first):
    out = []
    for t in scene.triangles[first:]:
        p = [np.array([x.x, x.y, x.z], dtype=np.float64) for x in (t.vertex0, t.vertex1, t.vertex2)]
        n = [np.array([x.x, x.y, x.z], dtype=np.float64) for x in (t.normal0, t.normal1, t.normal2)]
        out.append((p, n, t.materialIdx))
    return out


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("transform", ["identity", "nonuniform"])
def test_loader_matches_an_independent_parse(tmp_path, crlf, transform):
    # exact in float: powers-of-two scales and small translations, so positions must match bit for bit
    m = np.eye(4) if transform == "identity" else np.array([[2, 0, 0, 0.5], [0, 0.5, 0, -1], [0, 0, 4, 2], [0, 0, 0, 1]], dtype=np.float64)
    text = OBJ.replace("\n", "\r\n") if crlf else OBJ
    path = tmp_path / "model.obj"
    path.write_bytes(text.encode())
    s = ptss.Scene("cornell")
    before = s.desc.numTriangles
    added = s.add_obj(str(path), transform=None if transform == "identity" else m, material=3)
    want = numpy_parse(OBJ, m)
    assert added == len(want) == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 4
    got = tri_arrays(s, before)
    assert len(got) == len(want)
    for (p, n, mat), (wp, wn) in zip(got, want):
        assert mat == 3
        for a, b in zip(p, wp):
            assert np.array_equal(a, b.astype(np.float32).astype(np.float64))
        for a, b in zip(n, wn):
            assert np.allclose(a, b, atol=2e-7), (a, b)
    # a face without normals wears its face normal on all three vertices; one with normals keeps them apart
    assert np.array_equal(got[0][1][0], got[0][1][2])
    assert not np.array_equal(got[2][1][0], got[2][1][2])


def test_negative_indices_and_fan_order(tmp_path):
    path = tmp_path / "fan.obj"
    path.write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv -1 1 0\nf -5 -4 -3 -2 -1\n")
    s = ptss.Scene("cornell")
    before = s.desc.numTriangles
    assert s.add_obj(str(path)) == 3
    corners = [[(t.vertex0.x, t.vertex0.y), (t.vertex1.x, t.vertex1.y), (t.vertex2.x, t.vertex2.y)] for t in s.triangles[before:]]
    assert corners == [[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)], [(0, 0), (0, 1), (-1, 1)]]


@pytest.mark.parametrize("text", [
    "v 0 0 0\nv 1 0 0\nf 1 2 6\n",            # vertex index out of range
    "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n",   # index 0 does not exist
    "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 -7\n",  # relative index before the first vertex
    "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 3//1\n",   # no normal 1
    "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/1 2/1 3/1\n",      # no texture coordinate 1
    "v 0 0\n",                                # too few coordinates
    "v 0 0 x\n",                              # not a number
    "v 0 0 inf\n",                            # not finite
    "v 0 0 0\nv 1 0 0\nf 1 2\n",              # two vertices
    "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3/1/1/1\n",  # too many slashes
    "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3a\n",  # trailing garbage
    "v 0 0 0\nl 1 2\n",                       # an unsupported statement
])
def test_bad_input_is_rejected_and_leaves_the_scene_unchanged(tmp_path, text):
    path = tmp_path / "bad.obj"
    # a valid prefix first: the error comes after triangles have been read, and none of them may stay
    path.write_text("v 5 5 5\nv 6 5 5\nv 5 6 5\nf 1 2 3\n" + text)
    s = ptss.Scene("cornell")
    before = s.table()
    with pytest.raises(ptss.PtssError):
        s.add_obj(str(path))
    assert s.table() == before


def test_missing_file_and_bad_material_return_their_codes(tmp_path):
    import ctypes as C
    s = ptss.Scene("cornell")
    L = ptss.host_lib()
    n = C.c_size_t(7)
    assert L.ptss_scene_add_obj(s._h, str(tmp_path / "nope.obj").encode(), None, 0, C.byref(n)) == -2   # PTSS_HOST_EIO
    good = tmp_path / "ok.obj"
    good.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert L.ptss_scene_add_obj(s._h, str(good).encode(), None, s.desc.numMaterials, C.byref(n)) == -1   # PTSS_HOST_EINVAL
    assert L.ptss_scene_add_obj(s._h, str(good).encode(), None, -1, C.byref(n)) == -1
    assert n.value == 7 and s.desc.numTriangles == ptss.Scene("cornell").desc.numTriangles
    assert L.ptss_scene_add_obj(s._h, str(good).encode(), None, 0, C.byref(n)) == 0 and n.value == 1


def test_mesh_preset_is_deterministic_and_the_pinned_presets_are_unchanged():
    a, b = ptss.Scene("mesh"), ptss.Scene("mesh")
    assert a.desc.numTriangles == 14 + 20 * 4 ** 4 and a.desc.numSpheres == 0
    assert a.table() == b.table()
    # the Cornell box of the preset, then the icosphere's triangles: unit normals, vertices on the sphere
    tris = a.triangles[14:]
    c = np.array([0.5, -2.5, -5.5])
    for t in tris[::97]:
        for v, n in ((t.vertex0, t.normal0), (t.vertex1, t.normal1), (t.vertex2, t.normal2)):
            p = np.array([v.x, v.y, v.z]) - c
            assert abs(np.linalg.norm(p) - 1.5) < 1e-5
            assert abs(np.linalg.norm([n.x, n.y, n.z]) - 1) < 1e-6
    from test_scene import hexify
    with open(os.path.join(HERE, "golden", "scenes.json")) as f:
        pinned = json.load(f)
    for name in ("default", "cornell", "lambert", "mixed", "pointlight"):
        assert hexify(ptss.Scene(name).table()) == pinned[name], name


def test_icosphere_obj_round_trip_equals_the_preset_builder(tmp_path):
    # the same subdivision written as OBJ and read back: the same number of triangles, closed surface (every edge twice)
    path = tmp_path / "ico.obj"
    path.write_text(icosphere_obj(3))
    s = ptss.Scene("cornell")
    before = s.desc.numTriangles
    assert s.add_obj(str(path)) == 1280
    edges = {}
    for t in s.triangles[before:]:
        vs = [(t.vertex0.x, t.vertex0.y, t.vertex0.z), (t.vertex1.x, t.vertex1.y, t.vertex1.z), (t.vertex2.x, t.vertex2.y, t.vertex2.z)]
        for k in range(3):
            e = tuple(sorted((vs[k], vs[(k + 1) % 3])))
            edges[e] = edges.get(e, 0) + 1
    assert set(edges.values()) == {2}
