"""The scene image, on the host (csrc/ptpack.h through ptss.probe_pack_scene; no device).

Bytes: every image of every scene of tests/pack_scene_common.py reproduces the SHA-256 of (SceneLayout bytes, blob bytes) kept in
tests/golden/pack_scene.json, which the packer of the commit before ptpack.h existed produced in the hipcc host build — the probe
is the g++ build, so the two compilers are pinned to the same bits.

Structure: what a kernel relies on when it reads an image, checked from the decoded layout and the rows — the triangle
positions and class begins, the area lights' stored positions, the many-sphere tables and the containment of the chunk balls,
the mesh image's bounds and where its leaves live, the thresholds between the image kinds, and the padding."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import ptss
import pack_scene_common as pc

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pack_scene.json")))["digests"]
CASES = sorted(GOLDEN)   # "scene/every<0|1>/image<0|1>"

# csrc/ptscene.h: rows of the LDS work area behind the staged image — 4 of block scratch, then per wave (4 of 256 threads) the
# shadow-ray queue of 2 lights x 64 lanes: 8 planes of words and the answers as bytes
WORK_AREA_ROWS = 4 + 4 * (8 * 128 + 128 // 4) // 4
LDS_BYTES = 64 * 1024
# csrc/ptpack.h: stored chunk bound = R^2 (1 + m)^3 (1 + 4e-6) / (1 - mu), m = 5e-3, mu = m + m^2, rounded up
ACCEL_M = 5e-3
CHUNK_INFLATION = (1 + ACCEL_M) ** 3 * (1 + 4e-6) / (1 - (ACCEL_M + ACCEL_M * ACCEL_M))


def split(case):
    name, every, image = case.split("/")
    return name, int(every[-1]), int(image[-1])


@functools.lru_cache(maxsize=None)
def packed(case):
    name, every, image = split(case)
    layout, blob, in_lds = ptss.probe_pack_scene(pc.scene(name), every_sphere_loop=bool(every), image=image)
    blob.setflags(write=False)
    return layout, blob, in_lds


def ints(blob, off, n):
    return blob.view(np.int32).reshape(-1)[4 * off:4 * off + n]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def stored_triangles(L, blob):
    """(T, 9) float32 {v0, e1, e2} in storage order."""
    rows = blob[L["offTri"]:L["offTri"] + 3 * L["numTriangles"], :3]
    return np.ascontiguousarray(rows.reshape(-1, 9))


def is_mesh(L):
    return not L["triClassed"] and L["numLeaves"] > 0


def test_the_golden_file_covers_every_image_of_every_scene():
    want = set()
    for name in pc.NAMES:
        for every in (0, 1):
            n = ptss.probe_pack_scene_images(pc.scene(name), bool(every))
            want |= {f"{name}/every{every}/image{i}" for i in range(n)}
    assert want == set(CASES)
    # the many-sphere scenes get two images unless every sphere is looped over, every other scene one
    assert {c for c in CASES if c.endswith("image1")} == {f"{n}/every0/image1" for n in ("stress", "s70", "rand1024")}


@pytest.mark.parametrize("case", CASES)
def test_bytes_match_the_parent_commits_packer(case):
    L, blob, _ = packed(case)
    raw = np.array([L[f] for f in ptss.SCENE_LAYOUT_FIELDS], dtype=np.uint32)
    assert hashlib.sha256(raw.tobytes() + blob.tobytes()).hexdigest() == GOLDEN[case]


@pytest.mark.parametrize("case", CASES)
def test_sizes_and_padding(case):
    L, blob, in_lds = packed(case)
    assert 0 <= L["ldsVec4"] <= L["totalVec4"] and blob.shape == (L["totalVec4"] + 1, 4)
    assert in_lds == ((L["ldsVec4"] + WORK_AREA_ROWS) * 16 <= LDS_BYTES)
    if not L["accelSpheres"]:   # plain sphere rows: padded to a multiple of four with zero rows
        S = L["numSpheres"]
        pad = blob[L["offSphere"] + S:L["offSphere"] + (S + 3) // 4 * 4]
        assert L["offSphereMat"] == L["offSphere"] + (S + 3) // 4 * 4 and not bits(pad).any()
        assert L["numChunks"] == 0 and L["offSphereOrig"] == 0 and L["offSpherePos"] == 0


@pytest.mark.parametrize("case", CASES)
def test_triangle_positions_keys_and_class_begins(case):
    L, blob, _ = packed(case)
    name, _, _ = split(case)
    T = L["numTriangles"]
    pos = ints(blob, L["offTriPos"], T)
    assert np.array_equal(np.sort(pos), np.arange(T))   # a permutation
    original = np.empty(T, dtype=np.int64)
    original[pos] = np.arange(T)
    keys = bits(blob[L["offTri"] + 1:L["offTri"] + 3 * T:3, 3])
    assert np.array_equal(keys, (0xFFFFFFFE - original).astype(np.uint32))
    table = pc.triangle_table(pc.scene(name).desc)
    assert np.array_equal(bits(blob[L["offTri"]:L["offTri"] + 3 * T:3, :3]), bits(table["vertex0"][original]))
    begins = np.array([L[f"triClassPack{k}"] for k in range(5)], dtype="<u4").view(np.uint8)[:17].astype(int)
    if L["triClassed"]:
        assert T <= 255 and np.all(np.diff(begins) >= 0) and begins[0] == 0 and begins[16] == T
        cls = np.zeros(T, dtype=np.int32)
        tri, n3 = stored_triangles(L, blob), np.zeros((T, 3), dtype=np.float32)
        f32p, lim, g, c = C.POINTER(C.c_float), np.ones(T, dtype=np.float32), np.zeros((T, 6), np.float32), np.zeros((T, 6), np.float32)
        assert ptss.host_lib().ptss_probe_triangle_forms(tri.ctypes.data_as(f32p), n3.ctypes.data_as(f32p), n3.ctypes.data_as(f32p),
                                                         lim.ctypes.data_as(f32p), 0, T, cls.ctypes.data_as(C.POINTER(C.c_int)),
                                                         g.ctypes.data_as(f32p), c.ctypes.data_as(f32p)) == 0
        by_position = np.searchsorted(begins[1:], np.arange(T), side="right")   # c with begin(c) <= position < begin(c + 1)
        assert np.array_equal(by_position, cls)
        for code in range(16):   # the caller's order inside a class
            assert np.all(np.diff(original[begins[code]:begins[code + 1]]) > 0)
    elif not is_mesh(L):
        assert not begins.any() and np.array_equal(pos, np.arange(T))   # the caller's order


@pytest.mark.parametrize("case", CASES)
def test_area_lights_hold_stored_positions(case):
    L, blob, _ = packed(case)
    d = pc.scene(split(case)[0]).desc
    pos = ints(blob, L["offTriPos"], L["numTriangles"])
    for i in range(L["numAreaLights"]):
        first = d.areaLights[i].triangleIdx
        rows = bits(blob[L["offAreaLight"] + 2 * i:L["offAreaLight"] + 2 * i + 2])
        assert rows[0, 3] == pos[first] and rows[1, 0] == pos[first + 1] and not rows[1, 1:].any()
    assert L["numAreaLights"] == d.numAreaLights


@pytest.mark.parametrize("case", [c for c in CASES if c.endswith("every0/image0") and split(c)[0] in ("stress", "s70", "rand1024")])
def test_many_sphere_tables_and_chunk_balls(case):
    L, blob, _ = packed(case)
    d = pc.scene(split(case)[0]).desc
    S, K = L["numSpheres"], L["numChunks"]
    assert L["accelSpheres"] == 1 and K == (S + 15) // 16 and L["ldsVec4"] <= L["offSphereMat"]
    orig, pos = ints(blob, L["offSphereOrig"], 16 * K), ints(blob, L["offSpherePos"], S)
    assert np.array_equal(np.sort(orig[:S]), np.arange(S))
    assert np.array_equal(orig[pos], np.arange(S)) and np.array_equal(pos[orig[:S]], np.arange(S))   # inverse on [0, S)
    rows = blob[L["offSphere"]:L["offSphere"] + 16 * K]
    assert np.all(orig[S:] == orig[S - 1]) and np.array_equal(bits(rows[S:]), np.broadcast_to(bits(rows[S - 1]), (16 * K - S, 4)))
    centre = np.array([[d.spheres[i].position.x, d.spheres[i].position.y, d.spheres[i].position.z] for i in range(S)], dtype=np.float32)
    radius = np.array([d.spheres[i].radius for i in range(S)], dtype=np.float32)
    assert np.array_equal(bits(rows[:, :3]), bits(centre[orig])) and np.array_equal(bits(rows[:, 3]), bits(radius[orig] * radius[orig]))
    assert np.array_equal(ints(blob, L["offSphereMat"], 16 * K), [d.spheres[int(i)].materialIdx for i in orig])
    bound = blob[L["offChunk"]:L["offChunk"] + K].astype(np.float64)
    R = np.sqrt(bound[:, 3] / CHUNK_INFLATION)   # the radius the stored bound was inflated from (or a little more: it was rounded up)
    c64, r64 = centre[orig].astype(np.float64).reshape(K, 16, 3), np.abs(radius[orig].astype(np.float64)).reshape(K, 16)
    reach = np.sqrt(((c64 - bound[:, None, :3]) ** 2).sum(axis=2)) + r64
    assert np.all(reach <= R[:, None])   # every member inside its chunk's ball
    assert not bits(blob[L["offChunk"] + K:L["offChunk"] + (K + 3) // 4 * 4]).any()   # the bound rows' padding


MESH_CASES = [f"{name}/every0/image0" for name in ("mesh", "m530", "m1296", "t512", "mesh_400mat")]   # (all of them: test_image_kinds_...)


@pytest.mark.parametrize("case", MESH_CASES)
def test_mesh_bounds_are_the_probes_and_leaves_live_where_they_fit(case):
    L, blob, _ = packed(case)
    assert is_mesh(L)
    T, leaves, groups = L["numTriangles"], L["numLeaves"], L["numGroups"]
    assert leaves == (T + 15) // 16 and groups == (leaves + 15) // 16 and L["reserved"] == 0
    tri = stored_triangles(L, blob)
    none = np.zeros((0, 3), dtype=np.float32)
    for off, count, span in ((L["offLeaf"], leaves, 16), (L["offGroup"], groups, 256)):
        for k in range(count):
            _, b = ptss.probe_mesh_bound(tri[span * k:span * (k + 1)], none, none)
            assert np.array_equal(bits(blob[off + 3 * k:off + 3 * k + 3]).reshape(12), bits(b)), (span, k)
    assert not bits(blob[L["offGroup"] + 3 * groups:L["offGroup"] + 3 * ((groups + 3) // 4 * 4)]).any()
    staged = L["offLeaf"] < L["ldsVec4"]
    rows_with_leaves = L["ldsVec4"] + (0 if staged else 3 * leaves)
    assert staged == ((rows_with_leaves + WORK_AREA_ROWS) * 16 <= LDS_BYTES)
    assert L["offTri"] >= L["ldsVec4"] and L["offTriPos"] >= L["ldsVec4"]   # the triangle tables stay in global memory


def test_image_kinds_and_their_thresholds():
    kind = {c: ("mesh" if is_mesh(packed(c)[0]) else "accel" if packed(c)[0]["accelSpheres"] else "classed" if packed(c)[0]["triClassed"] else "plain")
            for c in CASES}
    assert [kind[f"t{n}/every0/image0"] for n in pc.THRESHOLDS] == ["classed", "plain", "plain", "mesh"]
    assert [kind[f"t{n}/every1/image0"] for n in pc.THRESHOLDS] == ["classed", "plain", "plain", "plain"]
    assert sorted(c for c in CASES if kind[c] == "mesh") == sorted(MESH_CASES)
    assert all(kind[c.replace("every0", "every1")] == "plain" for c in MESH_CASES)
    for name in ("stress", "s70", "rand1024"):
        assert kind[f"{name}/every0/image0"] == "accel" and kind[f"{name}/every0/image1"] != "accel" and kind[f"{name}/every1/image0"] != "accel"
        assert np.array_equal(bits(packed(f"{name}/every0/image1")[1]), bits(packed(f"{name}/every1/image0")[1]))   # image 1 is the plain image
    assert kind["p300/every0/image0"] == "plain"
    # leaves staged in LDS where they fit, in global memory where only the rest does
    assert packed("mesh/every0/image0")[0]["offLeaf"] < packed("mesh/every0/image0")[0]["ldsVec4"]
    L, _, in_lds = packed("mesh_400mat/every0/image0")
    assert in_lds and L["offLeaf"] >= L["ldsVec4"]
    # a NaN vertex or a coordinate of 2e15: neither bounded nor a mesh image, the caller's order, no fast reciprocal
    for name in ("nan_vertex", "huge_vertex"):
        L = packed(f"{name}/every0/image0")[0]
        assert kind[f"{name}/every0/image0"] == "plain" and L["numTriangles"] == 530
        assert (L["sphereBounded"], L["neePairs"], L["triClassed"]) == (0, 0, 0)
    assert packed("nan_vertex/every0/image0")[0]["triDetBounded"] == 0 and packed("m530/every0/image0")[0]["sphereBounded"] == 1


def test_argument_errors():
    H, d = ptss.host_lib(), pc.scene("cornell").desc
    n, words, raw = C.c_int(), C.c_size_t(), (C.c_ubyte * 140)()
    call = H.ptss_probe_pack_scene
    assert call(None, 0, 0, None, None, None, 0, None, 0, None) == -1
    assert call(C.byref(d), 2, 0, None, None, None, 0, None, 0, None) == -1
    assert call(C.byref(d), 0, 1, C.byref(n), None, None, 0, None, 0, None) == -1 and n.value == 1   # one image only
    assert call(C.byref(d), 0, -1, None, None, None, 0, None, 0, None) == -1
    assert call(C.byref(d), 0, 0, None, None, raw, 139, None, 0, None) == -1
    assert call(C.byref(d), 0, 0, None, None, raw, 140, None, 0, C.byref(words)) == 0 and words.value == 4 * 256
    small = np.zeros(words.value - 1, dtype=np.float32)
    assert call(C.byref(d), 0, 0, None, None, None, 0, small.ctypes.data_as(C.POINTER(C.c_float)), small.size, C.byref(words)) == -1
    assert words.value == 4 * 256
    bad = pc.TableScene(pc.preset_triangles())
    bad.desc.numAreaLights, bad.desc.numTriangles = 1, 13   # the box's light names triangles 12 and 13
    assert call(C.byref(bad.desc), 0, 0, None, None, None, 0, None, 0, None) == -1
