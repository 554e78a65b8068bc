"""Light maps read back, without a GPU (ptss_surface_atlas_blocks / ptss_lookup_lightmap): the record layouts against
the header, the exported symbols, the atlas with its blocks and sphere blocks, the host build of csrc/ptlightmap.h (the specification of
the device's rows) against a model in Python integers, exact rationals and numpy float32 (tests/lightmap_common.py), the properties the
lookup promises, and the sanitizers over a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from lightmap_common import (EMPTY, FILTERED, FILTERS, FLAGS, NO_BLOCK, REJECTED, affine_map, bad_block_rows, bad_hit_rows, hits_with_bad_rows,
                             make_hits, model_lookup, model_place, random_map, surfel_hits)
from surface_common import TRIANGLE, first_difference, same_bytes
from scene_update_common import triangles_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
UP = (0.0, 0.0, 1.0)


def lm_params(width, height, filter="bilinear", flags=(False, False), **kw):
    return ptss.lightmap_params(width, height, filter, modulate=flags[0], emission=flags[1], **kw)


@pytest.fixture(scope="module")
def mixed():
    """The "mixed" preset: (triangles, spheres, materials, atlas with blocks at 3 texels a unit into 96 columns)."""
    scene = ptss.Scene("mixed")
    tri, sph = ptss.scene_records(scene)
    assert len(tri) >= 12 and len(sph) >= 12
    return tri, sph, ptss.scene_materials(scene), ptss.surface_atlas_blocks(tri, sph, 3.0, 96, 1, 24)


def test_dtypes_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes and numpy mirrors."""
    block = ("x", "y", "width", "height")
    params = ("structSize", "atlasWidth", "atlasHeight", "filter", "flags", "firstTriangle", "numTriangleBlocks", "firstSphere", "numSphereBlocks", "reserved")
    material = ("diffuseColor", "specularColor", "absorption", "emmitance", "specularExponent", "indexOfRefraction", "diffAvg", "specAvg", "refrAvg",
                "roughness", "flags")
    body = "".join('printf("%%zu\\n", offsetof(ptss_surface_block, %s));' % f for f in block)
    body += "".join('printf("%%zu\\n", offsetof(ptss_lightmap_params, %s));' % f for f in params)
    body += "".join('printf("%%zu\\n", offsetof(ptss_material, %s));' % f for f in material)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { printf("%zu\\n%zu\\n%zu\\n", sizeof(ptss_surface_block), '
                   'sizeof(ptss_lightmap_params), sizeof(ptss_material)); ' + body +
                   ' printf("%d %d %u %u\\n", PTSS_LIGHTMAP_NEAREST, PTSS_LIGHTMAP_BILINEAR, PTSS_LIGHTMAP_MODULATE, PTSS_LIGHTMAP_EMISSION); return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    B, P, M = ptss.SURFACE_BLOCK_DTYPE, ptss_types.LightmapParams, ptss_types.MATERIAL_DTYPE
    assert got[:3] == [B.itemsize, C.sizeof(P), M.itemsize] == [16, 40, C.sizeof(ptss_types.Material)]
    assert got[3:7] == [B.fields[f][1] for f in block] == [0, 4, 8, 12]
    assert got[7:17] == [getattr(P, f).offset for f in params] == list(range(0, 40, 4))
    assert got[17:28] == [M.fields[f][1] for f in material]
    assert got[28:] == [ptss.LIGHTMAP_NEAREST, ptss.LIGHTMAP_BILINEAR, ptss.LIGHTMAP_MODULATE, ptss.LIGHTMAP_EMISSION] == [0, 1, 1, 2]


def test_libraries_export_the_symbols():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_lightmap_params", "ptss_lookup_lightmap", "ptss_lightmap_launches", "ptss_debug_lightmap_form"):
        assert hasattr(L, name), name
    for name in ("ptss_surface_atlas_blocks", "ptss_probe_lookup_lightmap"):
        assert hasattr(ptss.host_lib(), name), name
    p = ptss_types.LightmapParams()
    assert L.ptss_default_lightmap_params(C.byref(p)) == 0 and L.ptss_default_lightmap_params(None) == -1
    assert (p.structSize, p.atlasWidth, p.atlasHeight, p.filter, p.flags, p.reserved) == (40, 1, 1, ptss.LIGHTMAP_BILINEAR, 0, 0)
    assert (p.firstTriangle, p.numTriangleBlocks, p.firstSphere, p.numSphereBlocks) == (0, 0, 0, 0)
    q = ptss.lightmap_params(1, 1)
    assert bytes(p) == bytes(q)
    # refused before anything touches a device
    film = ptss.linear_params()
    assert L.ptss_lookup_lightmap(None, C.byref(p), C.byref(film), None, None, None, None, 0, None, None, None) == -1
    assert L.ptss_lightmap_launches(None, C.byref(C.c_ulonglong())) == -1 and L.ptss_debug_lightmap_form(None, 0) == -1


# ---- the atlas with blocks ------------------------------------------------------------------------------------------------------------
def test_the_atlas_blocks(mixed):
    tri, sph, _, (bt, bs, points, texels, height) = mixed
    W = 96
    # no spheres: ptss_surface_atlas' points, texels, height and count
    p0, t0, h0 = ptss.surface_atlas(tri, 3.0, W, 1, 24)
    b1, none, p1, t1, h1 = ptss.surface_atlas_blocks(tri, None, 3.0, W, 1, 24)
    assert len(none) == 0 and same_bytes(p0, p1) and same_bytes(t0, t1) and h0 == h1
    assert same_bytes(b1, bt) and same_bytes(points[:len(p0)], p0) and same_bytes(texels[:len(t0)], t0)   # the triangles come first
    # count-only equals filling
    assert ptss.surface_atlas_blocks(tri, sph, 3.0, W, 1, 24, fill=False) == (len(points), height)
    # every triangle point's texel is (y + j) * W + x + i of its block; i, j from the point itself: a = (3 i + 1) / (3 s)
    T = len(tri)
    tp = points["surface"] >= TRIANGLE
    assert tp[:len(p0)].all() and not tp[len(p0):].any()
    owner = points["surface"][tp] - TRIANGLE
    s = bt["width"][owner].astype(np.float64)
    assert (bt["width"] == bt["height"]).all() and (bt["width"] >= 1).all()
    i = np.rint((points["a"][tp].astype(np.float64) * 3 * s - 1) / 3).astype(np.int64)
    j = np.rint((points["b"][tp].astype(np.float64) * 3 * s - 1) / 3).astype(np.int64)
    assert np.array_equal(texels[tp], (bt["y"][owner] + j) * W + bt["x"][owner] + i)
    # spheres: h = clamp(ceil(pi r 3), 1, 24), w = 2 h, every texel of the block, rows bottom up, after the triangles
    at = len(p0)
    for k in range(len(sph)):
        want = np.float32(np.pi) * sph["radius"][k] * np.float32(3.0)
        h = int(min(max(np.ceil(want), 1), 24))
        assert (bs["width"][k], bs["height"][k]) == (2 * h, h), k
        mine = slice(at, at + 2 * h * h)
        jj, ii = np.divmod(np.arange(2 * h * h), 2 * h)
        assert (points["surface"][mine] == k).all() and (points["flags"][mine] == 0).all()
        assert np.array_equal(points["a"][mine], (ii.astype(np.float32) + np.float32(0.5)) / np.float32(2 * h))
        assert np.array_equal(points["b"][mine], (jj.astype(np.float32) + np.float32(0.5)) / np.float32(h))
        assert np.array_equal(texels[mine], (bs["y"][k] + jj) * W + bs["x"][k] + ii)
        at += 2 * h * h
    assert at == len(points) and len(set(texels.tolist())) == len(texels)
    assert len({int(h) for h in bs["height"]}) > 1   # the preset's spheres differ in size
    # every point is accepted by the generator's probe
    assert ptss.probe_surface_rays(tri, sph, points, np.zeros((len(points), 6), np.uint32), ptss.surface_params("normal"))[3] == 0
    # blocks are disjoint and at least one texel apart, spheres included, and inside the atlas
    blocks = [tuple(int(v) for v in b) for b in np.concatenate([bt, bs])]
    assert height == max(y + h for _, y, _, h in blocks) and all(x >= 0 and y >= 0 and x + w <= W for x, y, w, _ in blocks)
    for p, (xa, ya, wa, ha) in enumerate(blocks):
        for xb, yb, wb, hb in blocks[p + 1:]:
            assert xa + wa + 1 <= xb or xb + wb + 1 <= xa or ya + ha + 1 <= yb or yb + hb + 1 <= ya, (p, (xa, ya, wa, ha), (xb, yb, wb, hb))
    # a range of both tables names the caller's indices
    b2, s2, p2, _, _ = ptss.surface_atlas_blocks(tri, sph, 3.0, W, 1, 24, first_triangle=3, num_triangles=2, first_sphere=5, num_spheres=3)
    assert len(b2) == 2 and len(s2) == 3 and set(p2["surface"].tolist()) == {TRIANGLE | 3, TRIANGLE | 4, 5, 6, 7}
    # a radius that is not a number gives minSide
    odd = sph[:2].copy()
    odd["radius"] = (float("nan"), 1e30)
    _, s3, _, _, _ = ptss.surface_atlas_blocks(None, odd, 3.0, W, 2, 24)
    assert [tuple(b)[2:] for b in s3] == [(4, 2), (48, 24)]


def test_the_atlas_blocks_refuse(mixed):
    tri, sph = mixed[0], mixed[1]
    ok = dict(texels_per_unit=1.0, width=96, min_side=2, max_side=48)
    assert ptss.surface_atlas_blocks(tri, sph, fill=False, **ok)[0] > 0
    for bad in (dict(texels_per_unit=0.0), dict(texels_per_unit=float("nan")), dict(texels_per_unit=float("inf")), dict(min_side=0), dict(max_side=1),
                dict(max_side=4097), dict(max_side=97), dict(max_side=49)):   # the last: 2 * maxSide > atlasWidth with spheres
        with pytest.raises(ptss.PtssError):
            ptss.surface_atlas_blocks(tri, sph, **dict(ok, **bad))
    assert ptss.surface_atlas_blocks(tri, None, fill=False, **dict(ok, max_side=49))[0] > 0   # ... fine without them
    H = ptss.host_lib()
    made, height = C.c_size_t(), C.c_int()
    t, s = tri.ctypes.data_as(C.c_void_p), sph.ctypes.data_as(C.c_void_p)
    call = lambda tp=t, ft=0, nt=len(tri), sp=s, fs=0, ns=len(sph), made=C.byref(made), width=96: H.ptss_surface_atlas_blocks(
        tp, ft, nt, sp, fs, ns, 1.0, 2, 48, width, None, None, None, None, 0, C.byref(height), made)
    assert call() == 0
    assert call(tp=None) == -1 and call(sp=None) == -1 and call(made=None) == -1
    assert call(sp=None, ns=0) == 0 and call(tp=None, nt=0) == 0
    assert call(ft=1 << 30, nt=0) == -3 and call(fs=1 << 30, ns=0) == -3 and call(fs=(1 << 30) - 4, ns=5) == -3
    big = np.zeros(40000, dtype=ptss.SPHERE_DTYPE)   # 40,000 blocks of 96 x 48 in 96 columns: beyond 2^31 texels
    big["radius"] = 100.0
    assert call(sp=big.ctypes.data_as(C.c_void_p), ns=len(big), nt=0) == 0
    big = np.zeros(500000, dtype=ptss.SPHERE_DTYPE)
    big["radius"] = 100.0
    assert call(sp=big.ctypes.data_as(C.c_void_p), ns=len(big), nt=0) == -3


# ---- the probe against the model ------------------------------------------------------------------------------------------------------
SIDES = (1, 2, 3, 7, 64)


def side_triangles():
    """One triangle per side in SIDES at one texel a unit, one more that ends a shelf of 128 columns exactly, one that opens the next."""
    rows = [((0, 0, 0), (s, 0, 0), (0.5 * s, 0.125, 0)) for s in SIDES + (46, 17)]   # 1 + 2 + 3 + 7 + 64 + five gaps = 82, + 46 = 128
    v = np.array(rows, dtype=np.float32)
    return triangles_of(v[:, 0], v[:, 1], v[:, 2], 0, normals=np.tile(np.float32([0, 0, 1]), (len(v), 3, 1)))


def scattered_hits(tri_blocks, sph_blocks, count, seed, materials):
    """Hits all over both kinds of block: places inside, on the edges and outside (w beyond [0, 1]), every normal direction."""
    g = np.random.default_rng(seed)
    rows = []
    special = [0.0, 1.0, -0.25, 1.25, 0.5, 1e-3, 0.999, 1.0 / 3.0, 2.0 / 3.0]
    for k in range(count):
        m = int(g.integers(0, materials))
        if sph_blocks and k % 3 == 0:
            n = g.normal(size=3)
            n /= np.linalg.norm(n)
            if k % 15 == 0:
                n = [(0, 1, 0), (0, -1, 0), (-1e-7, 0, 1), (1e-7, 0, 1), (0, 0, 1), (0, 0, -1), (1, 0, 0)][(k // 15) % 7]   # poles, the seam
            rows.append((1, int(g.integers(0, sph_blocks)), 0.0, 0.0, tuple(n), m))
        else:
            w1 = special[int(g.integers(0, len(special)))] if k % 4 == 0 else float(g.random())
            w2 = special[int(g.integers(0, len(special)))] if k % 8 == 0 else float(g.random()) * (1.0 - min(max(w1, 0.0), 1.0))
            rows.append((2, int(g.integers(0, tri_blocks)), w1, w2, UP, m))
    return make_hits(rows)


@pytest.fixture(scope="module")
def sides():
    """Blocks of side 1, 2, 3, 7 and 64, one at a shelf's end, and three sphere blocks; a map with means above 2^48."""
    tri = side_triangles()
    sph = np.zeros(3, dtype=ptss.SPHERE_DTYPE)
    sph["radius"] = (0.3, 1.0, 5.0)
    W = 128
    bt, bs, points, texels, height = ptss.surface_atlas_blocks(tri, sph, 1.0, W, 1, 64)
    assert [int(b["width"]) for b in bt] == list(SIDES) + [46, 17]
    assert bt["x"][5] + bt["width"][5] == W and bt["y"][5] == 0 and bt["x"][6] == 0 and bt["y"][6] == 65   # a block at a shelf's end
    mat = np.zeros(3, dtype=ptss.MATERIAL_DTYPE)
    mat["diffuseColor"] = [(1.0, 0.0, 0.5), (0.25, 0.999, 1.0 / 3.0), (2.0, -1.0, float("nan"))]
    mat["emmitance"] = [(0.0, 0.0, 0.0), (1.5, 0.0, 70000.0), (float("nan"), -1.0, float("inf"))]
    return dict(tri=tri, sph=sph, W=W, H=height, bt=bt, bs=bs, points=points, texels=texels, mat=mat)


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("flags", FLAGS)
def test_the_probe_equals_the_model(sides, filter, flags):
    s = sides
    params = lm_params(s["W"], s["H"], filter, flags)
    hits = np.concatenate([scattered_hits(len(s["bt"]), len(s["bs"]), 400, 11, len(s["mat"])), surfel_hits(s["tri"], s["sph"], s["points"][::7])])
    for name, film in (("ordinary", random_map(s["W"], s["H"], s["texels"], 1, ones=0.2)),
                       ("above 2^48", random_map(s["W"], s["H"], s["texels"], 2, big=True, ones=0.2)),
                       ("filled", ptss.probe_dilate_linear(random_map(s["W"], s["H"], s["texels"], 3), s["W"], s["H"]))):
        got, info = ptss.probe_lookup_lightmap(s["mat"], hits, film, params, s["bt"], s["bs"])
        want, counts = model_lookup(s["mat"], hits, film, params, s["bt"], s["bs"])
        assert same_bytes(got, want), (name, first_difference(got, want))
        assert np.array_equal(info, counts) and info.sum() == len(hits), (name, info, counts)
        assert info[FILTERED] > 300 and (name == "filled" or info[EMPTY] > 0), (name, info)   # taps in the empty half, some with no other
        if name == "above 2^48":
            assert (got["r"][got["samples"] == 1] >> np.uint64(48)).any()
    # the counts are added to, info=False leaves them out
    again, info2 = ptss.probe_lookup_lightmap(s["mat"], hits, film, params, s["bt"], s["bs"], info=info)
    assert same_bytes(again, got) and np.array_equal(info2, 2 * info)
    assert ptss.probe_lookup_lightmap(s["mat"], hits, film, params, s["bt"], s["bs"], info=False)[1] is None


def test_the_seam_wraps_and_the_poles_clamp(sides):
    """A sphere block whose columns differ: a normal just left and just right of the seam (n.x = -+tiny, n.z = +1: longitude +-pi) blends
    the last and the first column; at the poles both rows are the edge row."""
    s = sides
    k = 2
    x, y, w, h = (int(v) for v in s["bs"][k])
    film = affine_map(s["W"], s["H"], (x, y, w, h), 1000, 16, 4096)
    params = lm_params(s["W"], s["H"], "bilinear")
    tiny = 1e-6
    hits = make_hits([(1, k, 0, 0, (-tiny, 0, 1), 0), (1, k, 0, 0, (tiny, 0, 1), 0), (1, k, 0, 0, (0, 1, 0), 0), (1, k, 0, 0, (0, -1, 0), 0)])
    got, info = ptss.probe_lookup_lightmap(None, hits, film, params, s["bt"], s["bs"])
    assert info[FILTERED] == 4
    mid = 1000 + 4096 * (h // 2 - 1) + 2048   # halfway between the two middle rows (h is even here)
    assert h % 2 == 0 and got["r"][0] == got["r"][1] == mid + 16 * (w - 1) // 2   # half of column w - 1, half of column 0
    lon0 = 1000 + 16 * (w // 2 - 1) + 8   # longitude 0 (n = (0, +-1, 0): atan2(0, -0) = 0): halfway between the middle columns
    assert got["r"][2] == lon0 + 4096 * (h - 1) and got["r"][3] == lon0
    want, _ = model_lookup(None, hits, film, params, s["bt"], s["bs"])
    assert same_bytes(got, want)


# ---- properties ----------------------------------------------------------------------------------------------------------------------
def own_point_hits(side):
    """The atlas' own points of one triangle block of `side`: (hits, i, j)."""
    j, i = np.nonzero(np.add.outer(np.arange(side), np.arange(side)) <= side - 1)
    hits = np.zeros(len(i), dtype=ptss.HIT_DTYPE)
    hits["kind"], hits["normal"] = 2, UP
    hits["w1"] = (3 * i + 1).astype(np.float32) / np.float32(3 * side)
    hits["w2"] = (3 * j + 1).astype(np.float32) / np.float32(3 * side)
    return hits, i, j


def test_a_the_atlas_own_points_return_their_texel_at_every_side():
    """(a) At (3 i + 1) / (3 s) both filters return the texel's own integer means exactly, s = 1 .. 4096: every q is 0 or 256 there — a
    numpy restatement of step 2 over every i of every side first (|fu - i| stays below 1 / 512), then the probe on a diagonal, the edges
    and a sample of each block (every texel up to side 64)."""
    third = np.float32(1.0) / np.float32(3.0)
    worst = 0.0
    for s in range(1, 4097):
        i = np.arange(s)
        fu = ((3 * i + 1).astype(np.float32) / np.float32(3 * s)) * np.float32(s) - third
        worst = max(worst, float(np.abs(fu.astype(np.float64) - i).max()))
        fl = np.floor(fu)
        q = ((fu - fl) * np.float32(256.0) + np.float32(0.5)).astype(np.int32)
        assert (((fl == i) & (q == 0)) | ((fl == i - 1) & (q == 256))).all(), s
    print(f"|fu - i| at most {worst:.3e}")
    assert worst < 1.0 / 512
    g = np.random.default_rng(5)
    for s in list(range(1, 65)) + [100, 255, 1000, 1365, 2048, 4095, 4096]:
        hits, i, j = own_point_hits(s)
        if s > 64:
            keep = np.unique(np.concatenate([np.nonzero((i == 0) | (j == 0) | (i + j == s - 1))[0][::max(1, s // 64)], g.integers(0, len(i), 200)]))
            hits, i, j = hits[keep], i[keep], j[keep]
        film = np.zeros(s * s, dtype=ptss.LINEAR_DTYPE)
        lower = np.add.outer(np.arange(s), np.arange(s)).reshape(-1) <= s - 1
        n = g.integers(1, 9, s * s).astype(np.uint64)
        for name in "rgb":
            film[name] = g.integers(0, 1 << 40, s * s).astype(np.uint64) * n
        film["samples"] = n.astype(np.uint32)
        film[~lower] = (0, 0, 0, 0, 0)   # the empty upper half
        block = np.array([(0, 0, s, s)], dtype=ptss.SURFACE_BLOCK_DTYPE)
        own = film[j * s + i]
        for filter in FILTERS:
            got, info = ptss.probe_lookup_lightmap(None, hits, film, lm_params(s, s, filter), block)
            assert info[FILTERED] == len(hits), (s, filter, info)
            for name in "rgb":
                assert np.array_equal(got[name], own[name] // own["samples"].astype(np.uint64)), (s, filter, name)   # (sums are exact multiples)


def test_a_every_column_of_every_side_through_the_probe():
    """(a) again, through the probe at EVERY side from 1 to 4096 and every i: one axis at a time on a block of s x 1 texels (w2 = 1 / 3
    lands on row 0 with qy = 0), both filters — the two axes share one routine."""
    third = np.float32(1.0) / np.float32(3.0)
    for s in range(1, 4097):
        i = np.arange(s)
        hits = np.zeros(s, dtype=ptss.HIT_DTYPE)
        hits["kind"], hits["normal"], hits["w2"] = 2, UP, third
        hits["w1"] = (3 * i + 1).astype(np.float32) / np.float32(3 * s)
        film = np.zeros(s, dtype=ptss.LINEAR_DTYPE)
        film["r"], film["g"], film["b"], film["samples"] = 3 * i + 1, 5 * i, (i.astype(np.uint64) << np.uint64(40)) + np.uint64(2), 1
        block = np.array([(0, 0, s, 1)], dtype=ptss.SURFACE_BLOCK_DTYPE)
        for filter in FILTERS:
            got, info = ptss.probe_lookup_lightmap(None, hits, film, lm_params(s, 1, filter), block)
            assert info[FILTERED] == s and same_bytes(got, film), (s, filter)


def test_b_a_sphere_blocks_own_points_return_their_texel_under_the_nearest_filter():
    """(b) heights 1 .. 64: the surfel of texel (i, j)'s point looks up texel (i, j)."""
    sph = np.zeros(1, dtype=ptss.SPHERE_DTYPE)
    for h in range(1, 65):
        sph["radius"] = (h - 0.5) / np.pi   # ceil(pi r) = h at one texel a unit
        _, bs, points, texels, height = ptss.surface_atlas_blocks(None, sph, 1.0, 128, 1, 64)
        assert tuple(bs[0]) == (0, 0, 2 * h, h) and height == h
        film = np.zeros(128 * h, dtype=ptss.LINEAR_DTYPE)
        film["r"][texels], film["g"][texels], film["b"][texels], film["samples"][texels] = texels, 7, texels.astype(np.uint64) << np.uint64(30), 1
        got, info = ptss.probe_lookup_lightmap(None, surfel_hits(None, sph, points), film, lm_params(128, h, "nearest"), None, bs)
        assert info[FILTERED] == len(points) and np.array_equal(got["r"], texels), h
        assert np.array_equal(got["b"], texels.astype(np.uint64) << np.uint64(30))


def test_c_a_constant_map_gives_the_constant(sides):
    """(c) every hit with a block, means up to 2^60, sums with samples 1, 3 and 40."""
    s = sides
    hits = scattered_hits(len(s["bt"]), len(s["bs"]), 300, 4, 1)
    for mean in (0, 1, 12345, (1 << 40) + 7, (1 << 48) + 1, (1 << 60) - 1, 1 << 60):
        film = np.zeros(s["W"] * s["H"], dtype=ptss.LINEAR_DTYPE)
        n = (np.arange(len(film)) % 3 == 0) * 2 + (np.arange(len(film)) % 5 == 0) * 12 + 1   # 1, 3, 13, 15: mean * n stays below 2^64
        film["r"], film["g"], film["b"], film["samples"] = np.uint64(mean) * n.astype(np.uint64), np.uint64(mean), 0, n
        film["g"] *= n.astype(np.uint64)
        for filter in FILTERS:
            got, info = ptss.probe_lookup_lightmap(None, hits, film, lm_params(s["W"], s["H"], filter), s["bt"], s["bs"])
            assert info[FILTERED] == len(hits)
            assert (got["r"] == mean).all() and (got["g"] == mean).all() and (got["b"] == 0).all() and (got["samples"] == 1).all(), (mean, filter)


def test_d_an_affine_map_gives_the_affine_value_of_the_quantised_place(sides):
    """(d) texel (i, j) of the side-64 block holds A + B i + C j with samples 1; wherever all four taps count and none is clamped the
    row is round(A + B (i0 + qx / 256) + C (j0 + qy / 256)) — the weighted mean of an affine function is its value at the weighted place."""
    s = sides
    x, y, w, h = (int(v) for v in s["bt"][4])
    A, Bc, Cc = 1 << 50, 3 << 20, 5 << 30
    film = affine_map(s["W"], s["H"], (x, y, w, h), A, Bc, Cc)   # the whole square: the upper half filled too
    g = np.random.default_rng(8)
    hits = make_hits([(2, 4, float(a), float(b), UP, 0) for a, b in g.random((500, 2)) * 0.96 + 0.02])
    got, info = ptss.probe_lookup_lightmap(None, hits, film, lm_params(s["W"], s["H"], "bilinear"), s["bt"], s["bs"])
    assert info[FILTERED] == len(hits)
    checked = 0
    for k, hit in enumerate(hits):
        i0, qx, j0, qy = model_place(hit, False, (x, y, w, h), False)
        if 0 <= i0 < w - 1 and 0 <= j0 < h - 1:
            num = 65536 * A + 256 * (Bc * (256 * i0 + qx) + Cc * (256 * j0 + qy))   # 65536 times the affine value
            assert int(got["r"][k]) == (num + 32768) // 65536, k
            checked += 1
    assert checked > 400


def test_e_modulate_and_emission(sides):
    """(e) diffuseColor 1.0 leaves the mean, 0.0 gives 0, 0.5 gives (m + 1) >> 1; emission alone adds the emmitance at the film's fixed
    point, saturating."""
    s = sides
    film = random_map(s["W"], s["H"], s["texels"], 6)
    mat = np.zeros(2, dtype=ptss.MATERIAL_DTYPE)
    mat["diffuseColor"] = [(1.0, 0.0, 0.5), (1.0, 1.0, 1.0)]
    mat["emmitance"] = [(0.0, 0.0, 0.0), (2.0, 0.0, 1e9)]
    hits = surfel_hits(s["tri"], s["sph"], s["points"][::5])
    hits["materialIdx"] = 0
    plain, _ = ptss.probe_lookup_lightmap(mat, hits, film, lm_params(s["W"], s["H"]), s["bt"], s["bs"])
    shaded, _ = ptss.probe_lookup_lightmap(mat, hits, film, lm_params(s["W"], s["H"], flags=(True, False)), s["bt"], s["bs"])
    assert plain["r"].any() and np.array_equal(shaded["r"], plain["r"]) and not shaded["g"].any()
    assert np.array_equal(shaded["b"], (plain["b"] + np.uint64(1)) >> np.uint64(1))
    hits["materialIdx"] = 1
    lit, _ = ptss.probe_lookup_lightmap(mat, hits, film, lm_params(s["W"], s["H"], flags=(False, True)), s["bt"], s["bs"])
    on = lit["samples"] == 1
    assert on.any() and np.array_equal(lit["r"][on], plain["r"][on] + np.uint64(2 << 20)) and np.array_equal(lit["g"], plain["g"])
    assert np.array_equal(lit["b"][on], plain["b"][on] + np.uint64(65536 << 20))   # clamped to clampMax = 65536
    assert not lit["r"][~on].any()   # no emission without a counted tap
    # saturation: a map near 2^64
    top = film.copy()
    top["r"][s["texels"]], top["samples"][s["texels"]] = np.uint64((1 << 64) - 5), 1
    sat, _ = ptss.probe_lookup_lightmap(mat, hits, top, lm_params(s["W"], s["H"], "nearest", flags=(False, True)), s["bt"], s["bs"])
    assert (sat["r"][sat["samples"] == 1] == np.uint64((1 << 64) - 1)).all()


@pytest.mark.parametrize("flags", FLAGS)
def test_f_every_rejection_writes_zeros_and_is_counted(sides, flags):
    """(f) one of every kind of rejected hit and block row, each alone and all together: a zero row, the right count, and the model's
    verdict. (The same cases run on buffers of the exact size under the sanitizers: test g.)"""
    s = sides
    film = random_map(s["W"], s["H"], s["texels"], 9)
    good = surfel_hits(s["tri"], s["sph"], s["points"][:200:2])
    params = lm_params(s["W"], s["H"], "bilinear", flags)
    hits, blocks = hits_with_bad_rows(good, s["bt"], params, len(s["mat"]))
    got, info = ptss.probe_lookup_lightmap(s["mat"], hits, film, params, blocks, s["bs"])
    want, counts = model_lookup(s["mat"], hits, film, params, blocks, s["bs"])
    assert same_bytes(got, want) and np.array_equal(info, counts), (info, counts)
    assert info[REJECTED] >= 10 + len(bad_block_rows(1, 1)) + (3 if any(flags) else 0) and info[NO_BLOCK] >= 5
    tri_hit = good[good["kind"] == 2][:1]
    for name, h in bad_hit_rows(tri_hit).items():
        row, one = ptss.probe_lookup_lightmap(s["mat"], h, film, params, s["bt"], s["bs"])
        assert not np.ascontiguousarray(row).view(np.uint64).any(), name
        assert one[REJECTED] == 1, (name, one)   # (a miss with a NaN is rejected: the fields are looked at first)
    for k, (name, row) in enumerate(bad_block_rows(s["W"], s["H"]).items()):
        h = tri_hit.copy()
        h["primitive"] = len(s["bt"]) + k
        out, one = ptss.probe_lookup_lightmap(s["mat"], h, film, params, blocks, s["bs"])
        assert one[REJECTED] == 1 and not np.ascontiguousarray(out).view(np.uint64).any(), name


def test_the_probe_refuses_what_the_device_call_refuses(sides):
    s = sides
    film = random_map(s["W"], s["H"], s["texels"], 9)
    hits = surfel_hits(s["tri"], s["sph"], s["points"][:8])
    look = lambda p, f=None: ptss.probe_lookup_lightmap(s["mat"], hits, film, p, s["bt"], s["bs"], film=f)
    assert look(lm_params(s["W"], s["H"]))[1].sum() == 8
    for change in (dict(structSize=36), dict(filter=2), dict(filter=-1), dict(flags=4), dict(flags=0x80000000), dict(reserved=1), dict(firstTriangle=-1),
                   dict(firstSphere=-1), dict(numTriangleBlocks=-1), dict(numSphereBlocks=-2)):
        p = lm_params(s["W"], s["H"])
        for k, v in change.items():
            setattr(p, k, v)
        with pytest.raises(ptss.PtssError):
            look(p)
    bad_film = ptss.linear_params()
    bad_film.scaleLog2 = 33
    with pytest.raises(ptss.PtssError):
        look(lm_params(s["W"], s["H"]), bad_film)
    H = ptss.host_lib()
    p, f = lm_params(s["W"], s["H"], num_triangle_blocks=len(s["bt"]), num_sphere_blocks=len(s["bs"])), ptss.linear_params()
    h = np.ascontiguousarray(hits).view(np.float32).reshape(-1, 12)
    out = np.zeros((8, 4), dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    call = lambda p=p, bt=ptr(s["bt"]), bs=ptr(s["bs"]), m=ptr(film), hh=ptr(h), n=8, o=ptr(out): H.ptss_probe_lookup_lightmap(
        ptr(s["mat"]), len(s["mat"]), C.byref(p), C.byref(f), bt, bs, m, hh, n, o, None)
    assert call() == 0
    assert call(bt=None) == -1 and call(bs=None) == -1 and call(m=None) == -1 and call(hh=None) == -1 and call(o=None) == -1
    assert call(o=ptr(film)) == -1                                   # out overlaps the map
    assert call(n=0, m=None, hh=None, o=None) == 0 and call(n=1 << 31) == -3
    for w, hgt in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
        q = lm_params(w, hgt, num_triangle_blocks=len(s["bt"]), num_sphere_blocks=len(s["bs"]))
        assert call(p=q) == -3, (w, hgt)
    with pytest.raises(ValueError):
        ptss.probe_lookup_lightmap(s["mat"], hits, film[:-1], lm_params(s["W"], s["H"]), s["bt"], s["bs"])


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------------
def test_g_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """(g) tests/csrc/lightmap_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host
    builds of csrc/ptlightmap.h and the atlas, every buffer a heap block of the exact size, one of every rejected hit and block row among
    the hits. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "lightmap_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "lightmap_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("lightmap_sanitize ok"), r.stdout + r.stderr
