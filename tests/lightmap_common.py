"""The model and the cases shared by tests/test_lightmap_cpu.py, tests/test_gpu_lightmap.py and tests/test_gpu_lightmap_main.py (light maps
read back: ptss_surface_atlas_blocks, ptss_lookup_lightmap).

model_lookup restates the head comment of csrc/ptlightmap.h hit by hit: the place in numpy float32 scalars (fma rounded once from
rationals, linreproject_common.f32_fma; ptm::atan through ptss_probe_math; the host's ptm::div and ptm::sqrt are the IEEE operations),
the mean in Python integers and exact rationals, the fixed point of the emission through linear_common.model_fixed. It shares no code with
the header and must agree with the probe byte for byte."""
import ctypes as C
from fractions import Fraction

import numpy as np

import ptss
from linear_common import model_fixed
from linreproject_common import f32_fma

F32 = np.float32
PI = F32(3.14159265358979323846)
TWO_PI = F32(2) * PI
HALF_PI = F32(1.5707963267948966)
THIRD = F32(1.0) / F32(3.0)
MASK64 = (1 << 64) - 1
FILTERS = ("nearest", "bilinear")
FLAGS = ((False, False), (True, False), (False, True), (True, True))   # (modulate, emission)
FILTERED, EMPTY, NO_BLOCK, REJECTED = range(4)
NS = (1, 63, 64, 65, 255, 256, 257, 1025)   # around a quad, a wave and a workgroup in both kernel forms


def atan(x):
    """ptm::atan on the host (ptss_probe_math op 3), one float32: the model does not restate the polynomial."""
    a, out = np.array([x], dtype=np.float32), np.empty(1, dtype=np.float32)
    f32p = C.POINTER(C.c_float)
    assert ptss.host_lib().ptss_probe_math(3, a.ctypes.data_as(f32p), None, out.ctypes.data_as(f32p), 1) == 0
    return out[0]


def atan2(y, x):
    """ptlinrp.h's quadrant rule; x and y finite."""
    y, x = F32(y), F32(x)
    ax, ay = abs(x), abs(y)
    if ax == 0 and ay == 0:
        return F32(0)
    if ax >= ay:
        a = atan(y / x)
        if x < 0:
            return a + PI if y >= 0 else a - PI
        return a
    return (HALF_PI if y > 0 else -HALF_PI) - atan(x / y)


def split_axis(f, side, nearest):
    f = min(max(F32(f), F32(-1.0)), F32(side))
    fl = np.floor(f)
    q = int(F32(F32(f - fl) * F32(256.0)) + F32(0.5))
    if nearest:
        q = 256 if q >= 128 else 0
    return int(fl), q


def model_place(hit, sphere, block, nearest):
    """(i0, qx, j0, qy) of a hit in a block that passed the checks."""
    x, y, w, h = block
    with np.errstate(over="ignore", invalid="ignore"):
        if sphere:
            n = [F32(c) for c in hit["normal"]]
            lon = atan2(n[0], -n[2])
            lat = atan2(n[1], np.sqrt(f32_fma(n[2], n[2], n[0] * n[0])))
            fu = (lon / TWO_PI + F32(0.5)) * F32(w) - F32(0.5)
            fv = (lat / PI + F32(0.5)) * F32(h) - F32(0.5)
        else:
            fu = F32(hit["w1"]) * F32(w) - THIRD
            fv = F32(hit["w2"]) * F32(h) - THIRD
    return split_axis(fu, w, nearest) + split_axis(fv, h, nearest)


def model_taps(place, sphere, block, atlas_width):
    """[(weight, texel number)] of the four taps."""
    x, y, w, h = block
    i0, qx, j0, qy = place
    taps = []
    for t in range(4):
        di, dj = t & 1, t >> 1
        weight = (qx if di else 256 - qx) * (qy if dj else 256 - qy)
        col, row = i0 + di, j0 + dj
        col = col % w if sphere else min(max(col, 0), w - 1)
        row = min(max(row, 0), h - 1)
        taps.append((weight, (y + row) * atlas_width + x + col))
    assert sum(wt for wt, _ in taps) == 65536
    return taps


def modulate_weight(c):
    with np.errstate(over="ignore", invalid="ignore"):
        t = F32(c) * F32(65536.0) + F32(0.5)
    if not t > 0:
        return 0
    return 65536 if t >= 65536 else int(t)


def model_verdict_before_taps(hit, params, blocks_tri, blocks_sph, num_materials):
    """(verdict or None to go on, sphere, block)."""
    kind = int(hit["kind"])
    if kind < 0 or kind > 2:
        return REJECTED, False, None
    if not (np.isfinite(hit["w1"]) and np.isfinite(hit["w2"]) and np.isfinite(hit["normal"]).all()):
        return REJECTED, False, None
    if kind == 0:
        return NO_BLOCK, False, None
    sphere = kind == 1
    k = int(hit["primitive"]) - (params.firstSphere if sphere else params.firstTriangle)
    if k < 0 or k >= (params.numSphereBlocks if sphere else params.numTriangleBlocks):
        return NO_BLOCK, sphere, None
    b = (blocks_sph if sphere else blocks_tri)[k]
    x, y, w, h = int(b["x"]), int(b["y"]), int(b["width"]), int(b["height"])
    if w == 0:
        return NO_BLOCK, sphere, None
    if x < 0 or y < 0 or w < 0 or h <= 0 or w > 8192 or h > 4096 or x + w > params.atlasWidth or y + h > params.atlasHeight:
        return REJECTED, sphere, None
    if params.flags and not 0 <= int(hit["materialIdx"]) < num_materials:
        return REJECTED, sphere, None
    return None, sphere, (x, y, w, h)


def model_lookup(materials, hits, map, params, blocks_tri=None, blocks_sph=None, film=None, info=None):
    """ptss_probe_lookup_lightmap in the terms above -> ((N,) LINEAR_DTYPE, (4,) uint32)."""
    film = film if film is not None else ptss.linear_params()
    params = ptss._lightmap_counts(params, blocks_tri, blocks_sph)
    num_materials = 0 if materials is None else len(materials)
    out = np.zeros(len(hits), dtype=ptss.LINEAR_DTYPE)
    counts = np.zeros(4, dtype=np.uint32) if info is None else np.array(info, dtype=np.uint32)
    nearest = params.filter == ptss.LIGHTMAP_NEAREST
    for i, hit in enumerate(hits):
        verdict, sphere, block = model_verdict_before_taps(hit, params, blocks_tri, blocks_sph, num_materials)
        if verdict is None:
            W, S = 0, [0, 0, 0]
            for weight, texel in model_taps(model_place(hit, sphere, block, nearest), sphere, block, params.atlasWidth):
                if weight == 0:
                    continue
                e = map[texel]
                N = int(e["samples"])
                if N == 0:
                    continue
                W += weight
                for c, name in enumerate("rgb"):
                    S[c] += weight * ((int(e[name]) + N // 2) // N)
            verdict = FILTERED if W else EMPTY
            if W:
                row = []
                for c in range(3):
                    mean = Fraction(S[c], W) + Fraction(1, 2)
                    m = mean.numerator // mean.denominator
                    mat = materials[int(hit["materialIdx"])] if params.flags else None
                    if params.flags & ptss.LIGHTMAP_MODULATE:
                        m = (m * modulate_weight(mat["diffuseColor"][c]) + 32768) >> 16
                    if params.flags & ptss.LIGHTMAP_EMISSION:
                        m = min(m + model_fixed(mat["emmitance"][c], film)[0], MASK64)
                    row.append(m)
                out[i] = (row[0], row[1], row[2], 1, 0)
        counts[verdict] += 1
    return out, counts


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def make_hits(rows):
    """[(kind, primitive, w1, w2, normal, materialIdx)] -> (N,) HIT_DTYPE."""
    hits = np.zeros(len(rows), dtype=ptss.HIT_DTYPE)
    for k, (kind, primitive, w1, w2, normal, material) in enumerate(rows):
        hits[k]["kind"], hits[k]["primitive"], hits[k]["w1"], hits[k]["w2"] = kind, primitive, w1, w2
        hits[k]["normal"], hits[k]["materialIdx"] = normal, material
    return hits


def surfel_hits(triangles, spheres, points):
    """The ptss_ray_hit rows a ray arriving at each point would report (ptss_probe_surface_rays' surfels)."""
    got = ptss.probe_surface_rays(triangles, spheres, points, np.zeros((len(points), 6), np.uint32), ptss.surface_params("normal"), surfels=True)
    assert got[3] == 0
    return got[2]


def random_map(width, height, texels, seed, big=False, ones=0.0):
    """A film of width x height whose `texels` hold samples: sums of random means times random counts (big: means up to 2^62 / count, so
    that a weighted sum needs two words), a share `ones` of them with samples == 1; every other texel all zero."""
    g = np.random.default_rng(seed)
    film = np.zeros(width * height, dtype=ptss.LINEAR_DTYPE)
    texels = np.asarray(texels, dtype=np.int64)
    n = len(texels)
    samples = g.integers(2, 40, n).astype(np.uint64)
    samples[g.random(n) < ones] = 1
    top = (1 << 57) if big else (1 << 24)
    for name in "rgb":
        film[name][texels] = g.integers(0, top, n).astype(np.uint64) * samples + g.integers(0, 40, n).astype(np.uint64) % samples
    film["samples"][texels] = samples.astype(np.uint32)
    film["clamped"][texels] = g.integers(0, 3, n).astype(np.uint32)
    return film


def bad_block_rows(atlas_width, atlas_height):
    """One of every kind of rejected block row, by name (and width == 0: no block)."""
    W, H = atlas_width, atlas_height
    return {
        "x < 0": (-1, 0, 2, 2), "y < 0": (0, -1, 2, 2), "width < 0": (0, 0, -2, 2), "height < 0": (0, 0, 2, -2), "height == 0": (0, 0, 2, 0),
        "x + width > atlasWidth": (W - 1, 0, 2, 2), "y + height > atlasHeight": (0, H - 1, 2, 2), "x far outside": (2 ** 31 - 1, 0, 2, 2),
        "y far outside": (0, 2 ** 31 - 1, 1, 1), "width > 8192": (0, 0, 8193, 1), "height > 4096": (0, 0, 1, 4097),
        "width INT_MIN": (0, 0, -2 ** 31, 1), "x INT_MIN": (-2 ** 31, 0, 1, 1),
    }


def bad_hit_rows(good):
    """One of every kind of rejected hit made from a good triangle hit (an array of one), by name."""
    nan, inf = float("nan"), float("inf")
    rows = {}
    for name, change in {"kind 3": dict(kind=3), "kind -1": dict(kind=-1), "kind INT_MAX": dict(kind=2 ** 31 - 1), "w1 NaN": dict(w1=nan),
                         "w1 inf": dict(w1=inf), "w2 -inf": dict(w2=-inf), "w2 NaN": dict(w2=nan), "normal NaN": dict(normal=(nan, 0, 1)),
                         "normal inf": dict(normal=(0, inf, 0)), "miss with NaN": dict(kind=0, w1=nan)}.items():
        h = good.copy()
        for k, v in change.items():
            h[k][0] = v
        rows[name] = h
    return rows


def hits_with_bad_rows(good_hits, blocks_tri, params, material_count):
    """good_hits with one of every rejected hit and block row inside the first 60 entries (entry 0 stays good) -> (hits, blocks_tri with
    the bad rows appended)."""
    tri_hit = good_hits[good_hits["kind"] == 2][:1].copy()
    bad_hits = list(bad_hit_rows(tri_hit).values())
    rows = list(bad_block_rows(params.atlasWidth, params.atlasHeight).values()) + [(3, 3, 0, 5)]   # the last: width == 0, no block
    blocks = np.concatenate([blocks_tri, np.array(rows, dtype=np.int32).view(ptss.SURFACE_BLOCK_DTYPE).reshape(-1)])
    for k in range(len(rows)):
        h = tri_hit.copy()
        h["primitive"][0] = params.firstTriangle + len(blocks_tri) + k
        bad_hits.append(h)
    for primitive in (params.firstTriangle + len(blocks), -1, 2 ** 31 - 1, -2 ** 31):   # outside the table: no block
        h = tri_hit.copy()
        h["primitive"][0] = primitive
        bad_hits.append(h)
    for material in (-1, material_count, 2 ** 31 - 1):   # rejected with a flag, fine without
        h = tri_hit.copy()
        h["materialIdx"][0] = material
        bad_hits.append(h)
    hits = good_hits.copy()
    assert 2 * len(bad_hits) < 63 <= len(hits)   # all of them inside the smallest batch but one
    hits[1:1 + 2 * len(bad_hits):2] = np.concatenate(bad_hits)
    return hits, blocks


def affine_map(width, height, block, base, dx, dy):
    """A film whose texel (i, j) of `block` has samples 1 and the value base + dx i + dy j in every channel."""
    film = np.zeros(width * height, dtype=ptss.LINEAR_DTYPE)
    x, y, w, h = block
    for j in range(h):
        for i in range(w):
            film[(y + j) * width + x + i] = (base + dx * i + dy * j,) * 3 + (1, 0)
    return film


def read_pfm(path, width):
    """A colour PFM of `width` columns -> ((rows * width, 3) float32 bottom row first, rows)."""
    b = open(path, "rb").read()
    head, size, scale, body = b.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert head == b"PF" and w == width and scale == b"-1.0" and len(body) == w * h * 12
    return np.frombuffer(body, "<f4").reshape(h * w, 3), h
