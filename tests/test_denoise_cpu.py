"""First-hit features and the denoiser without a GPU: the new C-ABI symbols and struct layouts, the argument checks that must
not touch a device, exact properties of the filter arithmetic (csrc/ptdenoise.h through ptss_probe_denoise), and an independent
float64 restatement of the formulas of DESIGN.md §3.17 on three synthetic feature sets.

Measured on the host build (x86-64), float output against the float64 model, 0..255 scale: planes 2.31e-05, sphere on a floor
2.00e-05, slanted floor 2.02e-05 — largest 2.31e-05; MODEL_TOLERANCE is four times that. No byte differed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptss
from ptss_types import DenoiseParams, PixelFeature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

MEASURED_MAX_DIFF = 2.31e-05
MODEL_TOLERANCE = 4 * MEASURED_MAX_DIFF
assert MODEL_TOLERANCE < 0.5   # beyond that the model and the header are not the same filter


def params(**kw):
    return ptss.default_denoise_params(**kw)


# ---- symbols, layouts, argument checks ----------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    dev = C.CDLL(ptss.DEVICE_LIB)
    host = C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_render_features", "ptss_default_denoise_params", "ptss_denoise", "ptss_read_denoise_plane"):
        assert hasattr(dev, name), name
    assert hasattr(host, "ptss_probe_denoise")


FIELDS = {
    "ptss_pixel_feature": (PixelFeature, ["normal", "depth", "albedo", "materialIdx"]),
    "ptss_denoise_params": (DenoiseParams, ["structSize", "levels", "sigmaColor", "sigmaNormal", "sigmaDepth"]),
}


@pytest.mark.parametrize("struct", sorted(FIELDS))
def test_mirrors_match_the_c_layout(struct, tmp_path):
    cls, names = FIELDS[struct]
    prints = "".join(f'printf(" %zu", offsetof({struct}, {n}));' for n in names)
    src = (f'#include <stdio.h>\n#include <stddef.h>\n#include "ptss.h"\n'
           f'int main(void){{printf("%zu", sizeof({struct})); {prints} return 0;}}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(cls)
    assert got[1:] == [getattr(cls, n).offset for n in names]
    if struct == "ptss_pixel_feature":
        assert got[0] == 32 == ptss.FEATURE_DTYPE.itemsize
        assert got[1] == 0 and got[3] == 16   # the two 16-byte rows
        assert got[1:] == [ptss.FEATURE_DTYPE.fields[n][1] for n in names]


def test_default_params():
    p = DenoiseParams()
    L = ptss.device_lib()
    assert L.ptss_default_denoise_params(None) == -1
    assert L.ptss_default_denoise_params(C.byref(p)) == 0
    assert p.structSize == C.sizeof(DenoiseParams) and 0 <= p.levels <= 6
    assert p.sigmaColor > 0 and p.sigmaNormal > 0 and p.sigmaDepth > 0


def test_argument_checks_without_a_device():
    """A null context, null pointers, a wrong structSize and levels outside 0..6 are answered on the host."""
    L = ptss.device_lib()
    buf = (C.c_float * 64)()
    ctx = C.c_void_p(1)   # never dereferenced: every call below fails before the context is looked at
    assert L.ptss_render_features(None, buf, None) == -1
    assert L.ptss_render_features(ctx, None, None) == -1
    good = params()
    assert L.ptss_denoise(None, buf, C.byref(good), buf, None) == -1
    assert L.ptss_denoise(ctx, None, C.byref(good), buf, None) == -1
    assert L.ptss_denoise(ctx, buf, None, buf, None) == -1
    assert L.ptss_denoise(ctx, buf, C.byref(good), None, None) == -1
    bad = params()
    bad.structSize -= 4
    assert L.ptss_denoise(ctx, buf, C.byref(bad), buf, None) == -1
    for levels in (-1, 7, 100):
        assert L.ptss_denoise(ctx, buf, C.byref(params(levels=levels)), buf, None) == -1
    assert b"levels" in L.ptss_last_error_detail()
    assert L.ptss_read_denoise_plane(None, buf, 3, None) == -1
    assert L.ptss_read_denoise_plane(ctx, None, 3, None) == -1


def test_probe_argument_checks():
    H = ptss.host_lib()
    acc = np.zeros(12, dtype=np.uint32)
    feat = np.zeros(4, dtype=ptss.FEATURE_DTYPE)
    out = np.zeros(16, dtype=np.uint8)
    a, f, o = acc.ctypes.data_as(C.POINTER(C.c_uint32)), feat.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    good = params()
    assert H.ptss_probe_denoise(a, 1.0, f, 2, 2, C.byref(good), o, None) == 0
    assert H.ptss_probe_denoise(None, 1.0, f, 2, 2, C.byref(good), o, None) < 0
    assert H.ptss_probe_denoise(a, 1.0, None, 2, 2, C.byref(good), o, None) < 0
    assert H.ptss_probe_denoise(a, 1.0, f, 0, 2, C.byref(good), o, None) < 0
    assert H.ptss_probe_denoise(a, 1.0, f, 2, 2, None, o, None) < 0
    assert H.ptss_probe_denoise(a, 1.0, f, 2, 2, C.byref(params(levels=7)), o, None) < 0
    bad = params()
    bad.structSize += 4
    assert H.ptss_probe_denoise(a, 1.0, f, 2, 2, C.byref(bad), o, None) < 0


# ---- synthetic feature sets: a pinhole camera at the origin looking down -z -------------------------------------------------
def pinhole(w, h, fov=1.2):
    ys, xs = np.mgrid[0:h, 0:w]
    t = np.tan(fov / 2)
    d = np.stack([((xs + 0.5) / w - 0.5) * 2 * t, ((ys + 0.5) / h - 0.5) * 2 * t * h / w, -np.ones((h, w))], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def pack(normal, depth, material, albedo=None):
    h, w = depth.shape
    f = np.zeros(h * w, dtype=ptss.FEATURE_DTYPE)
    f["normal"] = normal.reshape(-1, 3)
    f["depth"] = depth.reshape(-1)
    f["materialIdx"] = material.reshape(-1)
    f["albedo"] = 0.5 if albedo is None else albedo.reshape(-1, 3)
    miss = f["materialIdx"] < 0
    f["normal"][miss] = 0
    f["depth"][miss] = np.inf
    return f


def plane_hit(d, n, c):
    """Distance along unit rays d from the origin to the plane n . X = c (inf where it is not ahead)."""
    nd = d @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = c / nd
    return np.where((nd != 0) & (t > 0), t, np.inf)


def planes_at_an_edge(w, h):
    """Two walls of ONE material meeting in a vertical edge straight ahead: only normal and depth tell them apart."""
    d = pinhole(w, h)
    nl, nr = np.array([0.6, 0.0, 0.8]), np.array([-0.6, 0.0, 0.8])
    tl, tr = plane_hit(d, nl, -4.0), plane_hit(d, nr, -4.0)
    left = tl <= tr
    depth = np.where(left, tl, tr)
    normal = np.where(left[..., None], nl, nr)
    return pack(normal, depth, np.zeros((h, w), dtype=np.int32))


def sphere_on_a_floor(w, h):
    d = pinhole(w, h)
    centre, r = np.array([0.0, 0.0, -4.0]), 1.0
    b = d @ centre
    disc = b * b - (centre @ centre - r * r)
    ts = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0)), np.inf)
    tf = plane_hit(d, np.array([0.0, 1.0, 0.0]), -1.0)
    depth = np.minimum(ts, tf)
    material = np.where(np.isinf(depth), -1, np.where(ts <= tf, 1, 0)).astype(np.int32)
    with np.errstate(invalid="ignore"):
        ns = (d * ts[..., None] - centre) / r
    normal = np.where((material == 1)[..., None], ns, np.array([0.0, 1.0, 0.0]))
    return pack(np.nan_to_num(normal), depth, material)


def slanted_floor(w, h):
    """A floor seen at a grazing angle, to the horizon: depths from 1.4 to several hundred, misses above."""
    d = pinhole(w, h)
    depth = plane_hit(d, np.array([0.0, 1.0, 0.0]), -1.0)
    material = np.where(np.isinf(depth), -1, 0).astype(np.int32)
    normal = np.broadcast_to(np.array([0.0, 1.0, 0.0]), d.shape)
    return pack(normal, depth, material)


SETS = {"planes": planes_at_an_edge, "sphere": sphere_on_a_floor, "floor": slanted_floor}
W, H = 56, 40


def noisy_accum(features, ticks, seed):
    """`ticks` 8-bit samples per pixel around a colour that depends on the material and, smoothly, on the position."""
    rng = np.random.default_rng(seed)
    m = features["materialIdx"].reshape(H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    base = np.stack([90 + 50 * m + 0.8 * xs, 120 - 30 * m + 0.5 * ys, 60 + 40 * (m == 0) + 0.3 * (xs + ys)], axis=-1)
    acc = np.zeros((H, W, 3), dtype=np.uint32)
    for _ in range(ticks):
        acc += np.clip(base + rng.normal(0, 35, size=base.shape), 0, 255).astype(np.uint32)
    return acc.reshape(-1, 3)


# ---- the independent model: DESIGN.md §3.17 in float64 numpy, vectorised per tap -----------------------------------------------
def shifted(a, dx, dy, fill):
    """a[y + dy, x + dx], `fill` outside the frame."""
    out = np.full_like(a, fill)
    h, w = a.shape[:2]
    x0, x1 = max(0, -dx), min(w, w - dx)
    y0, y1 = max(0, -dy), min(h, h - dy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def model(accum, inverse_ticks, features, w, h, p):
    c = accum.reshape(h, w, 3).astype(np.float64) * float(np.float32(inverse_ticks))
    n = features["normal"].reshape(h, w, 3).astype(np.float64)
    z = features["depth"].reshape(h, w).astype(np.float64)
    m = features["materialIdx"].reshape(h, w).astype(np.int64)
    hit = m >= 0
    inside = np.ones((h, w), dtype=bool)
    with np.errstate(invalid="ignore"):
        def slope(dx, dy):
            a = np.where(shifted(inside, -dx, -dy, False), np.abs(z - shifted(z, -dx, -dy, 0.0)), np.inf)
            b = np.where(shifted(inside, dx, dy, False), np.abs(shifted(z, dx, dy, 0.0) - z), np.inf)
            g = np.fmin(a, b)
            return np.where(np.isfinite(g), g, 0.0)
        gx, gy = slope(1, 0), slope(0, 1)
    spline = {0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
    for level in range(p.levels):
        s = 2 ** level
        sigma = p.sigmaColor / s
        total = np.zeros_like(c)
        wsum = np.full((h, w), spline[0] * spline[0])
        lo, hi = c.copy(), c.copy()
        for j in range(-2, 3):
            for i in range(-2, 3):
                if i == 0 and j == 0:
                    continue
                ok = shifted(inside, i * s, j * s, False) & (shifted(m, i * s, j * s, -99) == m)
                cq, nq, zq = shifted(c, i * s, j * s, 0.0), shifted(n, i * s, j * s, 0.0), shifted(z, i * s, j * s, 1.0)
                e = ((cq - c) ** 2).sum(-1) / sigma ** 2
                with np.errstate(invalid="ignore", divide="ignore"):
                    e_n = np.maximum(0.0, 1.0 - (n * nq).sum(-1)) / p.sigmaNormal
                    tol = np.maximum(p.sigmaDepth * (gx * abs(i * s) + gy * abs(j * s)) + 1e-3 * z, 1e-30)
                    e_z = np.abs(z - zq) / tol
                e = np.where(hit & ok, e + e_n + e_z, e)
                with np.errstate(invalid="ignore"):
                    wq = np.where(ok, spline[abs(i)] * spline[abs(j)] * np.exp(-e), 0.0)
                wq = np.where(wq > 0, wq, 0.0)
                used = wq > 0
                total += wq[..., None] * (cq - c)
                wsum += wq
                lo = np.where(used[..., None], np.minimum(lo, cq), lo)
                hi = np.where(used[..., None], np.maximum(hi, cq), hi)
        c = np.clip(c + total / wsum[..., None], lo, hi)
    return c.reshape(-1, 3)


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_build_agrees_with_the_float64_model(name):
    features = SETS[name](W, H)
    accum = noisy_accum(features, 4, seed=11)
    worst, steps = 0.0, 0
    for levels in (1, 3, 5):
        p = params(levels=levels)
        rgba, flt = ptss.probe_denoise(accum, 0.25, features, W, H, p)
        want = model(accum, 0.25, features, W, H, p)
        diff = np.abs(flt.astype(np.float64) - want).max()
        worst = max(worst, float(diff))
        want_bytes = np.floor(want + 0.5).astype(np.int64)
        delta = np.abs(rgba[:, :3].astype(np.int64) - want_bytes)
        assert delta.max() <= 1
        steps = max(steps, int((delta.max(axis=1) > 0).sum()))
    print(f"{name}: largest |host - model| = {worst:.3g}, pixels one byte step apart = {steps} of {W * H}")
    assert worst <= MODEL_TOLERANCE
    assert steps <= 0.01 * W * H


# ---- exact properties ---------------------------------------------------------------------------------------------------------
def display_bytes(accum, inverse_ticks):
    v = accum.astype(np.float32) * np.float32(inverse_ticks) + np.float32(0.5)
    return v.astype(np.uint8)   # truncation, as (unsigned char)(v + 0.5f)


@pytest.mark.parametrize("inverse_ticks", [1.0, 0.25, 1.0 / 3.0, 1.0 / 28.0])
def test_levels_zero_is_the_display_value(inverse_ticks):
    features = sphere_on_a_floor(W, H)
    ticks = int(round(1 / inverse_ticks))
    accum = noisy_accum(features, ticks, seed=3)
    rgba, flt = ptss.probe_denoise(accum, np.float32(inverse_ticks), features, W, H, params(levels=0))
    assert np.array_equal(rgba[:, :3], display_bytes(accum, inverse_ticks))
    assert (rgba[:, 3] == 255).all()
    assert np.array_equal(flt, accum.astype(np.float32) * np.float32(inverse_ticks))


@pytest.mark.parametrize("name", sorted(SETS))
def test_a_constant_image_stays_constant(name):
    features = SETS[name](W, H)
    for value, inverse_ticks in (((1, 3, 5), 0.5), ((100, 101, 255), 1.0), ((77, 310, 5), 1.0 / 3.0)):
        accum = np.tile(np.array(value, dtype=np.uint32), (W * H, 1))
        want = display_bytes(accum, inverse_ticks)
        for levels in range(7):
            rgba, _ = ptss.probe_denoise(accum, np.float32(inverse_ticks), features, W, H, params(levels=levels))
            assert np.array_equal(rgba[:, :3], want), (value, levels)


def test_two_materials_never_mix():
    """Every output byte of a region lies within the min .. max of that region's input: a convex combination of its own taps."""
    rng = np.random.default_rng(5)
    material = np.zeros((H, W), dtype=np.int32)
    material[:, W // 2:] = 1
    material[H // 2:, : W // 4] = -1   # and a patch of misses
    normal = np.broadcast_to(np.array([0.0, 0.0, 1.0]), (H, W, 3))
    features = pack(normal, np.full((H, W), 3.0), material)
    accum = np.zeros((H, W, 3), dtype=np.uint32)
    ranges = {0: (10, 60), 1: (150, 250), -1: (70, 120)}
    for k, (a, b) in ranges.items():
        accum[material == k] = rng.integers(a, b + 1, size=(int((material == k).sum()), 3))
    accum = accum.reshape(-1, 3)
    for levels in range(1, 7):
        rgba, _ = ptss.probe_denoise(accum, 1.0, features, W, H, params(levels=levels, sigmaColor=1000.0))
        for k in ranges:
            region = material.reshape(-1) == k
            for ch in range(3):
                assert accum[region, ch].min() <= rgba[region, ch].min() and rgba[region, ch].max() <= accum[region, ch].max(), (levels, k)
        # ... and the filter does filter: inside a region the spread shrinks
        assert rgba[material.reshape(-1) == 1, 0].std() < accum[material.reshape(-1) == 1, 0].std()


def test_result_does_not_depend_on_the_frame_around_it():
    """An image, and the same image embedded in a larger background of misses, agree on the interior: taps beyond the frame
    and taps on another material are both simply absent."""
    features = planes_at_an_edge(W, H)
    accum = noisy_accum(features, 4, seed=9)
    bw, bh, ox, oy = W + 37, H + 21, 19, 8
    big_f = pack(np.zeros((bh, bw, 3)), np.full((bh, bw), np.inf), np.full((bh, bw), -1, dtype=np.int32)).reshape(bh, bw)
    big_f[oy:oy + H, ox:ox + W] = features.reshape(H, W)
    big_a = np.random.default_rng(2).integers(0, 1021, size=(bh, bw, 3)).astype(np.uint32)
    big_a[oy:oy + H, ox:ox + W] = accum.reshape(H, W, 3)
    for levels in (1, 2, 4, 6):
        p = params(levels=levels)
        rgba, flt = ptss.probe_denoise(accum, 0.25, features, W, H, p)
        big_rgba, big_flt = ptss.probe_denoise(big_a.reshape(-1, 3), 0.25, big_f.reshape(-1), bw, bh, p)
        assert np.array_equal(big_flt.reshape(bh, bw, 3)[oy:oy + H, ox:ox + W], flt.reshape(H, W, 3))
        assert np.array_equal(big_rgba.reshape(bh, bw, 4)[oy:oy + H, ox:ox + W], rgba.reshape(H, W, 4))


def test_misses_and_zero_normals_give_no_nan():
    features = pack(np.zeros((H, W, 3)), np.full((H, W), np.inf), np.full((H, W), -1, dtype=np.int32))
    features["depth"][::3] = np.inf
    hits = features.reshape(H, W)
    hits["materialIdx"][5:20, 5:30] = 2       # hits with ZERO normals and a few infinite depths in between
    hits["depth"][5:20, 5:30] = 2.5
    hits["depth"][8, 5:30] = np.inf
    accum = noisy_accum(features, 4, seed=1)
    for levels in range(7):
        rgba, flt = ptss.probe_denoise(accum, 0.25, features, W, H, params(levels=levels))
        assert np.isfinite(flt).all()
        assert flt.min() >= 0 and flt.max() <= 255
