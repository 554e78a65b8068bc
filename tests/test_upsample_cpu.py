"""Guided upsampling without a GPU (ptss_render_features_scaled / ptss_upsample): the new C-ABI symbols and the
layout of ptss_upsample_params, the argument checks that must not touch a device, the tap geometry against fractions.Fraction, exact
properties of the arithmetic (csrc/ptupsample.h through ptss_probe_upsample), and an independent float64 restatement of the formulas
of §3.22 on three synthetic feature sets.

The float64 model is written from the formulas (u = (X + 0.5) / f - 0.5 with a floor, not the integer form of the header). Measured
on the host build (x86-64), float output against the model on the 0..255 scale, lo 33x17 and 64x64, f = 2, 3, 4: planes 1.64e-05,
sphere on a floor 2.80e-05, slanted floor 1.70e-05 — largest 2.80e-05; MODEL_TOLERANCE is four times that. The
weight sums agree within 6.17e-07. A byte may differ from the model's only where the model's value lies within MODEL_TOLERANCE of a
k + 0.5 tie: 3, 10 and 3 bytes of the three sets do, by one step."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import ptss
from ptss_types import UpsampleParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

MEASURED_MAX_DIFF = 2.80e-05
MEASURED_MAX_WEIGHT_DIFF = 6.17e-07
MODEL_TOLERANCE = 4 * MEASURED_MAX_DIFF
assert MODEL_TOLERANCE < 0.5   # beyond that the model and the header are not the same filter
FACTORS = (2, 3, 4)
SHAPES = ((33, 17), (64, 64))


def params(**kw):
    return ptss.default_upsample_params(**kw)


# ---- symbols, layout, defaults, argument checks -------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    dev, host = C.CDLL(ptss.DEVICE_LIB), C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_render_features_scaled", "ptss_default_upsample_params", "ptss_upsample", "ptss_upsample_launches"):
        assert hasattr(dev, name), name
    for name in ("ptss_probe_upsample", "ptss_probe_upsample_axis"):
        assert hasattr(host, name), name
    assert ptss.device_lib().ptss_version() == 300   # no existing struct changed


def test_mirror_matches_the_c_layout(tmp_path):
    names = ["structSize", "factor", "sigmaNormal", "sigmaDepth"]
    prints = "".join(f'printf(" %zu", offsetof(ptss_upsample_params, {n}));' for n in names)
    src = (f'#include <stdio.h>\n#include <stddef.h>\n#include "ptss.h"\n'
           f'int main(void){{printf("%zu", sizeof(ptss_upsample_params)); {prints} return 0;}}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(UpsampleParams) == 16
    assert got[1:] == [getattr(UpsampleParams, n).offset for n in names]


def test_default_params():
    L = ptss.device_lib()
    p = UpsampleParams()
    assert L.ptss_default_upsample_params(None) == -1
    assert L.ptss_default_upsample_params(C.byref(p)) == 0
    assert p.structSize == C.sizeof(UpsampleParams) and p.factor == 2
    d = ptss.default_denoise_params()   # the denoiser's tolerances
    assert p.sigmaNormal == d.sigmaNormal == np.float32(0.1) and p.sigmaDepth == d.sigmaDepth == 4.0


def bad_params():
    out = [params(factor=f) for f in (0, -1, 5, 1 << 20)]
    for name in ("sigmaNormal", "sigmaDepth"):
        out += [params(**{name: v}) for v in (0.0, -1.0, float("inf"), float("nan"))]
    for delta in (-4, 4):
        p = params()
        p.structSize += delta
        out.append(p)
    return out


def test_argument_checks_without_a_device():
    """Every refusal that is decided before the context is looked at: the fake context below is never dereferenced."""
    L = ptss.device_lib()
    buf, out = (C.c_float * 64)(), (C.c_float * 64)()
    ctx = C.c_void_p(1)
    off = lambda b, n: C.c_void_p(C.addressof(b) + n)
    assert C.addressof(buf) % 16 == 0 and C.addressof(out) % 16 == 0
    assert L.ptss_render_features_scaled(None, 2, buf, None) == -1
    assert L.ptss_render_features_scaled(ctx, 2, None, None) == -1
    for factor in (0, -1, 5, 1 << 20):
        assert L.ptss_render_features_scaled(ctx, factor, buf, None) == -1, factor
        assert b"factor" in L.ptss_last_error_detail()
    for n in (4, 8, 12):
        assert L.ptss_render_features_scaled(ctx, 2, off(buf, n), None) == -1
    good = params()
    call = lambda c=ctx, lo=buf, fl=buf, fh=buf, p=C.byref(good), o=out, of=None: L.ptss_upsample(c, lo, fl, fh, p, o, of, None)
    for kw in (dict(c=None), dict(lo=None), dict(fl=None), dict(fh=None), dict(p=None), dict(o=None)):
        assert call(**kw) == -1, kw
    for p in bad_params():
        assert call(p=C.byref(p)) == -1, (p.structSize, p.factor, p.sigmaNormal, p.sigmaDepth)
    assert call(lo=off(buf, 2)) == -1 and call(o=off(out, 1)) == -1            # 4 B for the bytes
    assert call(fl=off(buf, 4)) == -1 and call(fh=off(buf, 8)) == -1 and call(of=off(out, 4)) == -1   # 16 B for features and floats
    assert call(o=buf) == -1                                                     # dev_out_hi == dev_lo
    assert b"dev_lo" in L.ptss_last_error_detail()
    n = C.c_ulonglong()
    assert L.ptss_upsample_launches(None, C.byref(n)) == -1
    assert L.ptss_upsample_launches(ctx, None) == -1


def test_probe_argument_checks():
    Hh = ptss.host_lib()
    lo = np.zeros((4, 4), dtype=np.uint8)
    fl = np.zeros(4, dtype=ptss.FEATURE_DTYPE)
    fh = np.zeros(16, dtype=ptss.FEATURE_DTYPE)
    out = np.zeros((16, 4), dtype=np.uint8)
    flt = np.zeros(64, dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = params()

    def call(l=vp(lo), a=vp(fl), w=2, h=2, b=vp(fh), p=C.byref(good), o=vp(out), f=flt.ctypes.data_as(C.POINTER(C.c_float))):
        return Hh.ptss_probe_upsample(l, a, w, h, b, p, o, f)

    assert call() == 0 and call(f=None) == 0
    for kw in (dict(l=None), dict(a=None), dict(b=None), dict(p=None), dict(o=None), dict(w=0), dict(h=-1), dict(o=vp(lo))):
        assert call(**kw) < 0, kw
    for p in bad_params():
        assert call(p=C.byref(p)) < 0, (p.structSize, p.factor, p.sigmaNormal, p.sigmaDepth)
    assert call(w=1 << 15, h=1 << 15, p=C.byref(params(factor=2))) < 0   # 2^32 hi-res pixels
    x0, k, fx = C.c_int(), C.c_int(), C.c_float()
    for X, f in ((-1, 2), (0, 0), (0, 5)):
        assert Hh.ptss_probe_upsample_axis(X, f, C.byref(x0), C.byref(k), C.byref(fx)) < 0
    assert Hh.ptss_probe_upsample_axis(0, 2, None, C.byref(k), C.byref(fx)) < 0


# ---- the tap table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", (1,) + FACTORS)
def test_tap_table_against_fractions(f):
    """u = (X + 0.5) / f - 0.5 exactly: x0 = floor(u), u - x0 = k / 2f, fx the float32 nearest to it; k is never f."""
    for X in range(0, 5 * f + 1):   # every phase, five periods (the first one reaches x0 = -1)
        u = Fraction(2 * X + 1, 2 * f) - Fraction(1, 2)
        x0, k, fx = ptss.probe_upsample_axis(X, f)
        floor = u.numerator // u.denominator
        assert x0 == floor and Fraction(k, 2 * f) == u - floor, (X, f)
        assert 0 <= k < 2 * f and k != f
        assert np.float32(fx) == np.float32(k) / np.float32(2 * f)   # one IEEE division
        assert abs(Fraction(float(fx)) - Fraction(k, 2 * f)) <= Fraction(k, 2 * f) / 2 ** 24
        nearest = x0 + (1 if 2 * k > 2 * f else 0)
        assert nearest == X // f
    assert ptss.probe_upsample_axis(0, f)[0] == (-1 if f > 1 else 0)


# ---- synthetic feature sets: a pinhole camera at the origin looking down -z, traced at any frame size ---------------------------
def pinhole(w, h, fov=1.2):
    ys, xs = np.mgrid[0:h, 0:w]
    t = np.tan(fov / 2)
    d = np.stack([((xs + 0.5) / w - 0.5) * 2 * t, ((ys + 0.5) / h - 0.5) * 2 * t * h / w, -np.ones((h, w))], axis=-1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def pack(normal, depth, material):
    h, w = depth.shape
    f = np.zeros(h * w, dtype=ptss.FEATURE_DTYPE)
    f["normal"], f["depth"], f["materialIdx"], f["albedo"] = normal.reshape(-1, 3), depth.reshape(-1), material.reshape(-1), 0.5
    miss = f["materialIdx"] < 0
    f["normal"][miss] = 0
    f["depth"][miss] = np.inf
    return f


def plane_hit(d, n, c):
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
    return pack(np.where(left[..., None], nl, nr), np.where(left, tl, tr), np.zeros((h, w), dtype=np.int32))


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
    return pack(np.nan_to_num(np.where((material == 1)[..., None], ns, np.array([0.0, 1.0, 0.0]))), depth, material)


def slanted_floor(w, h):
    """A floor seen at a grazing angle, to the horizon, misses above."""
    d = pinhole(w, h)
    depth = plane_hit(d, np.array([0.0, 1.0, 0.0]), -1.0)
    return pack(np.broadcast_to(np.array([0.0, 1.0, 0.0]), d.shape), depth, np.where(np.isinf(depth), -1, 0).astype(np.int32))


SETS = {"planes": planes_at_an_edge, "sphere": sphere_on_a_floor, "floor": slanted_floor}


def noisy_image(features, w, h, seed):
    """A display image: a colour that depends on the material and, smoothly, on the position, plus noise."""
    rng = np.random.default_rng(seed)
    m = features["materialIdx"].reshape(h, w)
    ys, xs = np.mgrid[0:h, 0:w]
    base = np.stack([90 + 50 * m + 0.8 * xs, 120 - 30 * m + 0.5 * ys, 60 + 40 * (m == 0) + 0.3 * (xs + ys)], axis=-1)
    rgba = np.full((h, w, 4), 255, dtype=np.uint8)
    rgba[..., :3] = np.clip(base + rng.normal(0, 25, size=base.shape), 0, 255).astype(np.uint8)
    rgba[..., 3] = rng.integers(0, 256, size=(h, w))   # the input's alpha is not read
    return rgba.reshape(-1, 4)


# ---- the independent model: DESIGN.md §3.22 in float64 numpy, vectorised per tap -------------------------------------------------
def model(lo_rgba, f_lo, w, h, f_hi, p):
    """-> (colour (hiH*hiW, 3), weight sum (hiH*hiW,), counted (hiH*hiW, 4) bool, tap index (hiH*hiW, 4), inside (hiH*hiW, 4))."""
    f = p.factor
    hw, hh = w * f, h * f
    c = lo_rgba.reshape(h, w, 4)[..., :3].astype(np.float64)
    n_lo, z_lo, m_lo = (f_lo["normal"].reshape(h, w, 3).astype(np.float64), f_lo["depth"].reshape(h, w).astype(np.float64),
                        f_lo["materialIdx"].reshape(h, w).astype(np.int64))
    n, z, m = (f_hi["normal"].reshape(hh, hw, 3).astype(np.float64), f_hi["depth"].reshape(hh, hw).astype(np.float64),
               f_hi["materialIdx"].reshape(hh, hw).astype(np.int64))
    hit = m >= 0
    with np.errstate(invalid="ignore"):
        def slope(axis):
            a = np.full((hh, hw), np.inf)
            b = np.full((hh, hw), np.inf)
            d = np.abs(np.diff(z, axis=axis))
            if axis == 1:
                a[:, 1:], b[:, :-1] = d, d
            else:
                a[1:, :], b[:-1, :] = d, d
            g = np.fmin(a, b)
            return np.where(np.isfinite(g), g, 0.0)
        gx, gy = slope(1), slope(0)
    Y, X = np.mgrid[0:hh, 0:hw]
    ux, uy = (X + 0.5) / f - 0.5, (Y + 0.5) / f - 0.5
    x0, y0 = np.floor(ux).astype(np.int64), np.floor(uy).astype(np.int64)
    fx, fy = ux - x0, uy - y0
    cn = c[np.clip(np.rint(uy).astype(np.int64), 0, h - 1), np.clip(np.rint(ux).astype(np.int64), 0, w - 1)]
    total, wsum = np.zeros((hh, hw, 3)), np.zeros((hh, hw))
    lo, hi = np.full((hh, hw, 3), np.inf), np.full((hh, hw, 3), -np.inf)
    counted, index, inside_all = [], [], []
    sn, sd = float(p.sigmaNormal), float(p.sigmaDepth)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            b = (fx if i else 1 - fx) * (fy if j else 1 - fy)
            ok = inside & (m_lo[cy, cx] == m)
            cq, nq, zq = c[cy, cx], n_lo[cy, cx], z_lo[cy, cx]
            ax, ay = np.abs(ux - qx) * f, np.abs(uy - qy) * f   # the tap's offset in hi-res pixels
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                e_n = np.maximum(0.0, 1.0 - (n * nq).sum(-1)) / sn
                e_z = np.abs(z - zq) / np.maximum(sd * (gx * ax + gy * ay) + 1e-3 * z, 1e-30)
                e = np.where(hit & ok, e_n + e_z, 0.0)
                wq = np.where(ok, b * np.exp(-e), 0.0)
            wq = np.where(wq > 0, wq, 0.0)
            used = wq > 0
            total += wq[..., None] * (cq - cn)
            wsum += wq
            lo = np.where(used[..., None], np.minimum(lo, cq), lo)
            hi = np.where(used[..., None], np.maximum(hi, cq), hi)
            counted.append(used.reshape(-1))
            index.append((cy * w + cx).reshape(-1))
            inside_all.append(inside.reshape(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((wsum > 0)[..., None], np.clip(cn + total / wsum[..., None], lo, hi), cn)
    return out.reshape(-1, 3), wsum.reshape(-1), np.stack(counted, 1), np.stack(index, 1), np.stack(inside_all, 1)


@pytest.mark.parametrize("name", sorted(SETS))
def test_host_build_agrees_with_the_float64_model(name):
    worst, worst_w, byte_steps = 0.0, 0.0, 0
    for w, h in SHAPES:
        f_lo = SETS[name](w, h)
        lo = noisy_image(f_lo, w, h, seed=7)
        for f in FACTORS:
            p = params(factor=f)
            f_hi = SETS[name](w * f, h * f)
            rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, p)
            want, want_w, _, _, _ = model(lo, f_lo, w, h, f_hi, p)
            got = np.stack([flt["r"], flt["g"], flt["b"]], 1).astype(np.float64)
            diff = float(np.abs(got - want).max())
            worst, worst_w = max(worst, diff), max(worst_w, float(np.abs(flt["weight"] - want_w).max()))
            assert diff <= MODEL_TOLERANCE, (w, h, f, diff)
            assert (rgba[:, 3] == 255).all()
            want_bytes = np.floor(want + 0.5).astype(np.int64)
            differs = rgba[:, :3].astype(np.int64) != want_bytes
            tie = np.abs(want - np.floor(want) - 0.5) <= MODEL_TOLERANCE   # the model's value is within the bound of k + 0.5
            assert not (differs & ~tie).any(), (w, h, f)
            assert np.abs(rgba[:, :3].astype(np.int64) - want_bytes).max() <= 1
            byte_steps += int(differs.sum())
    print(f"{name}: largest |host - model| = {worst:.3g} (weights {worst_w:.3g}), bytes one step apart = {byte_steps}")
    assert worst_w <= 4 * MEASURED_MAX_WEIGHT_DIFF


# ---- exact properties ---------------------------------------------------------------------------------------------------------
CASES = [(name, w, h, f) for name in sorted(SETS) for (w, h) in SHAPES[:1] for f in FACTORS]


@pytest.mark.parametrize("name,w,h,f", CASES)
def test_constant_image_stays_constant(name, w, h, f):
    f_lo, f_hi = SETS[name](w, h), SETS[name](w * f, h * f)
    lo = np.tile(np.array([37, 141, 250, 9], dtype=np.uint8), (w * h, 1))
    rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, params(factor=f))
    assert (rgba == [37, 141, 250, 255]).all()
    assert (flt["r"] == 37).all() and (flt["g"] == 141).all() and (flt["b"] == 250).all()


@pytest.mark.parametrize("name,w,h,f", CASES)
def test_output_stays_inside_the_taps_of_its_material(name, w, h, f):
    """Every channel lies in [min, max] of the in-frame lo taps that share P's material: two materials never mix. A hi pixel whose
    material no tap shares gets the nearest lo pixel's colour and weight 0."""
    f_lo, f_hi = SETS[name](w, h), SETS[name](w * f, h * f)
    lo = noisy_image(f_lo, w, h, seed=3)
    rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, params(factor=f))
    _, _, _, index, inside = model(lo, f_lo, w, h, f_hi, params(factor=f))
    same = inside & (f_lo["materialIdx"][index] == f_hi["materialIdx"][:, None])
    colours = lo[:, :3].astype(np.float64)[index]                       # (N, 4 taps, 3)
    low = np.where(same[..., None], colours, np.inf).min(axis=1)
    high = np.where(same[..., None], colours, -np.inf).max(axis=1)
    got = np.stack([flt["r"], flt["g"], flt["b"]], 1).astype(np.float64)
    shared = same.any(axis=1)
    assert shared.any()
    assert (got[shared] >= low[shared]).all() and (got[shared] <= high[shared]).all()
    assert (rgba[shared, :3] >= low[shared]).all() and (rgba[shared, :3] <= high[shared]).all()
    hw = w * f
    Y, X = np.divmod(np.arange(len(f_hi)), hw)
    nearest = lo[(Y // f) * w + X // f]
    orphan = ~shared
    assert (rgba[orphan, :3] == nearest[orphan, :3]).all() and (flt["weight"][orphan] == 0).all()
    assert (flt["weight"][shared] > 0).all()


def uniform_features(n, material=-1, depth=np.inf, normal=(0.0, 0.0, 0.0)):
    f = np.zeros(n, dtype=ptss.FEATURE_DTYPE)
    f["materialIdx"], f["depth"], f["normal"], f["albedo"] = material, depth, normal, 0.5
    return f


@pytest.mark.parametrize("f", FACTORS)
def test_border_pixels_skip_the_outside_taps(f):
    """Between misses only the bilinear weight counts, so the weight sum of a hi pixel is the bilinear weight of its in-frame taps:
    1 in the interior, less along the border, where x0 = -1 or x0 + 1 = width; a corner keeps one tap and takes its colour."""
    w, h = 3, 2
    lo = np.zeros((h, w, 4), dtype=np.uint8)
    lo[..., 0] = np.arange(w)[None, :] * 100
    lo[..., 1] = np.arange(h)[:, None] * 200
    rgba, flt = ptss.probe_upsample(lo.reshape(-1, 4), uniform_features(w * h), w, h, uniform_features(w * h * f * f), params(factor=f))
    hw, hh = w * f, h * f
    weight = flt["weight"].reshape(hh, hw)

    def axis_weight(X, size):   # Fractions: the bilinear weight of the taps of one axis that lie inside
        u = Fraction(2 * X + 1, 2 * f) - Fraction(1, 2)
        x0 = u.numerator // u.denominator
        fr = u - x0
        return (1 - fr if 0 <= x0 < size else 0) + (fr if 0 <= x0 + 1 < size else 0)

    for Y in range(hh):
        for X in range(hw):
            want = float(axis_weight(X, w) * axis_weight(Y, h))
            assert abs(weight[Y, X] - want) <= 3e-7, (X, Y)
            assert (want < 1) == (X < f // 2 or X >= hw - f // 2 or Y < f // 2 or Y >= hh - f // 2)
    out = rgba.reshape(hh, hw, 4)
    for (Y, X), (y, x) in {(0, 0): (0, 0), (0, hw - 1): (0, w - 1), (hh - 1, 0): (h - 1, 0), (hh - 1, hw - 1): (h - 1, w - 1)}.items():
        assert tuple(out[Y, X, :3]) == tuple(lo[y, x, :3])
    # inside, the image is the bilinear interpolation of the lo image
    want_r = np.array([[float((Fraction(2 * X + 1, 2 * f) - Fraction(1, 2)) * 100) for X in range(hw)] for _ in range(hh)])
    ok = (np.arange(hw) >= f // 2) & (np.arange(hw) < hw - f // 2)
    assert np.abs(flt["r"].reshape(hh, hw)[:, ok] - want_r[:, ok]).max() <= 1e-4


def test_factor_one_is_the_identity_with_alpha_255():
    w, h = 33, 17
    f_lo = sphere_on_a_floor(w, h)
    lo = noisy_image(f_lo, w, h, seed=5)
    for f_hi in (f_lo, planes_at_an_edge(w, h), uniform_features(w * h)):   # whatever the features say: every tap is the pixel itself
        rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, params(factor=1))
        assert (rgba[:, :3] == lo[:, :3]).all() and (rgba[:, 3] == 255).all()
        assert (np.stack([flt["r"], flt["g"], flt["b"]], 1) == lo[:, :3]).all()
    _, flt = ptss.probe_upsample(lo, f_lo, w, h, f_lo, params(factor=1))
    assert (np.abs(flt["weight"] - 1) <= 1e-5).all()   # exp(-(1 - n . n) / sigmaNormal): unit normals to float32 precision
    _, flt = ptss.probe_upsample(lo, uniform_features(w * h), w, h, uniform_features(w * h), params(factor=1))
    assert (flt["weight"] == 1).all()


def test_underflowed_weight_contributes_nothing():
    """Two lo pixels of one material; the right one lies so far behind the hi pixel's surface that its weight underflows: it adds
    nothing to the sum, to the weight or to the clamp, although its bilinear weight is the larger one."""
    w, h, f = 2, 1, 2
    f_lo = uniform_features(2, material=0, depth=2.0, normal=(0, 0, 1))
    f_lo["depth"][1] = 2.0e6
    f_hi = uniform_features(4 * 2, material=0, depth=2.0, normal=(0, 0, 1))
    lo = np.array([[10, 20, 30, 0], [200, 210, 220, 0]], dtype=np.uint8)
    rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, params(factor=f))
    out, weight = rgba.reshape(2, 4, 4), flt["weight"].reshape(2, 4)
    # hi pixels 0..2 have the left pixel among their taps: its colour exactly, its bilinear weight alone (0.75 of it: the one row)
    for X, b in ((0, 0.75), (1, 0.75), (2, 0.25)):
        assert tuple(out[0, X, :3]) == (10, 20, 30)
        assert abs(weight[0, X] - 0.75 * b) <= 1e-6, (X, weight[0, X])
    # hi pixel 3 sees only the right pixel (x0 = 1, x0 + 1 outside), which does not count: the nearest colour, weight 0
    assert tuple(out[0, 3, :3]) == (200, 210, 220) and weight[0, 3] == 0
    # the same pixel with a depth that matches counts again
    f_lo["depth"][1] = 2.0
    rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, params(factor=f))
    assert abs(flt["weight"].reshape(2, 4)[0, 1] - 0.75) <= 1e-6 and 10 < rgba.reshape(2, 4, 4)[0, 1, 0] < 200


def test_two_materials_never_mix():
    """A vertical material boundary that falls between two lo pixels: every hi pixel takes the colour of its own side exactly."""
    w, h, f = 4, 2, 2
    f_lo = uniform_features(w * h, material=0, depth=3.0, normal=(0, 0, 1))
    f_lo["materialIdx"].reshape(h, w)[:, 2:] = 1
    f_hi = uniform_features(w * h * f * f, material=0, depth=3.0, normal=(0, 0, 1))
    f_hi["materialIdx"].reshape(h * f, w * f)[:, 5:] = 1    # the true edge, seen at full size: one hi pixel to the right of the lo edge
    lo = np.zeros((h, w, 4), dtype=np.uint8)
    lo[:, :2, :3], lo[:, 2:, :3] = (20, 40, 60), (220, 200, 180)
    rgba, flt = ptss.probe_upsample(lo.reshape(-1, 4), f_lo, w, h, f_hi, params(factor=f))
    out = rgba.reshape(h * f, w * f, 4)
    assert (out[:, :5, :3] == (20, 40, 60)).all() and (out[:, 5:, :3] == (220, 200, 180)).all()
    assert (flt["weight"] > 0).all()


def test_a_surface_the_small_frame_did_not_see_takes_the_nearest_colour():
    """Thin geometry seen only at full size: a one-pixel column of another material in the hi-res features, absent from the lo ones."""
    w, h, f = 4, 3, 3
    f_lo = uniform_features(w * h, material=0, depth=3.0, normal=(0, 0, 1))
    f_hi = uniform_features(w * h * f * f, material=0, depth=3.0, normal=(0, 0, 1))
    f_hi["materialIdx"].reshape(h * f, w * f)[:, 7] = 5
    rng = np.random.default_rng(1)
    lo = rng.integers(0, 256, size=(h * w, 4)).astype(np.uint8)
    rgba, flt = ptss.probe_upsample(lo, f_lo, w, h, f_hi, params(factor=f))
    out, weight = rgba.reshape(h * f, w * f, 4), flt["weight"].reshape(h * f, w * f)
    for Y in range(h * f):
        assert tuple(out[Y, 7, :3]) == tuple(lo[(Y // f) * w + 7 // f, :3]) and weight[Y, 7] == 0
    assert (np.delete(weight, 7, axis=1) > 0).all()
