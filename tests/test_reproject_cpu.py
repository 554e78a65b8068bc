"""Reprojected history without a GPU (ptss_reproject / ptss_denoise_history): the new C-ABI symbols and struct
layouts, the argument checks that must not touch a device, an independent float64 restatement of the formulas on three analytic
feature sets seen from two poses of a real ptss_camera, and exact properties of the arithmetic (csrc/ptreproject.h through
ptss_probe_reproject).

The float64 model leaves out the pixels at which a threshold decision (a validity test, the floor of a tap coordinate, the frame
and coverage tests) lies within a relative 1e-4 of its threshold: float32 may legitimately decide them the other way. At most 2 %
of a case's pixels may be left out (measured: 0.26 % to 0.98 %). Measured on the host build (x86-64) over the remaining pixels of the
six cases, largest |host - model|: colour 4.52e-04 on the 0..255 scale (planes, w+g), weight 6.02e-04 on weights up to 68 (planes,
d+f); the tolerances are four times that."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptss
from ptss_types import HistoryEntry, ReprojectParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

MEASURED_MAX_COLOUR = 4.52e-04
MEASURED_MAX_WEIGHT = 6.02e-04
COLOUR_TOLERANCE = 4 * MEASURED_MAX_COLOUR
WEIGHT_TOLERANCE = 4 * MEASURED_MAX_WEIGHT
assert COLOUR_TOLERANCE < 0.5   # beyond that the model and the header are not the same arithmetic
NEAR_TIE = 1e-4
MAX_LEFT_OUT = 0.02

W, H = 64, 48


def params(**kw):
    return ptss.default_reproject_params(**kw)


# ---- symbols, layouts, defaults, argument checks ------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    dev = C.CDLL(ptss.DEVICE_LIB)
    host = C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_default_reproject_params", "ptss_reproject", "ptss_denoise_history"):
        assert hasattr(dev, name), name
    for name in ("ptss_probe_reproject", "ptss_probe_denoise_history"):
        assert hasattr(host, name), name


FIELDS = {
    "ptss_history_entry": (HistoryEntry, ["r", "g", "b", "weight"]),
    "ptss_reproject_params": (ReprojectParams, ["structSize", "cosNormal", "depthTolerance", "maxHistory", "minCoverage"]),
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
    if struct == "ptss_history_entry":
        assert got[0] == 16 == ptss.HISTORY_DTYPE.itemsize
        assert got[1:] == [ptss.HISTORY_DTYPE.fields[n][1] for n in names]


def test_default_params():
    p = ReprojectParams()
    L = ptss.device_lib()
    assert L.ptss_default_reproject_params(None) == -1
    assert L.ptss_default_reproject_params(C.byref(p)) == 0
    assert p.structSize == C.sizeof(ReprojectParams)
    assert (p.cosNormal, p.depthTolerance, p.maxHistory, p.minCoverage) == (np.float32(0.9), np.float32(0.02), 64.0, 0.25)


BAD_PARAMS = [dict(cosNormal=1.5), dict(cosNormal=-1.5), dict(cosNormal=float("nan")), dict(depthTolerance=-0.01),
              dict(depthTolerance=float("inf")), dict(depthTolerance=float("nan")), dict(maxHistory=-1.0), dict(maxHistory=float("inf")),
              dict(maxHistory=float("nan")), dict(minCoverage=-0.1), dict(minCoverage=1.5), dict(minCoverage=float("nan"))]


def test_argument_checks_without_a_device():
    """Null pointers, a wrong structSize, parameters out of range and aliased histories are answered on the host."""
    L = ptss.device_lib()
    buf, other = (C.c_float * 64)(), (C.c_float * 64)()
    ctx = C.c_void_p(1)   # never dereferenced: every call below fails before the context is looked at
    cam = ptss.default_camera()
    good = params()

    def call(ctx=ctx, now=buf, cam=cam, fprev=buf, hprev=buf, p=good, out=other):
        return L.ptss_reproject(ctx, now, C.byref(cam) if cam is not None else None, fprev, hprev, C.byref(p) if p is not None else None, out, None)

    assert call(ctx=None) == -1
    assert call(now=None) == -1
    assert call(out=None) == -1
    assert call(p=None) == -1
    assert call(cam=None) == -1 and call(fprev=None) == -1   # a history needs its camera and its features
    assert call(out=buf) == -1                               # dev_history_out == dev_history_prev
    assert b"dev_history_prev" in L.ptss_last_error_detail()
    bad = params()
    bad.structSize += 4
    assert call(p=bad) == -1
    for kw in BAD_PARAMS:
        assert call(p=params(**kw)) == -1, kw
        assert call(hprev=None, p=params(**kw)) == -1, kw   # with or without a history
    dn = ptss.default_denoise_params()
    pix = (C.c_ubyte * 64)()
    assert L.ptss_denoise_history(None, buf, buf, C.byref(dn), pix, None) == -1
    assert L.ptss_denoise_history(ctx, None, buf, C.byref(dn), pix, None) == -1
    assert L.ptss_denoise_history(ctx, buf, None, C.byref(dn), pix, None) == -1
    assert L.ptss_denoise_history(ctx, buf, buf, None, pix, None) == -1
    assert L.ptss_denoise_history(ctx, buf, buf, C.byref(dn), None, None) == -1
    assert L.ptss_denoise_history(ctx, buf, buf, C.byref(ptss.default_denoise_params(levels=7)), pix, None) == -1
    dn.structSize -= 4
    assert L.ptss_denoise_history(ctx, buf, buf, C.byref(dn), pix, None) == -1


def test_probe_argument_checks():
    Hh = ptss.host_lib()
    acc = np.zeros(12, dtype=np.uint32)
    feat = np.zeros(4, dtype=ptss.FEATURE_DTYPE)
    hist, out = np.ones(4, dtype=ptss.HISTORY_DTYPE), np.zeros(4, dtype=ptss.HISTORY_DTYPE)
    cam = ptss.default_camera()
    a, f, h, o = acc.ctypes.data_as(C.POINTER(C.c_uint32)), feat.ctypes.data_as(C.c_void_p), hist.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    good = params()

    def call(a=a, n=1, now=cam, prev=cam, w=2, fnow=f, fprev=f, hprev=h, p=good, out=o):
        return Hh.ptss_probe_reproject(a, 1.0, n, C.byref(now) if now is not None else None, C.byref(prev) if prev is not None else None, w, 2,
                                       fnow, fprev, hprev, C.byref(p) if p is not None else None, out)

    assert call() == 0
    assert call(prev=None, fprev=None, hprev=None) == 0   # no history
    for kw in (dict(a=None), dict(now=None), dict(fnow=None), dict(out=None), dict(p=None), dict(w=0), dict(n=-1), dict(prev=None),
               dict(fprev=None), dict(out=h)):
        assert call(**kw) < 0, kw
    bad = params()
    bad.structSize -= 4
    assert call(p=bad) < 0
    for kw in BAD_PARAMS:
        assert call(p=params(**kw)) < 0, kw
    dn = ptss.default_denoise_params(levels=1)
    rgba = np.zeros(16, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    assert Hh.ptss_probe_denoise_history(h, f, 2, 2, C.byref(dn), rgba, None) == 0
    assert Hh.ptss_probe_denoise_history(None, f, 2, 2, C.byref(dn), rgba, None) < 0
    assert Hh.ptss_probe_denoise_history(h, None, 2, 2, C.byref(dn), rgba, None) < 0
    assert Hh.ptss_probe_denoise_history(h, f, 2, 2, C.byref(ptss.default_denoise_params(levels=7)), rgba, None) < 0


# ---- analytic feature sets in world space, seen through the eye rays of a real camera ---------------------------------------
def camera(keys=""):
    cam = ptss.default_camera()
    for k in keys:
        assert ptss.move_camera(cam, k)
    return cam


_RAYS = {}


def rays_of(keys):
    """(origin (3,), unit directions (H*W, 3)) of ptss.camera_rays for the default camera moved by `keys`, as float64."""
    if keys not in _RAYS:
        r = ptss.camera_rays(camera(keys), W, H)
        _RAYS[keys] = (r[0, 0:3].astype(np.float64), r[:, 4:7].astype(np.float64))
    return _RAYS[keys]


def pack(normal, depth, material):
    f = np.zeros(len(depth), dtype=ptss.FEATURE_DTYPE)
    f["normal"], f["depth"], f["materialIdx"] = normal, depth, material
    f["albedo"] = 0.5
    miss = f["materialIdx"] < 0
    f["normal"][miss] = 0
    f["depth"][miss] = np.inf
    return f


def plane_hit(o, d, n, c):
    """Distance along rays o + t d to the plane n . X = c (inf where it is not ahead)."""
    nd = d @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (c - o @ n) / nd
    return np.where((nd != 0) & (t > 0), t, np.inf)


def planes_at_an_edge(o, d):
    nl, nr = np.array([0.6, 0.0, 0.8]), np.array([-0.6, 0.0, 0.8])
    tl, tr = plane_hit(o, d, nl, -4.0), plane_hit(o, d, nr, -4.0)
    left = tl <= tr
    depth = np.where(left, tl, tr)
    return pack(np.where(left[:, None], nl, nr), depth, np.where(np.isinf(depth), -1, 0))


def sphere_on_a_floor(o, d):
    centre, r = np.array([0.0, 0.0, -4.0]), 1.0
    oc = o - centre
    b = -(d @ oc)
    disc = b * b - (oc @ oc - r * r)
    ts = np.where(disc > 0, b - np.sqrt(np.maximum(disc, 0)), np.inf)
    ts = np.where(ts > 0, ts, np.inf)
    tf = plane_hit(o, d, np.array([0.0, 1.0, 0.0]), -1.0)
    depth = np.minimum(ts, tf)
    material = np.where(np.isinf(depth), -1, np.where(ts <= tf, 1, 0))
    with np.errstate(invalid="ignore"):
        ns = (o + d * ts[:, None] - centre) / r
    normal = np.where((material == 1)[:, None], ns, np.array([0.0, 1.0, 0.0]))
    return pack(np.nan_to_num(normal), depth, material)


def slanted_floor(o, d):
    depth = plane_hit(o, d, np.array([0.0, 1.0, 0.0]), -1.0)
    return pack(np.broadcast_to(np.array([0.0, 1.0, 0.0]), d.shape), depth, np.where(np.isinf(depth), -1, 0))


SETS = {"planes": planes_at_an_edge, "sphere": sphere_on_a_floor, "floor": slanted_floor}
# A 'w' step alone leaves every miss exactly on its own pixel centre (a direction does not change under a translation): the tap
# coordinates are then integers, every one a near tie of the floor, and the floor and sphere sets are left out by half. So the
# second move is a 'w' step plus one 'g' turn.
MOVES = {"d+f": "df", "w+g": "wg"}


def features_of(name, keys):
    return SETS[name](*rays_of(keys))


def noisy_accum(features, ticks, seed):
    rng = np.random.default_rng(seed)
    m = features["materialIdx"].reshape(H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    base = np.stack([90 + 50 * m + 0.8 * xs, 120 - 30 * m + 0.5 * ys, 60 + 40 * (m == 0) + 0.3 * (xs + ys)], axis=-1)
    acc = np.zeros((H, W, 3), dtype=np.uint32)
    for _ in range(ticks):
        acc += np.clip(base + rng.normal(0, 35, size=base.shape), 0, 255).astype(np.uint32)
    return acc.reshape(-1, 3)


def noisy_history(features, seed, broken=True):
    """Colours that depend on the material and the position, weights from below 1 to above maxHistory; with `broken`, a few entries
    of weight 0, of negative weight and with a NaN or an infinity, which must not count."""
    rng = np.random.default_rng(seed)
    m = features["materialIdx"].reshape(H, W)
    ys, xs = np.mgrid[0:H, 0:W]
    base = np.stack([60 + 40 * m + 1.1 * xs, 150 - 20 * m - 0.7 * ys, 80 + 30 * (m == 0) + 0.4 * (xs - ys)], axis=-1)
    colour = np.clip(base + rng.normal(0, 12, size=base.shape), 0, 255).reshape(-1, 3)
    h = np.zeros(W * H, dtype=ptss.HISTORY_DTYPE)
    h["r"], h["g"], h["b"] = colour[:, 0], colour[:, 1], colour[:, 2]
    h["weight"] = rng.uniform(0.5, 90.0, size=W * H)
    if broken:
        pick = rng.permutation(W * H)
        h["weight"][pick[:40]] = 0.0
        h["weight"][pick[40:60]] = -3.0
        h["g"][pick[60:80]] = np.nan
        h["b"][pick[80:90]] = np.inf
        h["weight"][pick[90:100]] = np.nan
    return h


# ---- the independent model: §3.19 in float64 numpy ------------------------------------------------------------------------------
def quat_rotate(q, v):
    """glm's quat * vec3 for q = (x, y, z, w)."""
    u = np.asarray(q[:3], dtype=np.float64)
    uv = np.cross(u, v)
    return v + 2.0 * (q[3] * uv + np.cross(u, uv))


def near(value, threshold, scale=None):
    scale = np.abs(threshold) if scale is None else scale
    return np.abs(value - threshold) <= NEAR_TIE * scale


def model(accum, inverse_ticks, n, keys_now, cam_prev, f_now, f_prev, hist, p):
    """-> colour (N, 3), weight (N,), near-tie mask, history weight w, disoccluded mask."""
    N = W * H
    c = accum.astype(np.float64) * float(np.float32(inverse_ticks))
    o_now, d = rays_of(keys_now)
    m = f_now["materialIdx"].astype(np.int64)
    hit = m >= 0
    o_prev = np.array([cam_prev.position.x, cam_prev.position.y, cam_prev.position.z], dtype=np.float64)
    q = cam_prev.rotation
    conj = np.array([-q.x, -q.y, -q.z, q.w], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(hit[:, None], o_now + d * f_now["depth"].astype(np.float64)[:, None] - o_prev, d)
    rng_ = np.linalg.norm(v, axis=1)
    l = quat_rotate(conj, v)
    s = -2.0 * np.tan(float(cam_prev.fieldOfView) / 2.0)
    front = l[:, 2] * float(cam_prev.zNear) > 0
    tie = near(l[:, 2], 0.0, np.linalg.norm(l, axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        fx = (l[:, 0] / (l[:, 2] * s) + 0.5) * W - 0.5
        fy = (l[:, 1] / (l[:, 2] * s * (H / W)) + 0.5) * H - 0.5
    inside = front & (fx >= -1) & (fx < W) & (fy >= -1) & (fy < H)
    tie |= front & (near(fx, -1.0) | near(fx, float(W)) | near(fy, -1.0) | near(fy, float(H)))
    fx, fy = np.where(inside, fx, 0.0), np.where(inside, fy, 0.0)
    x0, y0 = np.floor(fx), np.floor(fy)
    tie |= inside & (near(fx, np.rint(fx), np.maximum(1.0, np.abs(np.rint(fx)))) | near(fy, np.rint(fy), np.maximum(1.0, np.abs(np.rint(fy)))))
    tx, ty = fx - x0, fy - y0
    mp, np_, zp = f_prev["materialIdx"].astype(np.int64), f_prev["normal"].astype(np.float64), f_prev["depth"].astype(np.float64)
    hc = np.stack([hist["r"], hist["g"], hist["b"]], axis=-1).astype(np.float64)
    hw = hist["weight"].astype(np.float64)
    usable = np.isfinite(hc).all(axis=1) & np.isfinite(hw) & (hw > 0)
    normal = f_now["normal"].astype(np.float64)
    B, csum, wsum = np.zeros(N), np.zeros((N, 3)), np.zeros(N)
    lo, hi = c.copy(), c.copy()
    nearer = np.zeros(N, dtype=bool)      # some tap of the previous frame saw a nearer surface of this material and normal
    seen = np.zeros(N, dtype=bool)        # some tap saw the point itself
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
            b = np.where(i, tx, 1 - tx) * np.where(j, ty, 1 - ty)
            ok = inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (b > 0)
            qi = np.where(ok, qy * W + qx, 0)
            ok &= mp[qi] == m
            with np.errstate(invalid="ignore"):
                cos = (normal * np_[qi]).sum(axis=1)
                off = np.abs(zp[qi] - rng_)
                tol = p.depthTolerance * rng_
                tie |= ok & hit & (near(cos, p.cosNormal) | near(off, tol))
                same = ~hit | ((cos >= p.cosNormal) & (off <= tol))
                nearer |= ok & hit & (cos >= p.cosNormal) & (zp[qi] < rng_ - tol)
            seen |= ok & same
            ok &= same & usable[qi]
            B += np.where(ok, b, 0.0)
            csum += np.where(ok[:, None], b[:, None] * np.nan_to_num(hc[qi], posinf=0.0, neginf=0.0), 0.0)
            wsum += np.where(ok, b * np.nan_to_num(hw[qi], posinf=0.0), 0.0)
            lo = np.where(ok[:, None], np.minimum(lo, hc[qi]), lo)
            hi = np.where(ok[:, None], np.maximum(hi, hc[qi]), hi)
    have = B > 0
    tie |= have & near(B, p.minCoverage)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(have[:, None], csum / B[:, None], c)
        w = np.where(have, np.minimum(wsum / B, p.maxHistory), 0.0)
    w = np.where(B < p.minCoverage, 0.0, w)
    total = n + w
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where((w > 0)[:, None], c + (h - c) * (w / total)[:, None], c)
    out = np.clip(out, lo, hi)
    return out, total, tie, w, hit & inside & nearer & ~seen


def colours(entries):
    return np.stack([entries["r"], entries["g"], entries["b"]], axis=-1)


def case(name, move, n=4, seed=7, broken=True, **kw):
    keys = MOVES[move]
    f_prev, f_now = features_of(name, ""), features_of(name, keys)
    accum = noisy_accum(f_now, n, seed)
    hist = noisy_history(f_prev, seed + 1, broken)
    p = params(**kw)
    inv = np.float32(1.0) / np.float32(n)
    got = ptss.probe_reproject(accum, inv, n, camera(keys), camera(""), W, H, f_now, f_prev, hist, p)
    return got, model(accum, inv, n, keys, camera(""), f_now, f_prev, hist, p), accum, inv


@pytest.mark.parametrize("move", sorted(MOVES))
@pytest.mark.parametrize("name", sorted(SETS))
def test_host_build_agrees_with_the_float64_model(name, move):
    got, (want, want_weight, tie, w, _), _, _ = case(name, move)
    left_out = float(tie.mean())
    keep = ~tie
    dc = float(np.abs(colours(got).astype(np.float64) - want)[keep].max())
    dw = float(np.abs(got["weight"].astype(np.float64) - want_weight)[keep].max())
    print(f"{name} {move}: left out {100 * left_out:.2f} %, with history {int((w > 0).sum())} of {W * H}, "
          f"largest |host - model| colour {dc:.3g}, weight {dw:.3g}")
    assert left_out <= MAX_LEFT_OUT
    assert (w > 0).sum() > 0.3 * W * H   # the case does reproject
    assert dc <= COLOUR_TOLERANCE and dw <= WEIGHT_TOLERANCE


# ---- exact properties ---------------------------------------------------------------------------------------------------------
def current(accum, inv, n):
    """(c, n): what a pixel without usable history gets, bit for bit."""
    out = np.zeros(len(accum), dtype=ptss.HISTORY_DTYPE)
    c = accum.astype(np.float32) * np.float32(inv)
    out["r"], out["g"], out["b"], out["weight"] = c[:, 0], c[:, 1], c[:, 2], np.float32(n)
    return out


@pytest.mark.parametrize("name", sorted(SETS))
def test_no_history_and_zero_weight_give_the_current_image(name):
    f_prev, f_now = features_of(name, ""), features_of(name, "df")
    for n, inv in ((0, 1.0), (1, 1.0), (3, 1.0 / 3.0), (28, 1.0 / 28.0)):
        accum = noisy_accum(f_now, max(n, 1), seed=3)
        want = current(accum, inv, n)
        none = ptss.probe_reproject(accum, np.float32(inv), n, camera("df"), None, W, H, f_now, None, None)
        assert none.tobytes() == want.tobytes(), (name, n)
        hist = noisy_history(f_prev, 5)
        hist["weight"] = 0.0
        zero = ptss.probe_reproject(accum, np.float32(inv), n, camera("df"), camera(""), W, H, f_now, f_prev, hist)
        assert zero.tobytes() == want.tobytes(), (name, n)


@pytest.mark.parametrize("move", ["", "df", "w", "wg"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_a_constant_image_stays_constant(name, move):
    f_prev, f_now = features_of(name, ""), features_of(name, move)
    rng = np.random.default_rng(2)
    for value, n in (((1, 3, 5), 2), ((100, 101, 255), 1), ((77, 310, 5), 3)):
        accum = np.tile(np.array(value, dtype=np.uint32), (W * H, 1))
        inv = np.float32(1.0) / np.float32(n)
        c = np.array(value, dtype=np.float32) * inv
        hist = np.zeros(W * H, dtype=ptss.HISTORY_DTYPE)
        hist["r"], hist["g"], hist["b"] = c
        hist["weight"] = rng.uniform(0.5, 90.0, size=W * H)
        got = ptss.probe_reproject(accum, inv, n, camera(move), camera(""), W, H, f_now, f_prev, hist)
        assert (colours(got) == c).all(), (value, n)
        assert (got["weight"] > n).sum() > 0.3 * W * H


def test_two_materials_never_mix():
    """Every output channel of a material lies within the hull of the current colours and the history colours of THAT material."""
    rng = np.random.default_rng(5)
    f_prev, f_now = features_of("sphere", ""), features_of("sphere", "df")
    ranges = {0: (10, 60), 1: (150, 250), -1: (70, 120)}
    accum = np.zeros((W * H, 3), dtype=np.uint32)
    hist = np.zeros(W * H, dtype=ptss.HISTORY_DTYPE)
    hist["weight"] = 50.0
    for k, (a, b) in ranges.items():
        now, prev = f_now["materialIdx"] == k, f_prev["materialIdx"] == k
        assert now.sum() > 20 and prev.sum() > 20
        accum[now] = rng.integers(a, b + 1, size=(int(now.sum()), 3))
        for ch in "rgb":
            hist[ch][prev] = rng.integers(a, b + 1, size=int(prev.sum()))
    got = ptss.probe_reproject(accum, 1.0, 1, camera("df"), camera(""), W, H, f_now, f_prev, hist)
    for k, (a, b) in ranges.items():
        region = colours(got)[f_now["materialIdx"] == k]
        assert a <= region.min() and region.max() <= b, k
    assert (got["weight"] > 1).sum() > 0.3 * W * H


def test_a_camera_turned_away_gives_the_current_image():
    f_prev = features_of("sphere", "")
    keys = "f" * 18   # half a turn: nothing the previous camera saw lies ahead
    f_now = features_of("sphere", keys)
    accum = noisy_accum(f_now, 4, seed=8)
    got = ptss.probe_reproject(accum, 0.25, 4, camera(keys), camera(""), W, H, f_now, f_prev, noisy_history(f_prev, 9))
    assert got.tobytes() == current(accum, 0.25, 4).tobytes()


def wall_scene(o, d):
    """A back wall z = -6 and, before its left part, a nearer wall z = -3 with x <= 0.2, of the same material and normal."""
    n = np.array([0.0, 0.0, 1.0])
    tb, tn = plane_hit(o, d, n, -6.0), plane_hit(o, d, n, -3.0)
    with np.errstate(invalid="ignore"):
        tn = np.where((o + d * np.where(np.isinf(tn), 0.0, tn)[:, None])[:, 0] <= 0.2, tn, np.inf)
    depth = np.minimum(tb, tn)
    return pack(np.broadcast_to(n, d.shape), depth, np.where(np.isinf(depth), -1, 0))


def test_a_disoccluded_point_gets_the_current_image():
    """After two steps to the right (and a turn, so that no tap coordinate stays an integer) the back wall shows a strip the near
    wall hid: exactly there the history is dropped."""
    keys = "ddf"
    f_prev, f_now = wall_scene(*rays_of("")), wall_scene(*rays_of(keys))
    accum = noisy_accum(f_now, 4, seed=12)
    hist = noisy_history(f_prev, 13, broken=False)
    p = params()
    got = ptss.probe_reproject(accum, 0.25, 4, camera(keys), camera(""), W, H, f_now, f_prev, hist, p)
    _, _, tie, w, disoccluded = model(accum, np.float32(0.25), 4, keys, camera(""), f_now, f_prev, hist, p)
    keep = ~tie
    assert tie.mean() <= MAX_LEFT_OUT
    assert (disoccluded & keep).sum() >= 40   # a strip several pixels wide over the frame's height
    dropped = got.view(np.float32).reshape(-1, 4).view(np.uint32) == current(accum, 0.25, 4).view(np.float32).reshape(-1, 4).view(np.uint32)
    dropped = dropped.all(axis=1)
    assert dropped[disoccluded & keep].all()
    assert np.array_equal(dropped[keep], (w == 0)[keep])          # ... and nowhere else than where the model has no history
    on_back_wall = (f_now["depth"] > 5.0) & keep
    assert np.array_equal(dropped[on_back_wall & (w == 0)], np.ones(int((on_back_wall & (w == 0)).sum()), dtype=bool))
    assert (got["weight"][keep & ~dropped] > 4).all()


def test_max_history_caps_the_weight():
    f = features_of("planes", "")
    accum = noisy_accum(f, 4, seed=4)
    hist = noisy_history(f, 6, broken=False)
    hist["weight"] = 1000.0
    for cap in (0.0, 1.0, 64.0, 500.0):
        got = ptss.probe_reproject(accum, 0.25, 4, camera(""), camera(""), W, H, f, f, hist, params(maxHistory=cap))
        assert (got["weight"] <= np.float32(4 + cap)).all()
        assert ((got["weight"] == np.float32(4 + cap)).mean() > 0.9) or cap == 0.0
        if cap == 0.0:
            assert got.tobytes() == current(accum, 0.25, 4).tobytes()


def test_misses_and_zero_normals_give_no_nan():
    f = pack(np.zeros((W * H, 3)), np.full(W * H, np.inf), np.full(W * H, -1)).reshape(H, W)
    f["materialIdx"][5:20, 5:30] = 2       # hits with ZERO normals and a few infinite depths in between
    f["depth"][5:20, 5:30] = 2.5
    f["depth"][8, 5:30] = np.inf
    f = f.reshape(-1)
    accum = noisy_accum(f, 4, seed=1)
    hist = noisy_history(f, 2)
    for keys in ("", "df", "w"):
        for cos in (0.9, 0.0, -1.0):
            got = ptss.probe_reproject(accum, 0.25, 4, camera(keys), camera(""), W, H, f, f, hist, params(cosNormal=cos))
            flat = got.view(np.float32)
            assert np.isfinite(flat).all(), (keys, cos)
            assert colours(got).min() >= 0 and colours(got).max() <= 255
    assert (got["weight"] > 4).any()   # misses do find their history


@pytest.mark.parametrize("name", sorted(SETS))
def test_same_pose_is_the_weighted_mean(name):
    """The same camera and features on both sides: every pixel reprojects onto itself."""
    f = features_of(name, "")
    n = 4
    accum = noisy_accum(f, n, seed=21)
    hist = noisy_history(f, 22, broken=False)
    p = params()
    got = ptss.probe_reproject(accum, 0.25, n, camera(""), camera(""), W, H, f, f, hist, p)
    c = accum.astype(np.float64) * 0.25
    w = np.minimum(hist["weight"].astype(np.float64), p.maxHistory)
    want = (n * c + w[:, None] * colours(hist).astype(np.float64)) / (n + w)[:, None]
    # a pixel's own tap carries all but ~1e-5 of the bilinear weight; at a silhouette a neighbouring tap may be cut, which
    # changes nothing but that remainder
    assert np.abs(colours(got) - want).max() <= COLOUR_TOLERANCE + 255 * 2e-5
    assert np.abs(got["weight"] - (n + w)).max() <= WEIGHT_TOLERANCE + 90 * 2e-5


def test_denoise_history_probe_is_the_filter_on_the_history_colours():
    """levels = 0 converts; levels >= 1 equal ptss_probe_denoise on an accumulator that holds the same colours."""
    f = features_of("sphere", "")
    accum = noisy_accum(f, 1, seed=30)
    hist = current(accum, 1.0, 1)
    for levels in (0, 1, 3):
        p = ptss.default_denoise_params(levels=levels)
        a_rgba, a_flt = ptss.probe_denoise(accum, 1.0, f, W, H, p)
        h_rgba, h_flt = ptss.probe_denoise_history(hist, f, W, H, p)
        assert np.array_equal(a_rgba, h_rgba) and a_flt.tobytes() == h_flt.tobytes(), levels
    odd = hist.copy()
    odd["r"] = 17.25
    rgba, flt = ptss.probe_denoise_history(odd, f, W, H, ptss.default_denoise_params(levels=0))
    assert (rgba[:, 0] == 17).all() and (flt[:, 0] == np.float32(17.25)).all() and (rgba[:, 3] == 255).all()
