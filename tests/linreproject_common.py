"""Models and cases shared by tests/test_linreproject_cpu.py and tests/test_gpu_linreproject.py (ptss_reproject_linear; DESIGN.md
§3.35), independent of csrc/ptlinrp.h: the finish (steps 5 and 6: the film row and the moment row of a pixel given its reprojected
mean h, interpolated count w and variance s2) in Python integers and numpy float32, exactly; the lookup (steps 1 to 4) as a float64
restatement of the formulas, with the pixels marked at which float32 may decide a threshold the other way."""
from fractions import Fraction

import numpy as np

import ptss
from lindenoise_common import is_splat, model_counts, model_fixed_mean, model_means, round_half_even, words
from linear_common import MASK
from linstats_common import model_D

F32 = np.float32
LO_MASK = (1 << 40) - 1
NEAR_TIE = 1e-4
SEEDED, OFF_FILM, NO_TAP = 0, 1, 2


# ---- steps 5 and 6, exactly ---------------------------------------------------------------------------------------------------------------------
def model_history_count(w, max_history):
    """K: the float32 w rounded to nearest, ties to even, capped."""
    return min(round_half_even(Fraction(float(F32(w)))), int(max_history))


def model_luminance(m):
    return (54 * m[0] + 183 * m[1] + 19 * m[2] + 128) >> 8


def model_variance_integer(K, s2):
    """V: the float32 product (float)K * s2 as an integer; below 2^23 rounded to nearest even, an integer already above."""
    with np.errstate(over="raise"):
        f = F32(F32(K) * F32(s2))
    return round_half_even(Fraction(float(f)))


def model_finish(h, w, s2, splat, params, reproject):
    """(film row, moment row) as lists of four Python integers; s2 None: no tap carried a variance."""
    K = model_history_count(w, reproject.maxHistory)
    if K == 0:
        return [0, 0, 0, 0], [0, 0, 0, 0]
    m = [model_fixed_mean(F32(c), params) for c in h]
    film = [(v * K) & MASK for v in m] + [K << 16 if splat else K]
    y = model_luminance(m)
    if s2 is None:
        return film, [y, (y * y) & LO_MASK, (y * y) >> 40, 1]
    Q = K * y * y + model_variance_integer(K, s2)
    return film, [y * K, Q & LO_MASK, Q >> 40, K]


def model_row_variance(row):
    """The population variance of a moment row's luminance as a Fraction (N >= 1): (N Q - Sy^2) / N^2."""
    Sy, lo, hi, N = (int(v) for v in row)
    return Fraction(model_D(Sy, lo, hi, N), N * N)


def model_row_standard_error(row):
    """sqrt(variance / N) of a moment row in float64."""
    return float(np.sqrt(float(model_row_variance(row)) / int(row[3])))


def f32_fma(a, b, c):
    """fma(a, b, c) of three float32 as a float32: the exact a b + c in rationals, rounded once to nearest, ties to even."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return F32(0.0)
    mag = abs(x)
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1                                   # 2^e <= mag < 2^(e + 1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = round_half_even(mag / quantum)
    return F32(float(n * quantum) * (-1 if x < 0 else 1))   # (n quantum has at most 24 significant bits: exact as a float)


# ---- cameras and their centre rays --------------------------------------------------------------------------------------------------------------
def centre_rays(film):
    """(origins (P, 3), unit directions (P, 3)) of a film camera's centre rays as float64: ptss_generate_rays with jitter = 0 on the host."""
    c = ptss.film_camera(film.kind, film.width, film.height, film.camera, film.lensRadius, film.focusDistance, jitter=0)
    P = film.width * film.height
    rays = np.ascontiguousarray(ptss.probe_film_rays(c, np.zeros((P, 6), np.uint32))[0]).view(np.float32).reshape(-1, 8)
    return rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)


def quat_rotate(q, v):
    u = np.asarray(q[:3], dtype=np.float64)
    uv = np.cross(u, v)
    return v + 2.0 * (q[3] * uv + np.cross(u, uv))


def near(value, threshold, scale=None):
    scale = np.abs(threshold) if scale is None else scale
    return np.abs(value - threshold) <= NEAR_TIE * scale


# ---- steps 1 to 4 in float64 --------------------------------------------------------------------------------------------------------------------
def model_lookup(now, f_now, prev, f_prev, film_prev, moments_prev, params, reproject, motion_now=None):
    """-> dict of per-pixel arrays: status, h (P, 3), w, K, s2 (NaN: none), tie (a threshold within NEAR_TIE: leave the pixel out)."""
    Wn, Hn, W, H = now.width, now.height, prev.width, prev.height
    P = Wn * Hn
    o, d = centre_rays(now)
    m = f_now["materialIdx"].astype(np.int64)
    hit = m >= 0
    pc = prev.camera
    o_prev = np.array([pc.position.x, pc.position.y, pc.position.z], dtype=np.float64)
    conj = np.array([-pc.rotation.x, -pc.rotation.y, -pc.rotation.z, pc.rotation.w], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        point = o + d * f_now["depth"].astype(np.float64)[:, None] if motion_now is None else motion_now["prevPoint"].astype(np.float64)
        v = np.where(hit[:, None], point - o_prev, d)
    rng_ = np.linalg.norm(v, axis=1)
    l = quat_rotate(conj, v)
    tie = np.zeros(P, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        if prev.kind == ptss.FILM_EQUIRECT:
            front = np.isfinite(l).all(axis=1) & (l != 0).any(axis=1)
            lon, lat = np.arctan2(l[:, 0], -l[:, 2]), np.arctan2(l[:, 1], np.hypot(l[:, 0], l[:, 2]))
            fx, fy = (lon / (2 * np.pi) + 0.5) * W - 0.5, (lat / np.pi + 0.5) * H - 0.5
            tie |= near(np.abs(lon), np.pi)   # the seam itself: lon may come out at either end
        else:
            s = -2.0 * np.tan(float(pc.fieldOfView) / 2.0)
            front = l[:, 2] * float(pc.zNear) > 0
            tie |= near(l[:, 2], 0.0, np.linalg.norm(l, axis=1))
            fx = (l[:, 0] / (l[:, 2] * s) + 0.5) * W - 0.5
            fy = (l[:, 1] / (l[:, 2] * s * (H / W)) + 0.5) * H - 0.5
    inside = front & (fx >= -1) & (fx < W) & (fy >= -1) & (fy < H)
    tie |= front & (near(fx, -1.0) | near(fx, float(W)) | near(fy, -1.0) | near(fy, float(H)))
    fx, fy = np.where(inside, fx, 0.0), np.where(inside, fy, 0.0)
    x0, y0 = np.floor(fx), np.floor(fy)
    tie |= inside & (near(fx, np.rint(fx), np.maximum(1.0, np.abs(np.rint(fx)))) | near(fy, np.rint(fy), np.maximum(1.0, np.abs(np.rint(fy)))))
    tx, ty = fx - x0, fy - y0
    # the previous film as float64 rows
    splat = is_splat(film_prev)
    means = model_means(film_prev)
    usable = np.array([mm is not None for mm in means])
    down = 2.0 ** -params.scaleLog2
    colour = np.array([[float(F32(c)) * down for c in mm] if mm is not None else [0.0, 0.0, 0.0] for mm in means])
    count = np.array([float(F32(model_counts(int(e[3]), splat)[0])) if ok else 0.0 for e, ok in zip(words(film_prev), usable)])
    variance = np.full(W * H, np.nan)
    if moments_prev is not None:
        for q, row in enumerate(words(moments_prev)):
            if int(row[3]) >= 2:
                variance[q] = float(model_row_variance(row))
    mp, np_, zp = f_prev["materialIdx"].astype(np.int64), f_prev["normal"].astype(np.float64), f_prev["depth"].astype(np.float64)
    normal = f_now["normal"].astype(np.float64)
    B, csum, nsum = np.zeros(P), np.zeros((P, 3)), np.zeros(P)
    SB, ssum = np.zeros(P), np.zeros(P)
    lo, hi = np.full((P, 3), np.inf), np.full((P, 3), -np.inf)
    slo, shi = np.full(P, np.inf), np.full(P, -np.inf)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = (x0 + i).astype(np.int64), (y0 + j).astype(np.int64)
            if prev.kind == ptss.FILM_EQUIRECT:
                qx = np.where(qx < 0, qx + W, np.where(qx >= W, qx - W, qx))
            b = np.where(i, tx, 1 - tx) * np.where(j, ty, 1 - ty)
            ok = inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (b > 0)
            qi = np.where(ok, qy * W + qx, 0)
            ok &= mp[qi] == m
            with np.errstate(invalid="ignore"):
                cos = (normal * np_[qi]).sum(axis=1)
                off = np.abs(zp[qi] - rng_)
                tol = float(reproject.depthTolerance) * rng_
                tie |= ok & hit & (near(cos, float(reproject.cosNormal)) | near(off, tol))
                same = ~hit | ((cos >= float(reproject.cosNormal)) & (off <= tol))
            ok &= same & usable[qi]
            B += np.where(ok, b, 0.0)
            csum += np.where(ok[:, None], b[:, None] * colour[qi], 0.0)
            nsum += np.where(ok, b * count[qi], 0.0)
            lo = np.where(ok[:, None], np.minimum(lo, colour[qi]), lo)
            hi = np.where(ok[:, None], np.maximum(hi, colour[qi]), hi)
            carries = ok & ~np.isnan(variance[qi])
            vq = np.where(carries, variance[qi], 0.0)
            SB += np.where(carries, b, 0.0)
            ssum += b * vq
            slo = np.where(carries, np.minimum(slo, vq), slo)
            shi = np.where(carries, np.maximum(shi, vq), shi)
    have = B > 0
    safe = np.where(have, B, 1.0)
    h = np.clip(csum / safe[:, None], np.where(have[:, None], lo, 0.0), np.where(have[:, None], hi, 0.0))
    w = nsum / safe
    tie |= have & near(B, float(reproject.minCoverage))
    covered = have & (B >= float(reproject.minCoverage))
    cap = float(reproject.maxHistory)
    tie |= covered & (w < cap + 1) & (np.abs(w - np.floor(w) - 0.5) <= NEAR_TIE)
    K = np.minimum(np.rint(w), cap)
    seeded = covered & (K >= 1)
    s2 = np.where(SB > 0, np.clip(ssum / np.where(SB > 0, SB, 1.0), np.where(SB > 0, slo, 0.0), np.where(SB > 0, shi, 0.0)), np.nan)
    status = np.where(seeded, SEEDED, np.where(inside, NO_TAP, OFF_FILM))
    return dict(status=status, h=h, w=w, K=np.where(seeded, K, 0).astype(np.int64), s2=np.where(seeded, s2, np.nan), tie=tie)


def film_means(film):
    """(P, 3) int64 integer means of a film (0 where empty) and its (P,) K (0 where empty)."""
    splat = is_splat(film)
    ms = model_means(film)
    m = np.array([mm if mm is not None else (0, 0, 0) for mm in ms], dtype=np.int64)
    K = np.array([(int(e[3]) >> 16 if splat else int(e[3]) & 0xffffffff) if mm is not None else 0 for e, mm in zip(words(film), ms)], dtype=np.int64)
    return m, K


def compare_with_model(got_film, got_moments, model, params):
    """Host (or device) rows against model_lookup's pixels that are not near ties -> (share left out, largest |m' - model| in fixed-point
    steps, number of K that differ, largest relative difference of the rows' standard errors, number of statuses that differ)."""
    keep = ~model["tie"]
    m, K = film_means(got_film)
    seeded = model["status"] == SEEDED
    status_bad = int((keep & ((K > 0) != seeded)).sum())
    both = keep & seeded & (K > 0)
    want = np.clip(model["h"], 0.0, float(F32(params.clampMax))) * 2.0 ** params.scaleLog2
    step = float(np.abs(m[both] - want[both]).max()) if both.any() else 0.0
    k_bad = int((K[both] != model["K"][both]).sum())
    rel = 0.0
    if got_moments is not None:
        rows = words(got_moments)
        for p in np.nonzero(both & ~np.isnan(model["s2"]) & (K == model["K"]))[0]:
            want_se = np.sqrt(model["s2"][p] / K[p])
            got_se = model_row_standard_error(rows[p])
            if want_se > 0:
                rel = max(rel, abs(got_se - want_se) / want_se)
    return 1.0 - keep.mean(), step, k_bad, rel, status_bad
