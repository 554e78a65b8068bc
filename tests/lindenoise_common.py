"""Models and cases shared by tests/test_lindenoise_cpu.py and tests/test_gpu_lindenoise.py (ptss_denoise_linear):
prepare and finish in Python integers and numpy float32, one pass of the filter as a float64 restatement of the formulas — both
independent of csrc/ptlindn.h — and the films, moments and features the filter is tried on."""
from fractions import Fraction

import numpy as np

import ptss
from adaptive_common import f32_of_int
from linear_common import MASK, linear_film
from linstats_common import model_D, model_sqrt128, moments_of_rows, row_of_ys
from meter_common import model_mean_linear, model_mean_splat
from splat_common import splat_film

F32 = np.float32
H_SPLINE = {0: 0.375, 1: 0.25, 2: 0.0625}
LUMA = (54.0 / 256.0, 183.0 / 256.0, 19.0 / 256.0)
EXP_FLUSH = 87.33654475055310   # ptm::exp returns 0 below -this
MIN_SQUARE = 2.0 ** -149        # the smallest float32 above 0: a squared weight below half of it is 0


def words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4)


def is_splat(film):
    return np.asarray(film).dtype == ptss.SPLAT_DTYPE


# ---- prepare and finish, exactly ----------------------------------------------------------------------------------------------------------------
def model_weight_word(word3, splat):
    return word3 if splat else word3 & 0xffffffff


def model_means(film):
    """Per pixel None (empty) or the three integer means."""
    splat = is_splat(film)
    mean = model_mean_splat if splat else model_mean_linear
    out = []
    for r, g, b, w3 in ([int(v) for v in e] for e in words(film)):
        w = model_weight_word(w3, splat)
        out.append(None if w == 0 else (mean(r, w), mean(g, w), mean(b, w)))
    return out


def model_colour(m, scale_log2):
    """c = (float)m * 2^-scaleLog2 in float32."""
    return f32_of_int(m) * F32(2.0 ** -scale_log2)


def model_variance(Sy, sqLo, sqHi, N, scale_log2):
    """v of prepare in float32 steps: (se * 2^-scaleLog2)^2, +inf for N < 2."""
    if N < 2:
        return F32(np.inf)
    with np.errstate(over="ignore"):
        r = model_sqrt128(model_D(Sy, sqLo, sqHi, N))
        fn = f32_of_int(N)
        se = F32(r / F32(fn * np.sqrt(fn))) * F32(2.0 ** -scale_log2)
        return F32(se * se)


def model_prepare(film, moments, params):
    """(P, 4) float32 rows {c, v}; an empty pixel's is {0, 0, 0, -1}."""
    out = np.zeros((len(film), 4), F32)
    for p, (m, mo) in enumerate(zip(model_means(film), words(moments))):
        if m is None:
            out[p, 3] = ptss.DENOISE_LINEAR_EMPTY
            continue
        out[p, :3] = [model_colour(c, params.scaleLog2) for c in m]
        out[p, 3] = model_variance(*(int(v) for v in mo), params.scaleLog2)
    return out


def model_counts(word3, splat):
    """(K, clamped) of an output row."""
    if splat:
        return max(1, min(((word3 + 32768) & MASK) >> 16, (1 << 23) - 1)), 0
    return word3 & 0xffffffff, word3 >> 32


def round_half_even(x):
    """A Fraction or float (exactly representable) to the nearest integer, ties to even."""
    x = Fraction(x)
    k = x.numerator // x.denominator
    rest = x - k
    return k + 1 if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1) else k


def model_fixed_mean(c, params):
    """m' of one channel: clamp to [0, clampMax], scale, round to nearest even (c: a float32 or float64 value)."""
    c = float(c)
    c = 0.0 if not c > 0.0 else min(c, float(F32(params.clampMax)))
    return round_half_even(Fraction(c) * (1 << params.scaleLog2))


def model_entry(m, word3, splat):
    """The output row of a non-empty pixel with integer means m."""
    K, clamped = model_counts(word3, splat)
    return [(v * K) & MASK for v in m] + [K | (clamped << 32)]


def model_finish_means(film):
    """The output film of levels = 0 as (P, 4) uint64 rows."""
    splat = is_splat(film)
    rows = []
    for m, e in zip(model_means(film), words(film)):
        rows.append([0, 0, 0, 0] if m is None else model_entry(m, int(e[3]), splat))
    return np.array(rows, dtype=np.uint64).reshape(-1, 4)


# ---- one pass, float64 ----------------------------------------------------------------------------------------------------------------------------
def feature_planes(features, width, height):
    f = np.ascontiguousarray(features).view(ptss.FEATURE_DTYPE).reshape(height, width)
    return f["normal"].astype(np.float64), f["depth"].astype(np.float64), f["materialIdx"].astype(np.int64)


def shifted(a, dx, dy, fill):
    """a[y + dy, x + dx] where inside the frame, `fill` elsewhere, and the mask of inside."""
    h, w = a.shape[:2]
    out = np.full(a.shape, fill, dtype=a.dtype)
    inside = np.zeros((h, w), bool)
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
        inside[yd, xd] = True
    return out, inside


def model_slopes(depth):
    with np.errstate(invalid="ignore"):
        out = []
        for dx, dy in ((1, 0), (0, 1)):
            a, ia = shifted(depth, -dx, -dy, 0.0)
            b, ib = shifted(depth, dx, dy, 0.0)
            da = np.where(ia, np.abs(depth - a), np.inf)
            db = np.where(ib, np.abs(b - depth), np.inf)
            g = np.fmin(da, db)   # a NaN (inf - inf) loses against a number, as an ordered compare makes it
            g = np.where(np.isnan(g), np.inf, g)
            out.append(np.where(g < np.inf, g, 0.0))
    return out


def model_pass(plane, features, width, height, step, params, denoise):
    """One pass over a (P, 4) plane {c, v} (float32 or float64 rows) in float64 -> the (P, 4) float64 plane afterwards."""
    pl = np.asarray(plane, dtype=np.float64).reshape(height, width, 4)
    c, v = pl[..., :3], pl[..., 3]
    empty = v < 0
    normal, depth, mat = feature_planes(features, width, height)
    gx, gy = model_slopes(depth)
    hit = mat >= 0
    lum = c @ np.array(LUMA)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        acc, used = np.zeros((height, width)), np.zeros((height, width))
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                vq, inside = shifted(v, i, j, -1.0)
                ok = inside & (vq >= 0)
                k = (2 if i == 0 else 1) * (2 if j == 0 else 1)
                acc += np.where(ok, k * np.where(ok, vq, 0.0), 0.0)
                used += np.where(ok, k, 0)
        V = acc / np.where(used > 0, used, 1)
        tol = np.maximum(float(denoise.sigmaLuminance) * np.sqrt(V), 2.0 ** -params.scaleLog2)
        wp = H_SPLINE[0] ** 2
        total = np.zeros((height, width, 3))
        wsum = np.full((height, width), wp)
        vsum = wp * wp * v
        lo, hi = c.copy(), c.copy()
        for j in range(-2, 3):
            for i in range(-2, 3):
                if i == 0 and j == 0:
                    continue
                cq, inside = shifted(c, i * step, j * step, 0.0)
                vq, _ = shifted(v, i * step, j * step, -1.0)
                mq, _ = shifted(mat, i * step, j * step, -7)
                nq, _ = shifted(normal, i * step, j * step, 0.0)
                zq, _ = shifted(depth, i * step, j * step, 0.0)
                ok = inside & (mq == mat) & (vq >= 0)
                e = np.abs(cq @ np.array(LUMA) - lum) / tol
                ztol = np.maximum(float(denoise.sigmaDepth) * (gx * abs(i * step) + gy * abs(j * step)) + 1e-3 * depth, 1e-30)
                geo = np.maximum(0.0, 1.0 - (normal * nq).sum(axis=2)) / float(denoise.sigmaNormal) + np.abs(depth - zq) / ztol
                e = e + np.where(hit, geo, 0.0)
                w = H_SPLINE[abs(i)] * H_SPLINE[abs(j)] * np.exp(-e)
                w = np.where(ok & (e <= EXP_FLUSH) & (w > 0), w, 0.0)
                w = np.where(np.isnan(w), 0.0, w)
                use = w > 0
                total += np.where(use[..., None], w[..., None] * (cq - c), 0.0)
                wsum += w
                lo = np.where(use[..., None], np.minimum(lo, cq), lo)
                hi = np.where(use[..., None], np.maximum(hi, cq), hi)
                w2 = w * w
                vsum = vsum + np.where(use & (w2 > MIN_SQUARE / 2), w2 * np.where(use, vq, 0.0), 0.0)
        out = np.clip(c + total / wsum[..., None], lo, hi)
        vout = vsum / (wsum * wsum)
    res = np.concatenate([out, vout[..., None]], axis=2)
    res[empty] = (0.0, 0.0, 0.0, ptss.DENOISE_LINEAR_EMPTY)
    return res.reshape(-1, 4)


def model_run(film, moments, features, width, height, params, denoise):
    """The planes of a whole call in float64, passes applied to the float32 plane of prepare: the plane after the last pass."""
    plane = model_prepare(film, moments, params).astype(np.float64)
    for i in range(denoise.levels):
        plane = model_pass(plane, features, width, height, 1 << i, params, denoise)
    return plane


# ---- films, moments and features ---------------------------------------------------------------------------------------------------------------
def scene_features(width, height, seed=0, misses=True):
    """Two surfaces meeting at a slanted edge — material, normal and depth all change across it — and, with `misses`, a patch of misses."""
    g = np.random.default_rng(seed)
    f = np.zeros(width * height, dtype=ptss.FEATURE_DTYPE)
    ys, xs = np.divmod(np.arange(width * height), width)
    right = xs * 3 + ys > (3 * width + height) // 2
    f["normal"][~right] = (0.0, 0.0, 1.0)
    f["normal"][right] = (0.6, 0.0, 0.8)
    f["depth"] = np.where(right, 9.0 - 0.03 * xs + 0.01 * ys, 4.0 + 0.05 * xs + 0.02 * ys).astype(F32)
    f["materialIdx"] = np.where(right, 1, 0)
    f["albedo"] = g.uniform(0, 1, (width * height, 3)).astype(F32)
    if misses and width * height > 6:
        gone = (ys < max(1, height // 5)) & (xs >= width - max(1, width // 4))
        f["normal"][gone] = 0.0
        f["depth"][gone] = np.inf
        f["materialIdx"][gone] = -1
    return f


def truth_of(features, width, height):
    """The noise-free radiance of scene_features' two surfaces (and of its misses): a luminance step at the edge."""
    mat = np.ascontiguousarray(features)["materialIdx"]
    base = {0: (0.9, 0.6, 0.3), 1: (0.2, 0.3, 0.5), -1: (0.05, 0.05, 0.08)}
    return np.array([base[int(m)] for m in mat], dtype=np.float64)


def sampled_film(truth, samples, params, seed=0, noise=0.25, splat=False):
    """A film and its consistent moments: pixel p holds samples[p] draws of truth[p] * (1 + noise * N(0, 1)) per channel, clamped at 0,
    accumulated as the library accumulates them (fixed point per sample, its luminance and square into the moment row). A splat film
    holds the same sums with a weight of 65536 per sample (a box filter's)."""
    g = np.random.default_rng(seed)
    P = len(truth)
    film = splat_film(P) if splat else linear_film(P)
    rows = []
    one = 1 << params.scaleLog2
    for p in range(P):
        N = int(samples[p])
        draws = np.maximum(truth[p] * (1.0 + noise * g.standard_normal((N, 3))), 0.0)
        q = np.rint(draws * one).astype(np.int64)
        ys = [(54 * int(a) + 183 * int(b) + 19 * int(c) + 128) >> 8 for a, b, c in q]
        rows.append(row_of_ys(ys))
        sums = [int(v) for v in q.sum(axis=0)] if N else [0, 0, 0]
        if splat:
            film[p] = (sums[0], sums[1], sums[2], N << 16)   # S = sum (q * 65536) >> 16: the box filter's taps
        else:
            film[p] = (sums[0], sums[1], sums[2], N, 0)
    return film, moments_of_rows(rows)


def corner_holes(width, height):
    """Pixels at the corners of the 32 x 8 tiles (and of the frame): where a staged tile, its halo and the frame's border meet."""
    out = set()
    for y in (0, 7, 8, 15, 16, height - 1):
        for x in (0, 31, 32, 63, 64, width - 1):
            if 0 <= x < width and 0 <= y < height:
                out.add(y * width + x)
    return sorted(out)


def case(width, height, params, seed=0, splat=False, holes=True, single=True, misses=True, noise=0.25):
    """(film, moments, features) over scene_features: 2 .. 9 samples a pixel, empty pixels at the tile corners, some pixels of one sample."""
    g = np.random.default_rng(7000 * width + 10 * height + seed)
    P = width * height
    features = scene_features(width, height, seed, misses)
    samples = g.integers(2, 10, P)
    if single:
        samples[g.integers(0, P, max(1, P // 9))] = 1
    if holes and P >= 16:
        samples[corner_holes(width, height)] = 0
    film, moments = sampled_film(truth_of(features, width, height), samples, params, seed, noise, splat)
    return film, moments, features


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def first_difference(a, b):
    a, b = words(a), words(b)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist(), len(bad))
