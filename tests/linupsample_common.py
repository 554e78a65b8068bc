"""The model and the cases shared by tests/test_linupsample_cpu.py and tests/test_gpu_linupsample.py (ptss_upsample_linear; DESIGN.md
§3.36). The model restates the call in Python integers (means, counts, tap geometry, anchor, the exact path, ptlin::toFixed) and numpy
float32 scalars (weights, sums, hull), with fma rounded once from rationals and ptm::exp taken through ptss_probe_math; it shares no code
with csrc/ptlinup.h and must agree with the probe byte for byte."""
from fractions import Fraction

import numpy as np

import ptss
from adaptive_common import f32_of_int
from lindenoise_common import model_counts, model_fixed_mean, model_weight_word
from linear_common import MASK, params_of
from linreproject_common import f32_fma
from meter_common import host_exp as ptm_exp, model_mean_linear, model_mean_splat

F32 = np.float32
INF = F32(np.inf)
FACTORS = (1, 2, 3, 4)
# the kernel's tile of hi pixels: the GPU sizes below are chosen around it
TILE_X, TILE_Y = 32, 8


def words(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4)


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def first_difference(a, b):
    a, b = words(a), words(b)
    bad = np.nonzero((a != b).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist(), len(bad))


def is_splat(film):
    return np.asarray(film).dtype == ptss.SPLAT_DTYPE


# ---- float32 steps ---------------------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """fma of float32 scalars, rounded once; operands that are not finite go through float64, whose NaN and infinities are the same."""
    a, b, c = F32(a), F32(b), F32(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(invalid="ignore", over="ignore"):
            return F32(np.float64(a) * np.float64(b) + np.float64(c))
    return f32_fma(a, b, c)


def pmin(a, b):   # ptm::min: (b < a) ? b : a
    return b if b < a else a


def pmax(a, b):   # ptm::max: (a < b) ? b : a
    return b if a < b else a


def dot(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return fma(a[2], b[2], fma(a[1], b[1], F32(a[0]) * F32(b[0])))


def model_slope(z, has_a, za, has_b, zb):
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(F32(z) - F32(za)) if has_a else INF
        b = np.abs(F32(zb) - F32(z)) if has_b else INF
    g = pmin(a, b)
    return g if g < INF else F32(0.0)


def model_axis(X, f):
    r = X % f
    k = (2 * r + 1 + f) % (2 * f)
    x0 = X // f - (1 if 2 * r + 1 < f else 0)
    return x0, k, F32(k) / F32(2 * f)


def model_lo(film):
    """Per lo pixel None (empty) or ((m_r, m_g, m_b), K)."""
    splat = is_splat(film)
    mean = model_mean_splat if splat else model_mean_linear
    out = []
    for r, g, b, w3 in ([int(v) for v in e] for e in words(film)):
        w = model_weight_word(w3, splat)
        out.append(None if w == 0 else ((mean(r, w), mean(g, w), mean(b, w)), model_counts(w3, splat)[0]))
    return out


def model_upsample(film, width, height, features_lo, features_hi, params, up):
    """(the large film as (f^2 W H, 4) uint64 rows, [filtered, fallback, empty], per hi pixel the list of counted lo pixel indices)."""
    f, wrap = int(up.factor), bool(up.flags & ptss.UPSAMPLE_LINEAR_WRAP_X)
    hiW, hiH = width * f, height * f
    lo = model_lo(film)
    flo = np.ascontiguousarray(features_lo).view(ptss.FEATURE_DTYPE).reshape(-1)
    fhi = np.ascontiguousarray(features_hi).view(ptss.FEATURE_DTYPE).reshape(-1)
    down = F32(2.0 ** -params.scaleLog2)
    inv_normal = F32(1.0) / F32(up.sigmaNormal)
    sigma_depth = F32(up.sigmaDepth)
    zero, one, half = F32(0.0), F32(1.0), F32(0.5)
    out = np.zeros((hiW * hiH, 4), dtype=np.uint64)
    info = [0, 0, 0]
    counted_of = []
    for Y in range(hiH):
        y0, ky, fy = model_axis(Y, f)
        for X in range(hiW):
            x0, kx, fx = model_axis(X, f)
            P = Y * hiW + X
            F = fhi[P]
            mat, zp, hit = int(F["materialIdx"]), F32(F["depth"]), int(F["materialIdx"]) >= 0
            gx = gy = zero
            if hit:
                l, r, d, u = wrap or X > 0, wrap or X + 1 < hiW, Y > 0, Y + 1 < hiH
                Xl, Xr = (X - 1) % hiW, (X + 1) % hiW
                gx = model_slope(zp, l, fhi[Y * hiW + Xl]["depth"] if l else 0, r, fhi[Y * hiW + Xr]["depth"] if r else 0)
                gy = model_slope(zp, d, fhi[(Y - 1) * hiW + X]["depth"] if d else 0, u, fhi[(Y + 1) * hiW + X]["depth"] if u else 0)
            taps = []   # (b, w, q) of the counted taps, in tap order
            for t in range(4):
                i, j = t & 1, t >> 1
                qx, qy = x0 + i, y0 + j
                if wrap:
                    qx = qx + width if qx < 0 else (qx - width if qx >= width else qx)
                if not (0 <= qx < width and 0 <= qy < height):
                    continue
                q = qy * width + qx
                if lo[q] is None or int(flo[q]["materialIdx"]) != mat:
                    continue
                b = (fx if i else one - fx) * (fy if j else one - fy)
                e = zero
                if hit:
                    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                        ax = F32((2 * f - kx) if i else kx) * half
                        ay = F32((2 * f - ky) if j else ky) * half
                        e = e + pmax(zero, one - dot(F["normal"], flo[q]["normal"])) * inv_normal
                        tol = pmax(fma(sigma_depth, fma(gx, ax, gy * ay), F32(1e-3) * zp), F32(1e-30))
                        e = e + np.abs(zp - F32(flo[q]["depth"])) / tol
                with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                    w = b * ptm_exp(-e)
                if w > 0:
                    taps.append((b, w, q))
            counted_of.append([q for _, _, q in taps])
            if not taps:
                n = lo[(Y // f) * width + X // f]
                if n is None:
                    info[2] += 1
                else:
                    info[1] += 1
                    out[P] = [(m * n[1]) & MASK for m in n[0]] + [n[1]]
                continue
            info[0] += 1
            anchor = max(range(len(taps)), key=lambda k: (taps[k][0], -k))   # the largest b, the lower index on a tie
            ma, Ka = lo[taps[anchor][2]]
            colour = lambda q: [f32_of_int(m) * down for m in lo[q][0]]
            ca = colour(taps[anchor][2])
            row = []
            for ch in range(3):
                cs = [colour(q)[ch] for _, _, q in taps]
                if all(lo[q][0][ch] == ma[ch] for _, _, q in taps):
                    row.append(ma[ch])
                    continue
                s, ws = zero, zero
                for (b, w, q), c in zip(taps, cs):
                    s = fma(c - ca[ch], w, s)
                    ws = ws + w
                with np.errstate(over="ignore"):
                    v = ca[ch] + s / ws
                v = pmin(pmax(v, min(cs)), max(cs))
                row.append(model_fixed_mean(v, params))
            out[P] = [(m * Ka) & MASK for m in row] + [Ka]
    return out, info, counted_of


# ---- features of both sizes and films -------------------------------------------------------------------------------------------------------
def features_of(width, height, seed=0, misses=True, bad=False):
    """The features of one analytic scene at any size: two surfaces meeting at a slanted edge (material, normal and depth all change
    across it), a thin stripe of a third material narrower than a lo pixel, and, with `misses`, a patch of misses. Functions of the
    pixel centre in [0, 1]^2, so the lo and the hi features of a film describe the same picture. bad: a few NaN normals and depths and
    a depth of 1e30."""
    ys, xs = np.divmod(np.arange(width * height), width)
    u, v = (xs + 0.5) / width, (ys + 0.5) / height
    f = np.zeros(width * height, dtype=ptss.FEATURE_DTYPE)
    right = 3 * u + v > 2.0
    f["normal"][~right] = (0.0, 0.0, 1.0)
    f["normal"][right] = (0.6, 0.0, 0.8)
    f["depth"] = np.where(right, 9.0 - 3.0 * u + 1.0 * v, 4.0 + 5.0 * u + 2.0 * v).astype(F32)
    f["materialIdx"] = np.where(right, 1, 0)
    stripe = np.abs(u - v * 0.3 - 0.2) < 0.02
    f["materialIdx"][stripe] = 2
    f["albedo"] = 0.5
    if misses:
        gone = (v < 0.25) & (u > 0.7)
        f["normal"][gone] = 0.0
        f["depth"][gone] = np.inf
        f["materialIdx"][gone] = -1
    if bad and width * height >= 8:
        g = np.random.default_rng(977 + seed + width)
        pick = g.choice(width * height, size=max(3, width * height // 16), replace=False)
        f["depth"][pick[0::3]] = np.nan
        f["normal"][pick[1::3], 1] = np.nan
        f["depth"][pick[2::3]] = 1e30
    return f


def film_of(width, height, params, seed=0, splat=False, holes=True, big=False):
    """A film over features_of's picture: 1 .. 9 samples a pixel, sums that do not divide evenly, a luminance step at the edge, noise;
    holes: about a seventh of the pixels empty, a whole corner block among them; big: some means at and just below 2^40 (with
    params_of(20, 2^20): clampMax * 2^scaleLog2 = 2^40)."""
    g = np.random.default_rng(31 * width + 7 * height + seed + (1000 if splat else 0))
    P = width * height
    feat = features_of(width, height, seed)
    base = {0: (0.9, 0.6, 0.3), 1: (0.2, 0.3, 0.5), 2: (1.5, 1.4, 0.1), -1: (0.05, 0.05, 0.08)}
    one = 1 << params.scaleLog2
    film = np.zeros(P, dtype=ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE)
    N = g.integers(1, 10, P)
    if holes:
        N[g.random(P) < 0.14] = 0
        ys, xs = np.divmod(np.arange(P), width)
        N[(xs < max(1, width // 4)) & (ys >= height - max(1, height // 3))] = 0
    for p in range(P):
        n = int(N[p])
        if n == 0:
            continue
        m = [max(0, int(c * one * (1.0 + 0.2 * g.standard_normal()))) for c in base[int(feat["materialIdx"][p])]]
        jitter = int(g.integers(-3000, 3000))
        if big and p % 5 == 0:
            m = [(1 << 40) - int(k) for k in g.integers(0, 3, 3)]
            jitter = 0   # a weight of whole samples: the sums below hold these means exactly
        if splat:
            Wt = (n << 16) + jitter
            sums = [(c * Wt) >> 16 for c in m]
            film[p] = (sums[0], sums[1], sums[2], Wt)
        else:
            sums = [c * n + int(g.integers(0, n)) - n // 2 if c > n else c * n for c in m]
            film[p] = (sums[0], sums[1], sums[2], n, int(g.integers(0, 2)))
    return film


def case(width, height, factor, params, seed=0, splat=False, wrap=False, bad=False, big=False, holes=True):
    """(film_lo, features_lo, features_hi, an upsample_linear_params) of one synthetic case."""
    up = ptss.upsample_linear_params(factor, 0.1, 4.0, wrap_x=wrap)
    hi = features_of(width * factor, height * factor, seed, True, bad)
    hi["materialIdx"][5::13] = 7   # surfaces the small film did not see: no tap counts there, at factor 1 too
    return film_of(width, height, params, seed, splat, holes, big), features_of(width, height, seed, True, bad), hi, up


def wrapped_sums_film(P, splat, seed=0):
    """Entries no film holds: random 64-bit words, so sums wrap in the means' additions."""
    g = np.random.default_rng(4242 + seed)
    w = g.integers(0, 1 << 63, (P, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, (P, 4), dtype=np.uint64)
    if splat:
        w[:, 3] >>= np.uint64(20)   # weights below 2^44: the split of the wide division keeps to its words either way
    w[::7, 3] = 0
    return w.view(ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE).reshape(-1)


def integer_means(film, splat=None):
    """What every consumer takes of a film: per pixel None (empty) or the three integer means."""
    return [None if e is None else e[0] for e in model_lo(film)]


# ---- the refusal lists (defined against the probe by the CPU test; the GPU test imports them) ----------------------------------------------
UP_REFUSED = [dict(structSize=20), dict(structSize=0), dict(factor=0), dict(factor=5), dict(factor=-1), dict(sigmaNormal=0.0),
              dict(sigmaNormal=-1.0), dict(sigmaNormal=float("inf")), dict(sigmaNormal=float("nan")), dict(sigmaDepth=0.0),
              dict(sigmaDepth=float("inf")), dict(sigmaDepth=float("nan")), dict(flags=2), dict(flags=0x80000001), dict(reserved=1)]
FILM_REFUSED = [dict(structSize=16), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=float("inf")),
                dict(scaleLog2=32, clampMax=257.0), dict(exposure=-0.5), dict(exposure=float("nan")), dict(reserved=1)]
# (width, height, factor) the call refuses with PTSS_ERANGE
BAD_SIDES = ((0, 4, 2), (4, 0, 2), (-1, 4, 1), (2 ** 22 + 1, 1, 1), (1, 2 ** 22 + 1, 1), (2 ** 21 + 1, 1, 2), (1, 2 ** 20 + 1, 4), (2 ** 22, 512, 1),
             (46341, 46341, 1), (2 ** 15, 2 ** 14, 2), (11586, 11586, 4))


def changed(make, **kw):
    p = make()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


DEFAULT_PARAMS = params_of(20, 65536.0)
COARSE_PARAMS = params_of(6, 64.0)
BIG_PARAMS = params_of(20, float(2 ** 20))   # clampMax * 2^scaleLog2 = 2^40
