"""Models and cases shared by tests/test_glare_cpu.py and tests/test_gpu_glare.py (ptss_glare_build, ptss_resolve_linear_glare /
ptss_resolve_splat_glare): the source, the downs, the ups and the mixed mean in Python integers (wrapping at 2^64 where the
header's unsigned words would) — independent of csrc/ptglare.h — and the resolve's float steps in numpy float32 with the tone map taken
from the oracle and ptm::pow through ptss_probe_math, as linear_common.model_resolve takes them."""
from fractions import Fraction

import numpy as np

import oracle
import ptss
from adaptive_common import f32_of_int
from linear_common import GAMMA, MASK, host_pow
from linear_common import high_film as high_linear_film
from linear_common import linear_film, params_of
from linear_common import resolve_rows as linear_resolve_rows
from meter_common import largest_linear_rows, largest_splat_rows, model_mean_linear, model_mean_splat
from splat_common import high_film as high_splat_film
from splat_common import resolve_rows as splat_resolve_rows
from splat_common import splat_film

F32 = np.float32
SIZES = ((1, 1), (2, 1), (1, 5), (3, 3), (37, 21), (64, 48), (65, 34))   # 65 x 34: level 1 is 33 x 17, past one 16-texel tile in both axes
LEVELS = tuple(range(1, 9))
STRENGTHS = (0.0, 2.0 ** -16, 0.1, 1.0)
MODES = ("add", "mix")
TOP = 1 << 40   # the largest mean of a film the library filled


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def film_rows(film):
    return [[int(v) for v in e] for e in np.ascontiguousarray(film).view(np.uint64).reshape(-1, 4)]


def is_splat(film):
    return np.asarray(film).dtype == ptss.SPLAT_DTYPE


def model_threshold(threshold, params):
    """The threshold in the film's fixed point: the exact product rounded to the nearest integer, ties to even; not clamped."""
    s = Fraction(float(F32(threshold))) * (1 << params.scaleLog2)
    k = s.numerator // s.denominator
    rest = s - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1):
        k += 1
    return k


def model_means(film):
    """Per pixel (mr, mg, mb, w): the integer means of the resolve (0 where w = 0) and the samples or the weight."""
    splat = is_splat(film)
    out = []
    for r, g, b, w in film_rows(film):
        if not splat:
            w &= 0xffffffff
        mean = model_mean_splat if splat else model_mean_linear
        out.append((0, 0, 0, 0) if w == 0 else (mean(r, w), mean(g, w), mean(b, w), w))
    return out


def model_source(film, t):
    return [tuple(m - t if m > t else 0 for m in e[:3]) for e in model_means(film)]


def half(n):
    return (n + 1) // 2


def model_layout(width, height, levels):
    out, first, w, h = [], 0, width, height
    for _ in range(levels):
        w, h = half(w), half(h)
        out.append((w, h, first))
        first += w * h
    return out, first


def clamp(v, last):
    return min(max(v, 0), last)


DOWN = (1, 3, 3, 1)


def model_down(src, w, h):
    """One level down: src = w x h texels of three integers in rows -> (dst, half(w), half(h))."""
    dw, dh = half(w), half(h)
    dst = []
    for j in range(dh):
        ys = [clamp(2 * j - 1 + d, h - 1) for d in range(4)]
        for i in range(dw):
            xs = [clamp(2 * i - 1 + d, w - 1) for d in range(4)]
            acc = [0, 0, 0]
            for wy, y in zip(DOWN, ys):
                for wx, x in zip(DOWN, xs):
                    v = src[y * w + x]
                    for c in range(3):
                        acc[c] = (acc[c] + wx * wy * v[c]) & MASK
            dst.append(tuple(((a + 32) & MASK) >> 6 for a in acc))
    return dst, dw, dh


def model_up_at(a, w, h, x, y):
    """up(a) at texel (x, y) of the finer level; a = w x h texels."""
    i, j = x >> 1, y >> 1
    i2 = clamp(i + 1 if x & 1 else i - 1, w - 1)
    j2 = clamp(j + 1 if y & 1 else j - 1, h - 1)
    p, q, r, s = a[j * w + i], a[j * w + i2], a[j2 * w + i], a[j2 * w + i2]
    return tuple(((9 * p[c] + 3 * q[c] + 3 * r[c] + s[c] + 8) & MASK) >> 4 for c in range(3))


def model_downs(film, width, height, t, levels=8):
    """[d_1 .. d_levels], each (texels, w, h)."""
    out, cur, w, h = [], model_source(film, t), width, height
    for _ in range(levels):
        cur, w, h = model_down(cur, w, h)
        out.append((cur, w, h))
    return out


def model_ups(downs, levels):
    """[u_1 .. u_levels] from the downs of model_downs (at least `levels` of them)."""
    ups = [None] * levels
    ups[levels - 1] = downs[levels - 1]
    for k in range(levels - 2, -1, -1):
        d, w, h = downs[k]
        a, aw, ah = ups[k + 1]
        u = []
        for y in range(h):
            for x in range(w):
                up = model_up_at(a, aw, ah, x, y)
                u.append(tuple((d[y * w + x][c] + up[c]) & MASK for c in range(3)))
        ups[k] = (u, w, h)
    return ups


def pyramid_of(ups):
    """The levels one behind the other, as (entries,) GLARE_DTYPE."""
    rows = [list(t) + [0] for texels, _, _ in ups for t in texels]
    return np.array(rows, dtype=np.uint64).reshape(-1, 4).view(ptss.GLARE_DTYPE).reshape(-1)


def model_pyramid(film, width, height, params, glare, downs=None):
    downs = downs if downs is not None else model_downs(film, width, height, model_threshold(glare.threshold, params), glare.levels)
    return pyramid_of(model_ups(downs, glare.levels))


def strength_word(strength):
    return int(F32(strength) * F32(65536) + F32(0.5))


def model_mixed(film, width, height, pyramid, glare):
    """Per pixel (m'_r, m'_g, m'_b, w): what the glare resolve shows in place of the means."""
    L = glare.levels
    u1w, u1h = half(width), half(height)
    u1 = [tuple(int(v) for v in e[:3]) for e in np.ascontiguousarray(pyramid).view(np.uint64).reshape(-1, 4)[:u1w * u1h]]
    s = strength_word(glare.strength)
    k = 65536 - s if glare.mode == ptss.GLARE_MIX else 65536
    out = []
    for p, (mr, mg, mb, w) in enumerate(model_means(film)):
        up = model_up_at(u1, u1w, u1h, p % width, p // width)
        g = [((u + L // 2) & MASK) // L for u in up]
        out.append(tuple(((m * k + gc * s + 32768) & MASK) >> 16 for m, gc in zip((mr, mg, mb), g)) + (w,))
    return out


def model_resolve_glare(film, width, height, pyramid, params, glare, state=None):
    """The glare resolve of every pixel -> (linear (P, 4) float32, pixels (P, 4) uint8, history (P, 4) float32)."""
    splat = is_splat(film)
    mixed = model_mixed(film, width, height, pyramid, glare)
    P = len(mixed)
    linear, pixels, history = np.zeros((P, 4), F32), np.zeros((P, 4), np.uint8), np.zeros((P, 4), F32)
    pixels[:, 3] = 255
    exposure = F32(params.exposure)
    if state is not None:
        exposure = F32(np.asarray(state)["exposure"].reshape(-1)[0]) * exposure
    with np.errstate(over="ignore", invalid="ignore"):
        for p, (a, b, c, w) in enumerate(mixed):
            if w == 0 and a == b == c == 0:
                continue
            for ch, m in enumerate((a, b, c)):
                mean = f32_of_int(m) * F32(2.0 ** -params.scaleLog2)
                ex = mean * exposure
                linear[p, ch] = mean
                pixels[p, ch] = oracle.probe_quantize(float(ex))
                history[p, ch] = F32(255) * host_pow([min(max(ex, F32(0)), F32(1))], GAMMA)[0]
            linear[p, 3] = history[p, 3] = (f32_of_int(w) * F32(2.0 ** -16)) if splat else F32(w)
    return linear, pixels, history


# ---- the films ---------------------------------------------------------------------------------------------------------------------------------
def pool_of(splat, params):
    """The rows the films are drawn from: the resolve rows of linear_common / splat_common (adversarial means, N = 0 rows among them) and
    the largest rows a film the library filled can hold."""
    if splat:
        return np.concatenate([splat_resolve_rows(params), largest_splat_rows()])
    return np.concatenate([linear_resolve_rows(params), largest_linear_rows()[0]])


def empty_row(splat):
    """A pixel without samples whose sums are not zero (they must not count)."""
    f = splat_film(1) if splat else linear_film(1)
    f["r"], f["g"], f["b"] = 5, 6, 7
    return f


def film_of(width, height, splat, params, seed=0, kind="pool"):
    """A width x height film. kind "pool": rows of pool_of drawn at random, pixels without samples at the four corners, on every edge
    and inside; "high": linear_common / splat_common's high_film (sums no call of the library leaves: the words wrap); "top": every mean
    2^40."""
    P = width * height
    if kind == "high":
        return high_splat_film(P) if splat else high_linear_film(P)
    if kind == "top":
        if splat:   # S = 2^24 Wt, the most the splat calls can leave
            f = splat_film(P)
            f["r"] = f["g"] = f["b"] = 3 << 24
            f["weight"] = 3
        else:       # three samples of 2^40
            f = linear_film(P)
            f["r"] = f["g"] = f["b"] = 3 * TOP
            f["samples"] = 3
        return f
    pool = pool_of(splat, params)
    g = np.random.default_rng(1000 * width + height + seed)
    f = pool[g.integers(0, len(pool), P)].copy()
    holes = {0, width - 1, P - width, P - 1, (height // 2) * width, (height // 2) * width + width - 1, width // 2, P - 1 - width // 2,
             (height // 2) * width + width // 2, (height // 3) * width + width // 3}
    for p in holes:
        f[p] = empty_row(splat)[0]
    return f


def thresholds_for(film, params):
    """0, one inside the data (the median of the means that are not zero, as radiance) and one above everything a library film holds."""
    means = sorted(m for e in model_means(film) for m in e[:3] if 0 < m <= TOP)
    inside = means[len(means) // 2] / 2.0 ** params.scaleLog2 if means else 0.25
    return (0.0, float(F32(inside)), float(2.0 ** (40 - params.scaleLog2)))


def impulse_film(width, height, x, y, value, splat=False):
    """All pixels sampled and black but (x, y), whose mean is `value` in all channels."""
    P = width * height
    f = splat_film(P) if splat else linear_film(P)
    if splat:
        f["weight"] = 65536
    else:
        f["samples"] = 1
    f["r"][y * width + x] = f["g"][y * width + x] = f["b"][y * width + x] = value
    return f


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def first_difference(a, b):
    """For a failing assert: the first entry at which two pyramids differ."""
    a, b = (np.ascontiguousarray(v).view(np.uint64).reshape(-1, 4) for v in (a, b))
    if a.shape != b.shape:
        return a.shape, b.shape
    bad = np.nonzero((a != b).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), a[bad[0]].tolist(), b[bad[0]].tolist(), len(bad))


def default_params():
    return params_of(20, 65536.0)


# ---- the launches of a build (csrc/ptss_glare.hip): what ptss_glare_launches must count ---------------------------------------------------------
def model_tail_level(width, height, levels):
    """The level the single-workgroup tail starts from: the first from which on all levels hold at most GLARE_TAIL_ENTRIES texels together;
    `levels` when only the last fits or none does (then no tail runs)."""
    lv = model_layout(width, height, levels)[0]
    held, T = 0, levels
    for k in range(levels, 0, -1):
        held += lv[k - 1][0] * lv[k - 1][1]
        if held > ptss.GLARE_TAIL_ENTRIES:
            break
        T = k
    return T


def model_build_kernels(width, height, levels):
    """Kernels one ptss_glare_build launches: the reduce, a down and an up per level below the tail's first, and the tail when it has a
    level to build."""
    T = model_tail_level(width, height, levels)
    return 1 + 2 * (T - 1) + (1 if T < levels else 0)


def every_kernel_sizes():
    """Two films sized by the header's constants: level 1 of the first is one texel wider than four tiles and holds just more texels than
    the tail takes, so the tail starts at level 2 and one down and one up kernel run; the second is twice that in both axes, the tail starts at
    level 3. Neither side is a multiple of the tile."""
    w1 = 4 * ptss.GLARE_TILE + 1
    h1 = -(-(ptss.GLARE_TAIL_ENTRIES + 1) // w1)
    return (2 * w1, 2 * h1), (4 * w1, 4 * h1)
