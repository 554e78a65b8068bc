"""Models and cases shared by tests/test_splat_cpu.py and tests/test_gpu_splat.py (ptss_splat_paths / ptss_splat_paths_homed /
ptss_resolve_splat): the filter profiles in numpy float32 (exp through ptss_probe_math), the integer weights, the
contributions and the resolve with the wide division in Python integers, the drop and stray rules — independent of csrc/ptsplat.h — and
the positions and radiance rows the calls are tried on. The model looks for taps three pixels either side of a sample, more than any
radius reaches, so it does not lean on the window the header derives."""
import ctypes as C

import numpy as np

import oracle
import ptss
from adaptive_common import f32_of_int
from film_common import results_of
from linear_common import GAMMA, MASK, adversarial_results, host_pow, model_fixed

F32 = np.float32
KINDS = ("box", "tent", "gaussian")
RADII = (0.5, 1.0, 1.5, 2.0)
FW, FH = 40, 24          # the film of the GPU tests: no multiple of the 16 x 16 tile
JITTER_SEED = 0x51A7     # the streams of the jitter = 1 box identity: test_splat_cpu checks that no position they give lies on an integer
_f32p = C.POINTER(C.c_float)


def filters():
    """Every kind at every radius; the Gaussian with two alphas."""
    out = [ptss.splat_filter(kind, radius) for kind in KINDS for radius in RADII]
    return out + [ptss.splat_filter("gaussian", 1.5, 0.5), ptss.splat_filter("gaussian", 2.0, 7.25)]


def name_of(f):
    return "%s-%g-%g" % (KINDS[f.kind], f.radius, f.alpha)


def host_exp(x):
    """ptm::exp on the host (ptss_probe_math op 5) of one float32."""
    x = np.array([x], dtype=np.float32)
    out = np.empty_like(x)
    assert ptss.host_lib().ptss_probe_math(5, x.ctypes.data_as(_f32p), None, out.ctypes.data_as(_f32p), 1) == 0
    return out[0]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
class Model:
    """A ptss_splat_filter as the model sees it: the constants evaluated once, in float32."""

    def __init__(self, f):
        self.kind, self.R, self.alpha = KINDS[f.kind], F32(f.radius), F32(f.alpha)
        self.invR = F32(1) / self.R
        self.c = host_exp(-(self.alpha * (self.R * self.R))) if self.kind == "gaussian" else F32(0)
        self._cache = {}

    def profile(self, d):
        d = F32(d)
        if self.kind == "box":
            return F32(1) if -self.R <= d < self.R else F32(0)
        if self.kind == "tent":
            v = F32(1) - np.abs(d) * self.invR
            return v if v > 0 else F32(0)
        if not np.abs(d) < self.R:
            return F32(0)
        v = host_exp(-(self.alpha * (d * d))) - self.c
        return v if v > 0 else F32(0)

    def axis_weight(self, X, i):
        key = (np.float32(X).tobytes(), i)
        if key not in self._cache:
            d = F32(X) - (F32(i) + F32(0.5))
            self._cache[key] = int(F32(self.profile(d) * F32(65536) + F32(0.5)))
        return self._cache[key]

    def outside(self, X, extent):
        X = F32(X)
        return not (X >= -self.R and X <= F32(extent) + self.R)   # NaN and the infinities fail a comparison


def is_stray(X, Y, hx, hy):
    X, Y = F32(X), F32(Y)
    return not (F32(hx) <= X <= F32(hx + 1) and F32(hy) <= Y <= F32(hy + 1))


def model_splat(results, positions, film, width, height, filt, params, homed_first_pixel=None):
    """ptss_splat_paths / ptss_splat_paths_homed in Python integers -> (film afterwards as (P, 4) uint64 rows, dropped, clamped)."""
    M = filt if isinstance(filt, Model) else Model(filt)
    rad = np.ascontiguousarray(results).view(np.float32).reshape(-1, 4)
    pos = np.ascontiguousarray(positions).view(np.float32).reshape(-1, 2)
    rows = [[int(v) for v in e] for e in np.ascontiguousarray(film).view(np.uint64).reshape(-1, 4)]
    dropped = clamped = 0
    for k, ((X, Y), r) in enumerate(zip(pos, rad)):
        if homed_first_pixel is None:
            drop = M.outside(X, width) or M.outside(Y, height)
        else:
            home = homed_first_pixel + k
            drop = is_stray(X, Y, home % width, home // width)
        if drop:
            dropped += 1
            continue
        qs = [model_fixed(r[c], params) for c in range(3)]
        clamped += 1 if any(q[1] for q in qs) else 0
        nx, ny = int(np.floor(X)), int(np.floor(Y))
        for j in range(max(ny - 3, 0), min(ny + 4, height)):
            wy = M.axis_weight(Y, j)
            if wy == 0:
                continue
            for i in range(max(nx - 3, 0), min(nx + 4, width)):
                Wt = (M.axis_weight(X, i) * wy + 32768) >> 16
                if Wt == 0:
                    continue
                e = rows[j * width + i]
                for c in range(3):
                    e[c] = (e[c] + ((qs[c][0] * Wt + 32768) >> 16)) & MASK
                e[3] = (e[3] + Wt) & MASK
    return np.array(rows, dtype=np.uint64).reshape(-1, 4), dropped, clamped


def model_resolve_splat(film, params):
    """ptss_resolve_splat of every entry -> (linear (P, 4) float32, pixels (P, 4) uint8, history (P, 4) float32): the mean by the wide
    division floor((S 2^16 + Wt / 2) / Wt), the rest as linear_common.model_resolve."""
    rows = np.ascontiguousarray(film).view(np.uint64).reshape(-1, 4)
    P = len(rows)
    linear, pixels, history = np.zeros((P, 4), np.float32), np.zeros((P, 4), np.uint8), np.zeros((P, 4), np.float32)
    pixels[:, 3] = 255
    exposure = F32(params.exposure)
    for p, e in enumerate(rows):
        Wt = int(e[3])
        if Wt == 0:
            continue
        for c in range(3):
            m = ((int(e[c]) << 16) + Wt // 2) // Wt
            mean = f32_of_int(m) * F32(2.0 ** -params.scaleLog2)
            ex = mean * exposure
            linear[p, c] = mean
            pixels[p, c] = oracle.probe_quantize(float(ex))
            history[p, c] = F32(255) * host_pow([min(max(ex, F32(0)), F32(1))], GAMMA)[0]
        linear[p, 3] = history[p, 3] = f32_of_int(Wt) * F32(2.0 ** -16)
    return linear, pixels, history


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------------
def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def splat_film(P=FW * FH):
    return np.zeros(P, dtype=ptss.SPLAT_DTYPE)


def high_film(P=FW * FH):
    """A film whose sums start at 2^62."""
    f = splat_film(P)
    f["r"] = f["g"] = f["b"] = 1 << 62
    f["weight"] = 5 << 16
    return f


def film_words(f):
    return np.ascontiguousarray(f).view(np.uint64).reshape(-1, 4)


def positions_of(xy):
    p = np.zeros(len(xy), dtype=ptss.POSITION_DTYPE)
    a = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    p["x"], p["y"] = a[:, 0], a[:, 1]
    return p


def scatter_positions(width=FW, height=FH):
    """(x, y) rows for the scatter form: pixel centres, integer coordinates (corners and edges of pixels), one ulp either side of integers
    and of the half-integers where a box or tent edge falls, every film border and corner with its neighbours, just inside and outside the
    drop range of each radius, positions far outside, NaN and the infinities."""
    xs = [0.5, 1.5, 7.5, width - 0.5, 0.0, 1.0, 2.0, 17.0, float(width), float(width - 1), up(0.0), down(1.0), up(1.0), down(2.0), up(2.0),
          down(17.0), up(17.0), down(width), up(width), down(16.5), 16.5, up(16.5), 5.25, 5.75, 9.001, -0.25, -0.5, down(-0.5), -1.0, -1.5, -2.0,
          down(-2.0), width + 0.5, up(width + 0.5), width + 1.0, width + 2.0, up(width + 2.0), 1e-30, 3.3]
    scale = height / width
    pts = []
    for k, x in enumerate(xs):   # every x beside an interior y, every such y (scaled to the film's height) beside an interior x, and the diagonal
        y = (float(height) if x == width else x * scale if x > 3 else x) if k % 3 else x
        pts += [(x, 6.5 + (k % 5) * 0.2), (11.25 + (k % 7) * 0.125, min(y, height + 2.5)), (x, min(y, height + 2.5))]
    for cx in (0.0, float(width)):
        for cy in (0.0, float(height)):
            pts += [(cx, cy), (up(cx), down(cy)) if cy else (up(cx), up(cy)), (abs(cx - 0.5), abs(cy - 0.5))]
    bad = [(np.nan, 3.0), (3.0, np.nan), (np.nan, np.nan), (np.inf, 3.0), (3.0, -np.inf), (-np.inf, np.inf), (1e9, 3.0), (3.0, -1e9), (-40.0, -40.0),
           (2.0 ** 22 + 7, 1.0), (width + 2.5, 2.0), (2.0, height + 2.5), (-2.5, 2.0)]
    return positions_of(np.array(pts + bad, dtype=np.float32))


def radiance_rows(n, seed=0):
    """(n,) PATH_RESULT_DTYPE: linear_common's adversarial rows for the default parameters, repeated and permuted to length n."""
    base = adversarial_results(ptss.linear_params(), seed=seed)
    g = np.random.default_rng(seed + 77)
    reps = np.concatenate([base[g.permutation(len(base))] for _ in range(n // len(base) + 1)])
    return reps[:n]


def scatter_case(seed=0):
    """The scatter rows: every position of scatter_positions beside an adversarial radiance row -> (results, positions)."""
    pos = scatter_positions()
    return radiance_rows(len(pos), seed), pos


def homed_positions(first_pixel, n, seed=0, width=FW):
    """One position per home first_pixel .. first_pixel + n: the home's corners and edges (the K window), one ulp inside them, its
    centre, random places inside, and a few strays (one ulp outside, a neighbour's centre, NaN, far away) -> ((n,) POSITION_DTYPE, strays)."""
    g = np.random.default_rng(1000 + seed)
    xy = np.zeros((n, 2), dtype=np.float32)
    stray = np.zeros(n, dtype=bool)
    for k in range(n):
        hx, hy = (first_pixel + k) % width, (first_pixel + k) // width
        kind = k % 16 if n >= 16 else (k * 5 + seed) % 16
        if kind < 4:
            x, y = hx + (kind & 1), hy + (kind >> 1)                       # the four corners
        elif kind < 8:
            x, y = ((hx + 0.5, hy), (hx + 0.5, hy + 1), (hx, hy + 0.5), (hx + 1, hy + 0.5))[kind - 4]   # the middle of an edge
        elif kind == 8:
            x, y = up(hx), down(hy + 1)
        elif kind == 9:
            x, y = down(hx + 1), up(hy)
        elif kind == 10:
            x, y = hx + 0.5, hy + 0.5
        elif kind == 11 and k % 32 == 11:
            x, y = ((down(hx), hy + 0.5) if hx else (hx + 0.5, up(hy + 1)), (hx + 1.5, hy + 0.5), (np.nan, hy + 0.5), (hx + 0.5, -1e6))[(k // 32) % 4]
            stray[k] = True
        else:
            x, y = hx + g.uniform(0, 1), hy + g.uniform(0, 1)
        xy[k] = (x, y)
    return positions_of(xy), stray


def same_words(a, b):
    """Equal 32-bit words, a NaN standing for any NaN."""
    a = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)
    b = np.ascontiguousarray(b).view(np.uint32).reshape(len(b), -1)
    if a.shape != b.shape:
        return False
    fa, fb = a.view(np.float32), b.view(np.float32)
    return bool(((a == b) | (np.isnan(fa) & np.isnan(fb))).all())


def entry(r, g, b, weight):
    f = splat_film(1)
    f["r"], f["g"], f["b"], f["weight"] = r, g, b, weight
    return f


def resolve_rows(params):
    """(P,) SPLAT_DTYPE: Wt = 0, Wt a multiple of 65536 and not, means that round both ways, m above 2^24 (ties included), sums near 2^62
    over weights near 2^39, and sums that put the exposed mean around tone-map thresholds."""
    from fractions import Fraction
    from film_common import quant_thresholds
    s = params.scaleLog2
    one, w1 = 1 << s, 1 << 16
    rows = [entry(0, 0, 0, 0), entry(123, 456, 789, 0), entry(one, one // 2, 3, w1), entry(one // 3 + 1, 1, 2, w1), entry(one, one // 2, 3, 1),
            entry(one, 7, 0, 12288), entry(5 * one, one + 1, 2, 53248 + 16384), entry(one // 7, one, 1, 65535), entry(one, one, one, 65537)]
    for Wt in (2 * w1, 3 * w1, 3 * w1 + 1, 7 * w1 - 1, 300 * w1, 48998, 9270 + 51136):
        base = 5 * one // 7
        S = base * Wt >> 16
        rows.append(entry(S, S + 1, S + Wt, Wt))
        rows.append(entry(S + (Wt >> 17), S + (Wt >> 17) + 1, max(S - 1, 0), Wt))
    big = 1 << 25   # floats are 4 apart in [2^25, 2^26)
    rows.append(entry(big + 1, big + 2, big + 3, w1))
    rows.append(entry(big + 6, big + 5, big + 4, w1))
    rows.append(entry(3 * (big + 2), 3 * (big + 6) + 1, 3 * (big + 10) - 1, 3 * w1))
    rows.append(entry((big + 2) // 2, (big + 6) // 2, (big + 3) // 2, w1 // 2))
    rows.append(entry(1 << 40, (1 << 40) - 1, (1 << 39) + 1, w1))
    rows.append(entry((1 << 62) + (300 << 40), 1 << 62, (1 << 63) - 1, (1 << 39) - 1))
    rows.append(entry((1 << 63) - 1, (1 << 62) + 12345, 1 << 61, (1 << 38) + 12345))
    rows.append(entry((1 << 63) - 1, (1 << 63) - 2, 1 << 62, (1 << 23) * w1 - 1))
    T = quant_thresholds()[1:256]
    for t in (T[0], T[1], T[17], T[127], T[200], T[254]):
        for x in (down(t), t, up(t)):
            q = int(Fraction(float(x)) * one)
            rows.append(entry(q, q + 1, max(q - 1, 0), w1))
            rows.append(entry(5 * q + 2, 5 * q, 5 * q + 3, 5 * w1))
            rows.append(entry(q * 12288 >> 16, q * 53248 >> 16, (q * 20480 >> 16) + 1, 12288 + 53248))
    return np.concatenate(rows)
