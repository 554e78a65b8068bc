"""Models and cases shared by tests/test_linear_cpu.py and tests/test_gpu_linear.py (ptss_accumulate_paths_linear / ptss_resolve_linear;
DESIGN.md §3.29): the fixed-point sample and the resolve of a film entry in Python integers, exact fractions and numpy float32 —
independent of csrc/ptlinear.h — and the rows the two calls are tried on."""
import ctypes as C
from fractions import Fraction

import numpy as np

import oracle
import ptss
from adaptive_common import f32_of_int
from film_common import quant_thresholds, results_of

MASK = (1 << 64) - 1
# scaleLog2 with the largest clampMax it allows (clampMax * 2^scaleLog2 = 2^40), and the defaults
SCALES = ((0, 2.0 ** 40), (20, 2.0 ** 20), (32, 256.0), (20, 65536.0))


def params_of(scale_log2, clamp_max, exposure=1.0):
    return ptss.linear_params(scale_log2=scale_log2, clamp_max=clamp_max, exposure=exposure)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def model_fixed(x, params):
    """One channel -> (q, counted): the issue's rule in exact rational arithmetic."""
    x = np.float32(x)
    if np.isnan(x):
        return 0, 1
    counted = 0
    if x > np.float32(params.clampMax):
        x, counted = np.float32(params.clampMax), 1
    if not x > 0:
        return 0, counted
    s = Fraction(float(x)) * (1 << params.scaleLog2)
    k = s.numerator // s.denominator
    rest = s - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1):
        k += 1
    return k, counted


def model_accumulate(results, film, params, first_pixel=0, index=None):
    """ptss_accumulate_paths_linear in Python integers -> (film afterwards as (P, 4) uint64 rows, dropped)."""
    rad = np.ascontiguousarray(results).view(np.float32).reshape(-1, 4)
    rows = [[int(v) for v in e] for e in np.ascontiguousarray(film).view(np.uint64).reshape(-1, 4)]
    dropped = 0
    for i, r in enumerate(rad):
        p = first_pixel + i if index is None else int(index[i])
        if p >= len(rows):
            dropped += 1
            continue
        qs = [model_fixed(r[c], params) for c in range(3)]
        for c in range(3):
            rows[p][c] = (rows[p][c] + qs[c][0]) & MASK
        samples, clamped = rows[p][3] & 0xffffffff, rows[p][3] >> 32
        samples = (samples + 1) & 0xffffffff
        clamped = (clamped + (1 if any(q[1] for q in qs) else 0)) & 0xffffffff
        rows[p][3] = samples | (clamped << 32)
    return np.array(rows, dtype=np.uint64).reshape(-1, 4), dropped


_f32p = C.POINTER(C.c_float)


def host_pow(x, y):
    """ptm::pow on the host (ptss_probe_math op 6), float32 in and out."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    y = np.full_like(x, y)
    out = np.empty_like(x)
    assert ptss.host_lib().ptss_probe_math(6, x.ctypes.data_as(_f32p), y.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p), x.size) == 0
    return out


GAMMA = np.float32(1) / np.float32(2.2)   # ptm::kGamma = (1 / 2.2f)


def model_mean(total, N, params):
    """(m, mean): the integer mean and its float."""
    m = ((total + N // 2) & MASK) // N
    return m, f32_of_int(m) * np.float32(2.0 ** -params.scaleLog2)


def model_resolve(film, params):
    """ptss_resolve_linear of every entry -> (linear (P, 4) float32, pixels (P, 4) uint8, history (P, 4) float32)."""
    rows = np.ascontiguousarray(film).view(np.uint64).reshape(-1, 4)
    P = len(rows)
    linear, pixels, history = np.zeros((P, 4), np.float32), np.zeros((P, 4), np.uint8), np.zeros((P, 4), np.float32)
    pixels[:, 3] = 255
    exposure = np.float32(params.exposure)
    for p, e in enumerate(rows):
        N = int(e[3]) & 0xffffffff
        if N == 0:
            continue
        for c in range(3):
            _, mean = model_mean(int(e[c]), N, params)
            ex = mean * exposure
            linear[p, c] = mean
            pixels[p, c] = oracle.probe_quantize(float(ex))
            history[p, c] = np.float32(255) * host_pow([min(max(ex, np.float32(0)), np.float32(1))], GAMMA)[0]
        linear[p, 3] = history[p, 3] = np.float32(N)
    return linear, pixels, history


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------------
def up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def adversarial_channels(params, g):
    """float32 values for one channel: the special values, clampMax and its neighbours, ties of the rounding for even and odd k with their
    neighbours, half a unit, and random radiance."""
    s = params.scaleLog2
    unit = 2.0 ** -s
    cm = np.float32(params.clampMax)
    v = [np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, -1e-30, -3e38, 1e-45, 1e-38, -1e-45, 1.1754944e-38, cm, up(cm), down(cm), up(up(cm)), 3e38,
         unit / 2, up(unit / 2), down(unit / 2), unit, unit / 4, 0.18, 0.5, 1.0, 40.0]
    for k in (0, 1, 2, 3, 4, 5, 1000, 1001, 65534, 65535, (1 << 22) - 2, (1 << 22) - 1):   # (k + 0.5) units: exact in float32 while k < 2^22
        tie = np.float32((k + 0.5) * unit)
        if tie <= cm:
            v += [tie, up(tie), down(tie)]
    v += list((g.uniform(0, 1.3, 90) ** 4 * min(float(cm), 50.0)).astype(np.float32))
    return np.array(v, dtype=np.float32)


def adversarial_results(params, seed=3):
    """(M,) PATH_RESULT_DTYPE: the adversarial channels in every channel position, beside one another in three orders."""
    g = np.random.default_rng(seed)
    v = adversarial_channels(params, g)
    v = np.concatenate([v, np.zeros((-len(v)) % 3, dtype=np.float32)])
    rows = np.concatenate([v.reshape(-1, 3), g.permutation(v).reshape(-1, 3), g.permutation(v).reshape(-1, 3),
                           np.stack([v, np.full_like(v, 0.25), np.full_like(v, -1.0)], axis=1)])
    return results_of(rows.astype(np.float32))


def linear_film(P):
    return np.zeros(P, dtype=ptss.LINEAR_DTYPE)


def high_film(P):
    """A film whose sums start at 2^62."""
    f = linear_film(P)
    f["r"] = f["g"] = f["b"] = 1 << 62
    f["samples"], f["clamped"] = 5, 1
    return f


def entry(r, g, b, samples, clamped=0):
    f = linear_film(1)
    f["r"], f["g"], f["b"], f["samples"], f["clamped"] = r, g, b, samples, clamped
    return f


def resolve_rows(params):
    """(P,) LINEAR_DTYPE: N = 0, N = 1, integer means that round both ways, m above 2^24 where the conversion rounds (ties included), m at
    2^40, and sums that put the exposed mean around tone-map thresholds (for exposure 1: the caller scales for others)."""
    s = params.scaleLog2
    one = 1 << s
    rows = [entry(0, 0, 0, 0), entry(123, 456, 789, 0, 3), entry(0, 0, 0, 1), entry(one, one // 2, 3, 1), entry(one // 3 + 1, 1, 2, 1)]
    for N in (2, 3, 4, 7, 300):   # (sum + N / 2) / N rounds down, up, and sits on the half
        base = 5 * one // 7
        rows.append(entry(base * N, base * N + N // 2, base * N + N // 2 + 1, N))
        rows.append(entry(base * N + (N - 1) // 2, base * N + N - 1, max(base * N - 1, 0), N))
    big = 1 << 25   # floats are 4 apart in [2^25, 2^26): + 1 rounds down, + 2 is a tie that goes down (to even), + 3 up, + 6 a tie that goes up
    rows.append(entry(big + 1, big + 2, big + 3, 1))
    rows.append(entry(big + 6, big + 5, big + 4, 1))
    rows.append(entry(3 * (big + 2), 3 * (big + 6) + 1, 3 * (big + 10) - 1, 3))
    rows.append(entry(1 << 40, (1 << 40) - 1, (1 << 39) + 1, 1))
    rows.append(entry(7 << 40, (7 << 40) - 4, (7 << 40) + 3, 7))
    rows.append(entry((1 << 62) + (300 << 40), 1 << 62, (1 << 62) + 12345, 300))
    T = quant_thresholds()[1:256]
    for t in (T[0], T[1], T[17], T[127], T[200], T[254]):   # means on a threshold and on its neighbours (exact while t * 2^s is an integer below 2^24; else near it)
        for x in (down(t), t, up(t)):
            q = int(Fraction(float(x)) * one)
            rows.append(entry(q, q + 1, max(q - 1, 0), 1))
            rows.append(entry(5 * q + 2, 5 * q, 5 * q + 3, 5))
    return np.concatenate(rows)


def same_words(a, b):
    """Equal 32-bit words, a NaN standing for any NaN."""
    a = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)
    b = np.ascontiguousarray(b).view(np.uint32).reshape(len(b), -1)
    if a.shape != b.shape:
        return False
    fa, fb = a.view(np.float32), b.view(np.float32)
    return bool(((a == b) | (np.isnan(fa) & np.isnan(fb))).all())


def film_words(f):
    return np.ascontiguousarray(f).view(np.uint64).reshape(-1, 4)
