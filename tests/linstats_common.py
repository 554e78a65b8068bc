"""Models and cases shared by tests/test_linstats_cpu.py and the GPU tests of the linear film's sampling plan
(ptss_accumulate_paths_linear_stats / ptss_plan_samples_linear): a sample's luminance moments and the weight of a pixel in
Python integers and numpy float32 — independent of csrc/ptlinstats.h — and the moment rows the plan is tried on."""
import numpy as np

import ptss
from adaptive_common import UNSAMPLED, f32_of_int
from linear_common import MASK, model_fixed

LO_MASK = (1 << 40) - 1
MASK128 = (1 << 128) - 1
W_SCALE = np.float32(262144)
W_CAP = np.float32(524287)


def moment_words(m):
    return np.ascontiguousarray(m).view(np.uint64).reshape(-1, 4)


def zero_moments(P):
    return np.zeros(P, dtype=ptss.MOMENT_DTYPE)


def high_moments(P):
    """Moments whose words start at 2^62."""
    m = zero_moments(P)
    m["sumY"] = m["sqLo"] = m["sqHi"] = 1 << 62
    m["samples"] = 5
    return m


# ---- a sample ----------------------------------------------------------------------------------------------------------------------------------
def model_luminance(qr, qg, qb):
    return (54 * qr + 183 * qg + 19 * qb + 128) >> 8


def model_sample(radiance, params):
    """(y, lo, hi) of one radiance triple."""
    q = [model_fixed(radiance[c], params)[0] for c in range(3)]
    y = model_luminance(*q)
    assert y <= 1 << 40
    sq = y * y
    return y, sq & LO_MASK, sq >> 40


def model_accumulate_moments(results, moments, params, first_pixel=0, index=None):
    """The moment rows after ptss_accumulate_paths_linear_stats, in Python integers -> ((P, 4) uint64 rows, dropped)."""
    rad = np.ascontiguousarray(results).view(np.float32).reshape(-1, 4)
    rows = [[int(v) for v in e] for e in moment_words(moments)]
    dropped = 0
    for i, r in enumerate(rad):
        p = first_pixel + i if index is None else int(index[i])
        if p >= len(rows):
            dropped += 1
            continue
        y, lo, hi = model_sample(r, params)
        for c, v in enumerate((y, lo, hi, 1)):
            rows[p][c] = (rows[p][c] + v) & MASK
    return np.array(rows, dtype=np.uint64).reshape(-1, 4), dropped


# ---- the weight --------------------------------------------------------------------------------------------------------------------------------
def model_D(Sy, sqLo, sqHi, N, consistent=False):
    """D of the issue in exact integers, wrapped to 128 bits as the two-word arithmetic wraps."""
    Q = ((sqHi << 40) + sqLo) & MASK128
    A = (N * Q) & MASK128
    B = (Sy * Sy) & MASK128
    if consistent:
        assert N * ((sqHi << 40) + sqLo) >= Sy * Sy, "Cauchy-Schwarz"
        assert N * ((sqHi << 40) + sqLo) < 1 << 127 and Sy * Sy < 1 << 126
    return A - B if A >= B else 0


def model_sqrt128(D):
    """sqrt(D) as float32 by the issue's steps, written out."""
    hi = D >> 64
    if hi == 0:
        return np.sqrt(f32_of_int(D))
    s = hi.bit_length()
    s += s & 1
    m = D >> s
    if D & ((1 << s) - 1):
        m |= 1
    assert m < 1 << 64
    return np.sqrt(f32_of_int(m)) * np.float32(2.0 ** (s // 2))


def floor_fixed(params, plan):
    return np.float32(plan.floor) * np.float32(2.0 ** params.scaleLog2)


def model_rel(Sy, sqLo, sqHi, N, params, plan, consistent=False):
    r = model_sqrt128(model_D(Sy, sqLo, sqHi, N, consistent))
    fn = f32_of_int(N)
    se = r / (fn * np.sqrt(fn))
    mean = f32_of_int(Sy) / fn
    return se / (mean + floor_fixed(params, plan))


def model_weight(Sy, sqLo, sqHi, N, params, plan, consistent=False):
    if N < plan.minSamples:
        return UNSAMPLED
    if N >= plan.maxSamples:
        return 0
    with np.errstate(over="ignore"):
        rel = model_rel(Sy, sqLo, sqHi, N, params, plan, consistent)
    assert np.isfinite(rel)
    if not rel > np.float32(plan.threshold):
        return 0
    return int(min(rel * W_SCALE, W_CAP))


def model_weights(moments, params, plan, consistent=False):
    return [model_weight(int(e[0]), int(e[1]), int(e[2]), int(e[3]), params, plan, consistent) for e in moment_words(moments)]


def check_plan(moments, n, params, plan, cdf, index, info, weights=None):
    """The plan (cdf, index, info) against the model's weights and the three properties, in Python integers."""
    w = weights if weights is not None else model_weights(moments, params, plan)
    P, total = len(w), sum(w)
    assert [int(c) for c in cdf] == list(np.cumsum(np.array(w, dtype=object))), "cdf"
    N = moment_words(moments)[:, 3]
    want = dict(totalWeight=total, activePixels=sum(1 for v in w if v > 0), unsampledPixels=int((N < plan.minSamples).sum()),
                cappedPixels=int((N >= plan.maxSamples).sum()), uniform=int(total == 0))
    assert info == want, (info, want)
    assert len(index) == n
    idx = index.astype(np.int64)
    assert (np.diff(idx) >= 0).all() and (n == 0 or (0 <= idx[0] and idx[-1] < P)), "non-decreasing, inside the film"
    if total == 0:
        assert [int(v) for v in idx] == [(i * P + P // 2) // n for i in range(n)], "uniform fallback"
        return
    count = np.bincount(idx, minlength=P)
    for p in range(P):
        assert abs(int(count[p]) * total - n * w[p]) < total, (p, int(count[p]), w[p], total, n)
        assert w[p] > 0 or count[p] == 0, p


# ---- moment rows -------------------------------------------------------------------------------------------------------------------------------
def row_of_ys(ys):
    """The consistent moment row of luminances ys (Python integers, each <= 2^40)."""
    ys = [int(y) for y in ys]
    return [sum(ys), sum((y * y) & LO_MASK for y in ys), sum((y * y) >> 40 for y in ys), len(ys)]


def moments_of_rows(rows):
    return np.array(rows, dtype=np.uint64).reshape(-1, 4).view(ptss.MOMENT_DTYPE).reshape(-1)


def consistent_moments(samples, g, scale=1 << 20, spread=1.0):
    """A consistent moment film: pixel p holds samples[p] luminances around a random mean (log-uniform below `scale` * 64), noise
    proportional to it by `spread` (0: every sample equal, D = 0)."""
    rows = []
    for N in samples:
        mean = float(np.exp(g.uniform(0, np.log(64.0 * scale))))
        ys = np.clip(np.rint(mean * (1.0 + spread * g.uniform(0, 1.5) * g.standard_normal(int(N)))), 0, float(1 << 40)).astype(np.int64)
        rows.append(row_of_ys(ys))
    return moments_of_rows(rows) if rows else zero_moments(0)


def random_word_moments(P, g):
    """Random words as moments: inputs that do not belong together (the arithmetic wraps; both sides must still agree). A third has sample
    counts a plan may meet, and of those some have small words, so that every branch is met."""
    m = g.integers(0, 2 ** 63, (P, 4), dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, (P, 4), dtype=np.uint64)
    m[::3, 3] = g.integers(0, 64, len(m[::3]))
    m[::6, 0] >>= np.uint64(30)
    m[::6, 2] >>= np.uint64(50)
    m[::12, 2] = 0
    m[::12, 1] >>= np.uint64(20)
    m[3::12, 0] >>= np.uint64(50)   # a small sum under a large second moment: the cap
    return m.view(ptss.MOMENT_DTYPE).reshape(-1)


def conversion_rows():
    """Consistent rows with D = 0, D just below and above 2^64 (the two conversion paths), an odd and an even bit length of D's high
    word, and D near 2^127 — each as (what, row)."""
    rows = []
    rows.append(("D = 0, dark", row_of_ys([0] * 8)))
    rows.append(("D = 0, bright", row_of_ys([1 << 40] * 9)))
    rows.append(("D = 0, mid", row_of_ys([123456789] * 100)))
    # two values a and b, k each: D = N^2 ((a - b) / 2)^2 = (k (a - b))^2
    for what, k, d in (("D just below 2^64", 4, (1 << 30) - 1), ("D = 2^64", 4, 1 << 30), ("D just above 2^64", 4, (1 << 30) + 1),
                       ("high word of 1 bit", 4, (1 << 30) + 5), ("high word of 2 bits", 4, 3 << 29), ("high word of 3 bits", 5, 1 << 31),
                       ("high word of 4 bits", 4, 1 << 32), ("high word of 21 bits", 8, 1 << 39), ("high word of 22 bits", 8, (1 << 39) + (1 << 38))):
        rows.append((what, row_of_ys([5, 5 + d] * k)))
    # D near 2^127: N = 2^23 - 2 samples, half at 0 and half at 2^40 -> D = (N / 2 * 2^40)^2 just below 2^124; the largest D a film can hold
    # is N^2 2^80 / 4 < 2^124, so 2^127 itself is reached by words that do not belong together (random_word_moments, and below)
    h = (1 << 22) - 1
    y = 1 << 40
    rows.append(("D at a consistent film's maximum", [h * y, h * ((y * y) & LO_MASK), h * ((y * y) >> 40), 2 * h]))
    return rows


def inconsistent_rows():
    """Rows no film holds: D near 2^127 and 2^128, A < B, words that wrap."""
    top = (1 << 64) - 1
    return [("D near 2^127", [0, 0, 1 << 63, (1 << 23) - 1]), ("A wraps to 0", [0, 0, 1 << 63, 16]), ("D near 2^128", [1, top, top, 9]),
            ("A < B", [1 << 50, 0, 0, 9]), ("B wraps", [top, top, top, 8]), ("all ones", [top, top, top, (1 << 23) - 1]),
            ("sticky bit set", [0, 1, 1 << 40, 8]), ("sticky bit clear", [0, 0, 1 << 40, 8])]
