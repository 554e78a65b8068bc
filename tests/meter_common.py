"""Models and cases shared by tests/test_meter_cpu.py and tests/test_gpu_meter.py (ptss_meter_linear / ptss_meter_splat /
ptss_meter_exposure): the bin of a film entry, the histogram, the ranks, C and sumLog in Python integers — independent of
csrc/ptmeter.h — and the three float steps in numpy float32 with ptm::exp taken through ptss_probe_math (the host's ptm::div is the IEEE
quotient, which numpy's float32 division is too), so the model is exact as well."""
import ctypes as C
from fractions import Fraction

import numpy as np

import ptss
from adaptive_common import f32_of_int
from linear_common import MASK, entry, high_film, linear_film
from splat_common import splat_film

BINS = 329
LAST = BINS - 1
LN2 = np.float32(0.69314718)
_f32p = C.POINTER(C.c_float)


def host_exp(x):
    """ptm::exp on the host (ptss_probe_math op 5), one float32."""
    a = np.array([x], dtype=np.float32)
    out = np.empty_like(a)
    assert ptss.host_lib().ptss_probe_math(5, a.ctypes.data_as(_f32p), None, out.ctypes.data_as(_f32p), 1) == 0
    return out[0]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def model_mean_linear(total, N):
    return ((total + N // 2) & MASK) // N


def model_mean_splat(S, Wt):
    m = ((S << 16) + Wt // 2) // Wt   # the wide division itself
    if Wt < 1 << 39 and S // Wt < 1 << 48:
        return m
    a, rem = S // Wt, S % Wt   # beyond what the split is exact for (no film the library filled): the split's own wrapping words
    return (((a << 16) & MASK) + ((((rem << 16) & MASK) + Wt // 2) & MASK) // Wt) & MASK


def model_luminance(mr, mg, mb):
    return ((54 * mr + 183 * mg + 19 * mb + 128) & MASK) >> 8   # (a film the library filled never wraps)


def model_bin_of_luminance(Y):
    if Y == 0:
        return 0
    e = Y.bit_length() - 1
    if e > 40:
        return LAST
    sub = ((Y >> (e - 3)) if e >= 3 else (Y << (3 - e))) & 7
    return 1 + 8 * e + sub


def model_bin(words, splat=False):
    """(bin or -1, Y) of one entry given as its four 64-bit words."""
    r, g, b, w = (int(v) for v in words)
    if not splat:
        w &= 0xffffffff
    if w == 0:
        return -1, 0
    mean = model_mean_splat if splat else model_mean_linear
    Y = model_luminance(mean(r, w), mean(g, w), mean(b, w))
    return model_bin_of_luminance(Y), Y


def film_rows(film):
    return np.ascontiguousarray(film).view(np.uint64).reshape(-1, 4)


def model_histogram(film, splat=False, first_pixel=0, count=None, histogram=None):
    rows = film_rows(film)
    count = len(rows) - first_pixel if count is None else count
    h = [0] * BINS if histogram is None else [int(v) for v in histogram]
    for e in rows[first_pixel:first_pixel + count]:
        b, _ = model_bin(e, splat)
        if b >= 0:
            h[b] = (h[b] + 1) & 0xffffffff
    return np.array(h, dtype=np.uint32)


def f32_of_fraction(v):
    """The float32 nearest to the exact rational v, ties to even: the candidates around the double nearest to v, compared exactly."""
    c = np.float32(float(v))
    best = None
    for x in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(x):
            continue
        d = abs(Fraction(float(x)) - v)
        even = (int(np.float32(x).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, x)
    return np.float32(best[1])


def new_state():
    return np.zeros(1, dtype=ptss.METER_STATE_DTYPE)


def model_exposure(histogram, state, params, meter):
    """ptss_meter_exposure -> the state afterwards, (1,) METER_STATE_DTYPE."""
    h = [int(v) for v in histogram]
    s = np.array(state, dtype=ptss.METER_STATE_DTYPE).reshape(1).copy()
    fresh = int(s["updates"][0]) == 0
    prev = np.float32(1) if fresh else s["exposure"][0]
    lo_f, hi_f = np.float32(meter.minExposure), np.float32(meter.maxExposure)
    clamp = lambda x: min(max(x, lo_f), hi_f)
    T = sum(h[1:])
    target = exposure = prev
    mean_log2 = np.float32(0) if fresh else s["meanLog2"][0]
    Cn = sum_log = 0
    if T:
        lo, hi = T * meter.lowPermille // 1000, T - T * meter.highPermille // 1000
        before = 0
        for b in range(1, BINS):
            end = before + h[b]
            sum_log += max(0, min(end, hi) - max(before, lo)) * (2 * (b - 1) + 1)
            before = end
        Cn = hi - lo
        assert Cn >= 1
        with np.errstate(over="ignore", invalid="ignore"):
            mean_log2 = f32_of_int(sum_log) / (f32_of_int(Cn) * np.float32(16)) - np.float32(params.scaleLog2)
            target = clamp(np.float32(meter.key) * host_exp(-mean_log2 * LN2))
            if fresh:
                exposure = target
            else:   # ptm::fma: one rounding of the exact (target - prev) * rate + prev
                d = np.float32(target - prev)
                exposure = clamp(f32_of_fraction(Fraction(float(d)) * Fraction(float(np.float32(meter.rate))) + Fraction(float(prev))))
    s["exposure"], s["target"], s["meanLog2"] = exposure, target, mean_log2
    s["updates"] = min(int(s["updates"][0]) + 1, 0xffffffff)
    s["metered"], s["black"], s["counted"], s["sumLog"] = T, h[0], Cn, sum_log
    return s


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------------
def luminance_values():
    """0, 1, 2, 7, 8, 9 and every 2^k, 2^k +- 1 up to 2^40 (2^40 + 1 is beyond a film the library filled and is left out)."""
    v = {0, 1, 2, 7, 8, 9}
    for k in range(41):
        v |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    return sorted(y for y in v if y <= 1 << 40)


def means_for(Y):
    """Channel means (each at most 2^40) whose luminance is exactly Y, in a few shapes: grey, and ones that reach Y through the weights and
    the + 128 rounding."""
    out = [(Y, Y, Y)]
    for mr, mb in ((0, 0), (1, 0), (Y // 2, Y // 3), (min(Y * 2, 1 << 40), 0), (0, min(Y * 4, 1 << 40))):
        # 183 mg in [256 Y - 128 - rest, 256 Y + 127 - rest]
        rest = 54 * mr + 19 * mb
        lo, hi = 256 * Y - 128 - rest, 256 * Y + 127 - rest
        mg = -(-max(lo, 0) // 183)
        if lo <= 183 * mg <= hi and mg <= 1 << 40:
            out.append((mr, mg, mb))
    return out


def linear_entry_of_means(m, N):
    """A linear entry with samples = N whose integer means are m: sums m * N (+ less than half a sample, which rounds away)."""
    return entry(m[0] * N, m[1] * N + (N - 1) // 2, max(m[2] * N - N // 2, 0) if N > 1 else m[2] * N, N)


def splat_entry_of_means(m, Wt):
    """A filtered entry whose wide division gives m (for Wt = k * 2^16: S = m * k)."""
    assert Wt % 65536 == 0
    f = splat_film(1)
    k = Wt >> 16
    f["r"], f["g"], f["b"], f["weight"] = m[0] * k, m[1] * k, m[2] * k, Wt
    return f


def bin_film(bins, splat=False):
    """A film whose pixel i lands in bins[i] (>= 1; 0 for black; -1 for a pixel without samples): grey entries of one sample."""
    f = splat_film(len(bins)) if splat else linear_film(len(bins))
    for i, b in enumerate(bins):
        if b < 0:
            f["r"][i], f["g"][i], f["b"][i] = 5, 6, 7   # sums without samples are not metered
            continue
        Y = 0 if b == 0 else ((8 + (b - 1) % 8) << ((b - 1) // 8)) >> 3 if (b - 1) // 8 >= 3 else None
        if Y is None:   # e < 3: the luminances 1 .. 7
            e, sub = (b - 1) // 8, (b - 1) % 8
            Y = (8 + sub) >> (3 - e)
            assert model_bin_of_luminance(Y) == b, "no luminance has this bin"
        f["r"][i] = f["g"][i] = f["b"][i] = Y
        if splat:
            f["weight"][i] = 65536
        else:
            f["samples"][i] = 1
    return f


def largest_linear_rows():
    """Entries at the top of what ptss_accumulate_paths_linear can leave: every sample at 2^40 (bin 321), just below it (bin 320), and the rows of
    linear_common.high_film, whose sums no accumulate could have made (they saturate into the last bin or wrap)."""
    rows = [entry(1 << 40, 1 << 40, 1 << 40, 1), entry(7 << 40, 7 << 40, 7 << 40, 7), entry((1 << 40) - 256, 1 << 40, 1 << 40, 1),
            entry(((1 << 23) - 1) << 40, ((1 << 23) - 1) << 40, ((1 << 23) - 1) << 40, (1 << 23) - 1), entry(1 << 40, 0, 0, 1), entry(0, 0, 1 << 40, 3)]
    return np.concatenate(rows), high_film(3)


def largest_splat_rows():
    """S = 2^24 * Wt, the most the splat calls can leave (m = 2^40), for small, odd and large weights, and one unit below."""
    f = splat_film(6)
    for i, Wt in enumerate((1, 3, 65535, 65536, (1 << 38) + 1, (1 << 39) - 1)):
        f["r"][i] = f["g"][i] = f["b"][i] = Wt << 24
        f["weight"][i] = Wt
    g = f.copy()
    g["g"] -= 1
    return np.concatenate([f, g])


def adversarial_films():
    """(name, film, splat): films accumulated from linear_common's adversarial rows at three scales, and filtered films from splat_common's."""
    from linear_common import SCALES, adversarial_results, params_of
    from splat_common import resolve_rows as splat_resolve_rows
    from linear_common import resolve_rows as linear_resolve_rows
    out = []
    g = np.random.default_rng(11)
    for scale_log2, clamp_max in SCALES[:3]:
        params = params_of(scale_log2, clamp_max)
        rows = adversarial_results(params)
        film, _ = ptss.probe_accumulate_linear(rows, linear_film(90), index=g.integers(0, 80, len(rows)).astype(np.uint32), params=params)
        out.append((("accumulated", scale_log2), film, False))
        out.append((("resolve rows", scale_log2), linear_resolve_rows(params), False))
        out.append((("splat resolve rows", scale_log2), splat_resolve_rows(params), True))
    return out


def exposure_histograms():
    """(name, histogram): the histograms the exposure is tried on."""
    z = lambda: np.zeros(BINS, dtype=np.uint32)
    out = [("empty", z())]
    h = z(); h[0] = 12345; out.append(("all black", h))
    h = z(); h[1 + 8 * 20 + 3] = 777; out.append(("one bin", h))
    h = z(); h[0] = 9; h[5] = 1000; h[300] = 333; out.append(("two far bins", h))
    h = z(); h[17] = 1; out.append(("one pixel", h))
    h = z(); h[200] = 2 ** 32 - 1; h[0] = 2 ** 32 - 1; out.append(("a bin of 2^32 - 1", h))
    h = z(); h[1:] = 2 ** 32 - 1; out.append(("every bin full", h))
    h = z(); h[1] = 50; out.append(("the lowest bin", h))
    h = z(); h[321] = 50; out.append(("the highest bin of a film", h))
    g = np.random.default_rng(2)
    h = z(); h[100:260] = g.integers(0, 5000, 160); h[0] = 40; out.append(("a spread", h))
    return out


def state_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
