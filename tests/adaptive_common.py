"""Models and cases shared by tests/test_adaptive_cpu.py and tests/test_gpu_adaptive.py (ptss_accumulate_paths_stats / ptss_plan_samples;
DESIGN.md §3.28): the weight of a pixel in Python integers and numpy float32 — independent of csrc/ptadaptive.h — and the films the
plan is tried on."""
import numpy as np

import ptss

SCAN_TILE = 2048          # pixels per workgroup of the device's scan (csrc/ptadaptive.h kScanTile)
UNSAMPLED = 1 << 19
MASK = (1 << 64) - 1


def f32_of_int(x):
    """The float32 nearest to the non-negative integer x, ties to even, without passing through a double."""
    b = x.bit_length()
    if b <= 24:
        return np.float32(x)
    s = b - 24
    q, rem, half = x >> s, x & ((1 << s) - 1), 1 << (s - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return np.float32(q) * np.float32(2.0 ** s)   # q <= 2^24 times a power of two: exact


def standard_error(r, g, b, N, Q):
    """se of the issue: D in wrapping 64-bit integers, the rest in float32 (numpy's sqrt, division and product are correctly rounded)."""
    A = (N * Q) & MASK
    B = (r * r + g * g + b * b) & MASK
    D = A - B if A >= B else 0
    fn = np.float32(N)
    return np.sqrt(f32_of_int(D)) / (fn * np.sqrt(fn))


def model_weight(r, g, b, N, Q, params):
    if N < params.minSamples:
        return UNSAMPLED
    if N >= params.maxSamples:
        return 0
    se = standard_error(r, g, b, N, Q)
    if not se > np.float32(params.threshold):
        return 0
    return int(min(se * np.float32(1024), np.float32(524287)))


def model_weights(film, moments, params):
    f = np.ascontiguousarray(film).view(np.uint32).reshape(-1, 4)
    return [model_weight(int(e[0]), int(e[1]), int(e[2]), int(e[3]), int(q), params) for e, q in zip(f, moments)]


def check_plan(film, moments, n, params, cdf, index, info):
    """The plan (cdf, index, info) against the model's weights and the three properties of the issue, in Python integers."""
    w = model_weights(film, moments, params)
    P, total = len(w), sum(w)
    assert [int(c) for c in cdf] == list(np.cumsum(np.array(w, dtype=object))), "cdf"
    f = np.ascontiguousarray(film).view(np.uint32).reshape(-1, 4)
    want = dict(totalWeight=total, activePixels=sum(1 for v in w if v > 0), unsampledPixels=int((f[:, 3] < params.minSamples).sum()),
                cappedPixels=int((f[:, 3] >= params.maxSamples).sum()), uniform=int(total == 0))
    assert info == want, (info, want)
    assert len(index) == n
    idx = index.astype(np.int64)
    assert (np.diff(idx) >= 0).all() and (n == 0 or (0 <= idx[0] and idx[-1] < P)), "non-decreasing, inside the film"
    count = np.bincount(idx, minlength=P)
    if total == 0:
        assert [int(v) for v in idx] == [(i * P + P // 2) // n for i in range(n)], "uniform fallback"
        return
    for p in range(P):
        assert abs(int(count[p]) * total - n * w[p]) < total, (p, int(count[p]), w[p], total, n)
        assert w[p] > 0 or count[p] == 0, p


def film_of(samples, g, spread=1.0):
    """A consistent film and its moments: pixel p holds samples[p] random byte triples around a random mean, `spread` scaling the noise
    (0: every sample equal, so D = 0)."""
    P = len(samples)
    film, moments = np.zeros(P, dtype=ptss.FILM_DTYPE), np.zeros(P, dtype=np.uint64)
    for p, N in enumerate(samples):
        mean, dev = g.uniform(0, 255, 3), g.uniform(0, 60) * spread
        q = np.clip(np.rint(mean + dev * g.standard_normal((int(N), 3))), 0, 255).astype(np.int64)
        film["r"][p], film["g"][p], film["b"][p] = q.sum(axis=0) if N else (0, 0, 0)
        film["samples"][p] = N
        moments[p] = int((q * q).sum())
    return film, moments


def random_bytes_film(P, g):
    """Random bytes as film and moments: inputs that do not belong together (the arithmetic wraps; both sides must still agree)."""
    film = g.integers(0, 2 ** 32, (P, 4), dtype=np.uint64).astype(np.uint32)
    film[::3, 3] = g.integers(0, 64, len(film[::3]))   # a third with sample counts a plan may meet
    moments = g.integers(0, 2 ** 63, P, dtype=np.uint64) * np.uint64(2) + g.integers(0, 2, P, dtype=np.uint64)
    return film.view(ptss.FILM_DTYPE).reshape(-1), moments
