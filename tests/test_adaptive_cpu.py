"""Adaptive film sampling without a GPU (ptss_accumulate_paths_stats / ptss_plan_samples): the record layouts against the
header, the exported symbols, the host build of csrc/ptadaptive.h (the specification of the device's plan) against a model in Python
integers and numpy float32, the targets against Python integers, the three properties a plan keeps, the fallback, and the host
accumulation with moments against ptss_probe_accumulate and the oracle's tone map."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import ptss
import ptss_types
from adaptive_common import UNSAMPLED, check_plan, f32_of_int, film_of, model_weight, random_bytes_film, standard_error
from film_common import adversarial_radiance, results_of, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_structs_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes mirrors."""
    pf = ("structSize", "minSamples", "maxSamples", "threshold")
    nf = ("totalWeight", "activePixels", "unsampledPixels", "cappedPixels", "uniform", "reserved")
    body = "".join('printf("%%zu\\n", offsetof(ptss_plan_params, %s));' % f for f in pf)
    body += "".join('printf("%%zu\\n", offsetof(ptss_plan_info, %s));' % f for f in nf)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { printf("%zu\\n%zu\\n", sizeof(ptss_plan_params), '
                   'sizeof(ptss_plan_info)); ' + body + ' return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Pp, Pi = ptss_types.PlanParams, ptss_types.PlanInfo
    assert got[:2] == [C.sizeof(Pp), C.sizeof(Pi)] == [16, 32]
    assert got[2:6] == [getattr(Pp, f).offset for f in pf] == [0, 4, 8, 12]
    assert got[6:] == [getattr(Pi, f).offset for f in nf] == [0, 8, 12, 16, 20, 24]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_libraries_export_the_symbols():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_accumulate_paths_stats", "ptss_default_plan_params", "ptss_plan_cdf_entries", "ptss_plan_samples", "ptss_adaptive_launches"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_accumulate_stats", "ptss_probe_plan_samples"):
        assert hasattr(ptss.host_lib(), name), name
    assert L.ptss_version() == 300
    p = ptss_types.PlanParams()
    assert L.ptss_default_plan_params(C.byref(p)) == 0 and L.ptss_default_plan_params(None) == -1
    assert (p.structSize, p.minSamples, p.maxSamples, p.threshold) == (16, 8, 1 << 23, 0.5)
    d = ptss.plan_params()
    assert bytes(d) == bytes(p)
    entries = C.c_size_t()
    for P in (1, 2048, 2049, 1920 * 1080, 2 ** 31 - 1):
        assert L.ptss_plan_cdf_entries(P, C.byref(entries)) == 0 and entries.value >= P and ptss.plan_cdf_entries(P) == entries.value
    assert L.ptss_plan_cdf_entries(0, C.byref(entries)) == -5 and L.ptss_plan_cdf_entries(2 ** 31, C.byref(entries)) == -5
    assert L.ptss_plan_cdf_entries(16, None) == -1
    # refused before anything touches a device
    assert L.ptss_accumulate_paths_stats(None, None, None, 0, 0, None, None, 16, None, None, None) == -1
    assert L.ptss_plan_samples(None, None, None, 16, C.byref(p), 0, None, None, None, None) == -1
    assert L.ptss_adaptive_launches(None, (C.c_ulonglong * 2)()) == -1


def weight(r, g, b, N, Q, params):
    e = ptss_types.FilmEntry(r, g, b, N)
    return int(ptss.host_lib().ptss_probe_plan_weight(C.byref(e), Q, C.byref(params)))


def test_int_to_float_model():
    for x in (0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 53 + 1, 2 ** 63 + 2 ** 39, 2 ** 63 + 2 ** 39 + 1,
              2 ** 64 - 1, 3 * 2 ** 40 + 2 ** 16, 3 * 2 ** 40 + 2 ** 16 + 1):
        f = f32_of_int(x)
        lo, hi = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(np.inf))
        assert abs(int(f) - x) <= abs(int(lo) - x) and abs(int(f) - x) <= abs(int(hi) - x), x
        if abs(int(f) - x) == abs(int(lo) - x) or abs(int(f) - x) == abs(int(hi) - x):   # a tie: the even one
            assert (int(f.view(np.uint32)) & 1) == 0 or int(f) == x, x


def test_weights_equal_the_model():
    g = np.random.default_rng(1)
    params = ptss.plan_params(min_samples=8, max_samples=1000, threshold=0.5)
    # N around minSamples and maxSamples
    film, moments = film_of([0, 1, 7, 8, 9, 998, 999, 1000, 1001, 5000], g)
    for e, Q in zip(words(film), moments):
        r, gg, b, N = (int(v) for v in e)
        want = model_weight(r, gg, b, N, int(Q), params)
        assert weight(r, gg, b, N, int(Q), params) == want, (N, want)
        assert (want == UNSAMPLED) == (N < 8) and (N < 1000 or want == 0)
    # D = 0: every sample equal — converged whatever the threshold, also 0
    for thr in (0.0, 0.5):
        p = ptss.plan_params(threshold=thr)
        for N, q in ((8, 0), (8, 255), (100, 17), (2 ** 23 - 1, 255)):
            assert weight(q * N, q * N, q * N, N, 3 * q * q * N, p) == model_weight(q * N, q * N, q * N, N, 3 * q * q * N, p) == 0
    # se one ulp either side of the threshold
    for N, half in ((16, 1), (64, 3), (1000, 40), (100000, 2)):   # N samples, half at q - half and half at q + half in one channel
        q = 100
        r, Q = q * N, (N // 2) * ((q - half) ** 2 + (q + half) ** 2)
        se = standard_error(r, 0, 0, N, Q)
        assert se > 0
        below, above = np.nextafter(se, np.float32(0)), np.nextafter(se, np.float32(np.inf))
        for thr, live in ((below, True), (se, False), (above, False)):
            p = ptss.plan_params(threshold=float(thr))
            got = weight(r, 0, 0, N, Q, p)
            assert got == model_weight(r, 0, 0, N, Q, p) and (got > 0) == live, (N, half, float(thr))
    # the cap: se * 1024 beyond 2^19 - 1 (inconsistent inputs reach it; consistent ones stay below 128 * 1024)
    p = ptss.plan_params(threshold=0.0)
    assert weight(0, 0, 0, 8, 2 ** 40, p) == model_weight(0, 0, 0, 8, 2 ** 40, p) == 524287
    assert weight(0, 0, 0, 8, 2 ** 63, p) == 0   # 8 * 2^63 wraps to 0: D = 0
    assert weight(255 * 4, 0, 0, 8, 4 * 255 * 255, p) == model_weight(255 * 4, 0, 0, 8, 4 * 255 * 255, p) < 128 * 1024
    # random consistent films, and random bytes that do not belong together
    film, moments = film_of(g.integers(8, 200, 300), g)
    rf, rm = random_bytes_film(600, g)
    for f, m, pp in ((film, moments, params), (rf, rm, ptss.plan_params(min_samples=3, max_samples=1 << 23, threshold=0.25))):
        for e, Q in zip(words(f), m):
            r, gg, b, N = (int(v) for v in e)
            got = weight(r, gg, b, N, int(Q), pp)
            assert got == model_weight(r, gg, b, N, int(Q), pp) and got <= UNSAMPLED, (r, gg, b, N, int(Q))


def test_targets_equal_python_integers():
    g = np.random.default_rng(2)
    T = ptss.host_lib().ptss_probe_plan_target
    cases = [(1, 1), (1, 2 ** 31 - 1), (2 ** 50, 1), (2 ** 50, 2 ** 31 - 1), (2 ** 50 - 1, 2 ** 31 - 2), (7, 3), (3, 7), (2 ** 19, 4 * 1920 * 1080)]
    cases += [(int(g.integers(1, 2 ** 50, endpoint=True)), int(g.integers(1, 2 ** 31))) for _ in range(200)]
    for total, n in cases:
        for i in {0, 1, n // 2, n - 2, n - 1} | {int(v) for v in g.integers(0, n, 5)}:
            if 0 <= i < n:
                want = (i * total + total // 2) // n
                assert T(i, n, total) == want and want < total, (i, n, total)


@pytest.mark.parametrize("seed", range(6))
def test_plan_properties_on_random_films(seed):
    g = np.random.default_rng(100 + seed)
    P = int((1, 2, 37, 700, 2049, 5000)[seed])
    params = ptss.plan_params(min_samples=4, max_samples=40, threshold=float(g.uniform(0.2, 3.0)))
    film, moments = film_of(g.integers(0, 48, P), g, spread=float(g.uniform(0, 1)))
    for n in (1, 63, P, 4 * P + 3):
        cdf, index, info = ptss.probe_plan_samples(film, moments, n, params)
        check_plan(film, moments, n, params, cdf, index, info)
    rf, rm = random_bytes_film(P, g)
    cdf, index, info = ptss.probe_plan_samples(rf, rm, 2 * P + 1, params)
    check_plan(rf, rm, 2 * P + 1, params, cdf, index, info)


def test_fallback_when_nothing_is_left():
    g = np.random.default_rng(3)
    params = ptss.plan_params(min_samples=4, max_samples=40, threshold=1.0)
    for P in (1, 5, 640):
        capped, _ = film_of(np.full(P, 40), g)                    # every pixel at maxSamples
        flat, fm = film_of(np.full(P, 10), g, spread=0.0)         # every pixel converged (D = 0)
        for film, moments in ((capped, np.zeros(P, np.uint64)), (flat, fm)):
            for n in (1, P - 1, P, 3 * P + 1):
                if n == 0:
                    continue
                cdf, index, info = ptss.probe_plan_samples(film, moments, n, params)
                assert info["uniform"] == 1 and info["totalWeight"] == 0 and info["activePixels"] == 0 and not cdf.any()
                check_plan(film, moments, n, params, cdf, index, info)
                if n == P:
                    assert np.array_equal(index, np.arange(P))
    # refusals of the probe: the device call's, alignment aside
    film, moments = film_of([5, 5], g)
    for bad in (dict(min_samples=0), dict(max_samples=0), dict(max_samples=(1 << 23) + 1), dict(min_samples=9, max_samples=8), dict(threshold=-0.5),
                dict(threshold=float("inf")), dict(threshold=float("nan"))):
        with pytest.raises(ptss.PtssError):
            ptss.probe_plan_samples(film, moments, 4, ptss.plan_params(**bad))
    wrong = ptss.plan_params()
    wrong.structSize = 12
    with pytest.raises(ptss.PtssError):
        ptss.probe_plan_samples(film, moments, 4, wrong)


def test_probe_accumulate_stats_against_probe_accumulate_and_the_oracle():
    rad = adversarial_radiance()
    n, P = len(rad), 97
    res = results_of(rad)
    q = np.array([[oracle.probe_quantize(float(v)) for v in row] for row in rad], dtype=np.uint64)
    sq = (q * q).sum(axis=1)
    g = np.random.default_rng(2)
    maps = {"all on one pixel": np.full(n, 5, np.uint32), "many to few": g.integers(0, 7, n).astype(np.uint32), "sorted": np.sort(g.integers(0, P, n)).astype(np.uint32),
            "with entries beyond the film": np.where(np.arange(n) % 10 == 3, P + np.arange(n), g.integers(0, P, n)).astype(np.uint32)}
    start = np.zeros(P, dtype=ptss.FILM_DTYPE)
    start["r"], start["g"], start["b"], start["samples"] = 1000, 2000, 3000, 40
    m0 = g.integers(0, 2 ** 40, P).astype(np.uint64)
    px0, hs0 = np.full((P, 4), 9, np.uint8), np.full((P, 4), -2.0, np.float32)
    for what, index in maps.items():
        film, moments, pixels, history, rejected = ptss.probe_accumulate_stats(res, start, m0, index=index, pixels=px0, history=hs0)
        want, want_px, want_hs, want_rej = ptss.probe_accumulate(res, start, index=index, pixels=px0, history=hs0)
        assert np.array_equal(words(film), words(want)) and np.array_equal(pixels, want_px) and rejected == want_rej, what
        assert words(history).tobytes() == words(want_hs).tobytes(), what
        m = m0.copy()
        keep = index < P
        np.add.at(m, index[keep], sq[keep])
        assert np.array_equal(moments, m), what
    # without an index, from a first pixel > 0, NULL outputs
    film, moments, pixels, history, rejected = ptss.probe_accumulate_stats(res[:60], start, m0, first_pixel=30)
    want, _, _, _ = ptss.probe_accumulate(res[:60], start, first_pixel=30)
    m = m0.copy()
    m[30:90] += sq[:60]
    assert np.array_equal(words(film), words(want)) and np.array_equal(moments, m) and pixels is None and history is None and rejected == 0
    with pytest.raises(ptss.PtssError):
        ptss.probe_accumulate_stats(res[:60], start, m0, first_pixel=40)   # leaves the film
