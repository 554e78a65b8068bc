"""The meter of the two linear films without a GPU (ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure and the metered resolves;
DESIGN.md §3.31): the record layouts against the header, the exported symbols and the defaults, and the host build of csrc/ptmeter.h (the
specification of the device's histogram and exposure) against the model of tests/meter_common.py: the bin of a pixel at every power of
two and its neighbours, the largest rows of both films, histograms on sub-ranges and carried across calls, the exposure on histograms
that corner the percentile cuts, the clamps and the adaptation, and the properties the design rests on — order freedom and the shift of
a doubled film."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from linear_common import SCALES, high_film, linear_film, params_of
from meter_common import (BINS, LAST, adversarial_films, bin_film, exposure_histograms, largest_linear_rows, largest_splat_rows,
                          linear_entry_of_means, luminance_values, means_for, model_bin, model_bin_of_luminance, model_exposure,
                          model_histogram, model_luminance, new_state, splat_entry_of_means, state_equal)
from splat_common import high_film as high_splat_film
from splat_common import splat_film

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")


def test_structs_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes mirrors and the numpy record."""
    fields = (("ptss_meter_params", ("structSize", "key", "lowPermille", "highPermille", "rate", "minExposure", "maxExposure", "reserved")),
              ("ptss_meter_state", ("exposure", "target", "meanLog2", "updates", "metered", "black", "counted", "sumLog")))
    body = "".join('printf("%%zu\\n", sizeof(%s));' % s for s, _ in fields)
    body += "".join('printf("%%zu\\n", offsetof(%s, %s));' % (s, f) for s, fs in fields for f in fs)
    body += 'printf("%d %zu\\n", PTSS_METER_BINS, _Alignof(ptss_meter_state));'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { ' + body + ' return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Par, Sta = ptss_types.MeterParams, ptss_types.MeterState
    assert got[:2] == [C.sizeof(Par), C.sizeof(Sta)] == [32, 48] and ptss.METER_STATE_DTYPE.itemsize == 48
    assert got[2:10] == [getattr(Par, f).offset for f in fields[0][1]] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert got[10:18] == [getattr(Sta, f).offset for f in fields[1][1]] == [ptss.METER_STATE_DTYPE.fields[f][1] for f in fields[1][1]]
    assert got[10:18] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert got[18:] == [ptss.METER_BINS, 8] == [BINS, 8]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed
    header = open(os.path.join(CSRC, "ptmeter.h")).read()   # the launch shape the GPU tests size their largest film by
    assert int(re.search(r"kBlock = (\d+);", header).group(1)) == ptss_types.METER_BLOCK
    assert int(re.search(r"kGridCap = (\d+);", header).group(1)) == ptss_types.METER_GRID_CAP


def test_libraries_export_the_symbols_and_the_defaults():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_meter_params", "ptss_meter_linear", "ptss_meter_splat", "ptss_meter_exposure", "ptss_resolve_linear_metered",
                 "ptss_resolve_splat_metered", "ptss_meter_launches"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_meter_bin", "ptss_probe_meter_linear", "ptss_probe_meter_splat", "ptss_probe_meter_exposure"):
        assert hasattr(ptss.host_lib(), name), name
    assert L.ptss_version() == 300
    m = ptss_types.MeterParams()
    assert L.ptss_default_meter_params(C.byref(m)) == 0 and L.ptss_default_meter_params(None) == -1
    assert (m.structSize, m.key, m.lowPermille, m.highPermille, m.rate, m.minExposure, m.maxExposure, m.reserved) == \
        (32, float(np.float32(0.18)), 100, 20, 1.0, 2.0 ** -16, 2.0 ** 16, 0)
    assert bytes(ptss.meter_params()) == bytes(m)
    # refused before anything touches a device
    p = ptss.linear_params()
    assert L.ptss_meter_linear(None, None, 0, 0, None, None) == -1 and L.ptss_meter_splat(None, None, 0, 0, None, None) == -1
    assert L.ptss_meter_exposure(None, None, C.byref(p), C.byref(m), None, None) == -1
    assert L.ptss_resolve_linear_metered(None, None, 0, 0, C.byref(p), None, None, None, None, None) == -1
    assert L.ptss_resolve_splat_metered(None, None, 0, 0, C.byref(p), None, None, None, None, None) == -1
    assert L.ptss_meter_launches(None, (C.c_ulonglong * 3)()) == -1


def test_the_probes_refuse_what_the_calls_refuse():
    H = ptss.host_lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    film, spl, h, state = linear_film(12), splat_film(12), np.zeros(BINS, np.uint32), new_state()
    for probe, f in ((H.ptss_probe_meter_linear, film), (H.ptss_probe_meter_splat, spl)):
        assert probe(vp(f), 0, 12, vp(h)) == 0 and probe(vp(f), 3, 0, vp(h)) == 0 and probe(None, 0, 0, None) == 0
        assert probe(None, 0, 12, vp(h)) != 0 and probe(vp(f), 0, 12, None) != 0
        for first, count in ((0, 2 ** 31), (2 ** 31, 1), (2 ** 31 - 1, 1), (2 ** 30, 2 ** 30), (2 ** 63, 2 ** 63)):
            assert probe(vp(f), first, count, vp(h)) != 0, (first, count)
    assert not h.any()   # twelve pixels without samples: nothing metered
    b = C.c_int(7)
    words = np.zeros(4, np.uint64)
    assert H.ptss_probe_meter_bin(None, 0, C.byref(b), None) != 0 and H.ptss_probe_meter_bin(vp(words), 0, None, None) != 0
    assert H.ptss_probe_meter_bin(vp(words), 0, C.byref(b), None) == 0 and b.value == -1
    exp = lambda params, meter, hist=h, st=state: H.ptss_probe_meter_exposure(vp(hist), ref(params), ref(meter), vp(st))
    good, lin = ptss.meter_params(), ptss.linear_params()
    assert exp(lin, good) == 0 and exp(None, good) != 0 and exp(lin, None) != 0 and exp(lin, good, hist=None) != 0 and exp(lin, good, st=None) != 0
    nan, inf = float("nan"), float("inf")
    for change in (dict(structSize=28), dict(structSize=0), dict(key=0.0), dict(key=-0.18), dict(key=nan), dict(key=inf), dict(lowPermille=1000),
                   dict(highPermille=1000), dict(lowPermille=500, highPermille=500), dict(lowPermille=2 ** 32 - 1, highPermille=2),
                   dict(rate=-0.01), dict(rate=1.01), dict(rate=nan), dict(minExposure=-1.0), dict(minExposure=nan), dict(minExposure=inf),
                   dict(maxExposure=inf), dict(maxExposure=nan), dict(maxExposure=-1.0), dict(minExposure=2.0, maxExposure=1.0), dict(reserved=1)):
        meter = ptss.meter_params()
        for k, v in change.items():
            setattr(meter, k, v)
        assert exp(lin, meter) != 0, change
    for change in (dict(structSize=16), dict(scaleLog2=33), dict(clampMax=0.0), dict(exposure=-0.5), dict(reserved=1)):
        params = ptss.linear_params()
        for k, v in change.items():
            setattr(params, k, v)
        assert exp(params, good) != 0, change
    # the boundaries are allowed
    for meter in (ptss.meter_params(low_permille=999, high_permille=0), ptss.meter_params(low_permille=0, high_permille=999),
                  ptss.meter_params(rate=0.0), ptss.meter_params(min_exposure=0.0, max_exposure=0.0), ptss.meter_params(min_exposure=3.0, max_exposure=3.0)):
        assert exp(lin, meter) == 0
    assert int(state["updates"][0]) == 6   # the calls that were not refused, and only they, moved the state


def test_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/meter_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host build
    of csrc/ptmeter.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "meter_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "meter_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("meter_sanitize ok"), r.stdout + r.stderr


# ---- pixel -> bin ----------------------------------------------------------------------------------------------------------------------------------
def test_bins_at_every_power_of_two_and_around_it():
    seen = set()
    for Y in luminance_values():
        want = model_bin_of_luminance(Y)
        assert (want == 0) == (Y == 0) and want <= 321
        for m in means_for(Y):
            assert model_luminance(*m) == Y, (Y, m)
            for N in (1, 2, 7, 300):
                e = linear_entry_of_means(m, N)
                assert ptss.probe_meter_bin(e) == model_bin(e.view(np.uint64)) == (want, Y), (Y, m, N)
            for Wt in (65536, 3 * 65536, 300 * 65536):
                e = splat_entry_of_means(m, Wt)
                assert ptss.probe_meter_bin(e, splat=True) == model_bin(e.view(np.uint64), True) == (want, Y), (Y, m, Wt)
        seen.add(want)
    assert {0, 1, 9, 13, 17, 19, 23, 25, 26, 321} <= seen and len(seen) >= 80   # Y = 0, 1, 2, 3, 4, 5, 7, 8, 9 and 2^40
    # the shape of a bin: an eighth of an octave, linear in the mantissa
    for e in range(3, 41):
        for sub in range(8):
            lo = (8 + sub) << (e - 3)
            assert model_bin_of_luminance(lo) == 1 + 8 * e + sub and (lo == 1 << 40 or model_bin_of_luminance(lo + (1 << (e - 3)) - 1) == 1 + 8 * e + sub)
            if lo == 1 << 40:
                break
    # pixels that are not metered, whatever their sums
    for words, splat in (((0, 0, 0, 0), False), ((5, 6, 7, 0), False), ((5, 6, 7, 3 << 32), False), ((1 << 63, 1, 2, 0), True)):
        assert ptss.probe_meter_bin(np.array(words, np.uint64), splat) == model_bin(words, splat) == (-1, 0)
    # the odd weights of the wide division
    g = np.random.default_rng(4)
    for _ in range(300):
        Wt = int(g.integers(1, 1 << 39))
        words = [int(g.integers(0, (Wt << 24) + 1)) for _ in range(3)] + [Wt]
        assert ptss.probe_meter_bin(np.array(words, np.uint64), True) == model_bin(words, True)


def test_the_largest_rows_stay_inside_the_bound():
    rows, beyond = largest_linear_rows()
    bins = [ptss.probe_meter_bin(e)[0] for e in rows]
    assert bins == [model_bin(e)[0] for e in rows.view(np.uint64).reshape(-1, 4)]
    assert bins[:4] == [321, 321, 320, 321] and bins[4:] == [model_bin((1 << 40, 0, 0, 1))[0], model_bin((0, 0, 1 << 40, 3))[0]] and max(bins) == 321   # m = 2^40: the top of a film the library filled
    srows = largest_splat_rows()
    got = [ptss.probe_meter_bin(e, True) for e in srows]
    assert got == [model_bin(e, True) for e in srows.view(np.uint64).reshape(-1, 4)]
    assert [b for b, _ in got[:6]] == [321] * 6 and [y for _, y in got[:6]] == [1 << 40] * 6 and max(b for b, _ in got) == 321
    # sums no call of the library leaves (linear_common.high_film, splat_common.high_film) stay inside the histogram all the same
    for film, splat in ((beyond, False), (high_splat_film(3), True)):
        for e in film:
            b, Y = ptss.probe_meter_bin(e, splat)
            assert (b, Y) == model_bin(np.ascontiguousarray(e).view(np.uint64).reshape(-1), splat) and 0 <= b <= LAST
    assert ptss.probe_meter_bin(np.array([1 << 50, 1 << 50, 1 << 50, 1], np.uint64)) == (LAST, 1 << 50)   # e > 40 saturates
    assert ptss.probe_meter_bin(np.array([1 << 41, 1 << 41, 1 << 41, 1], np.uint64)) == (LAST, 1 << 41)
    h = ptss.probe_meter_linear(np.concatenate([rows, beyond]))
    assert np.array_equal(h, model_histogram(np.concatenate([rows, beyond]))) and h.sum() == len(rows) + len(beyond)


# ---- histograms -------------------------------------------------------------------------------------------------------------------------------------
def test_histograms_equal_the_model():
    for name, film, splat in adversarial_films():
        probe = ptss.probe_meter_splat if splat else ptss.probe_meter_linear
        P = len(film)
        whole = probe(film)
        assert np.array_equal(whole, model_histogram(film, splat)), name
        metered = int((film["weight"] != 0).sum()) if splat else int((film["samples"] != 0).sum())
        assert int(whole.sum()) == metered > 0, name
        first, count = P // 3, P // 2
        part = probe(film, first, count)
        assert np.array_equal(part, model_histogram(film, splat, first, count)), name
        # carried over two calls = one call over the union, on a histogram that was in use
        start = np.arange(BINS, dtype=np.uint32) * 3
        two = probe(film, first + count, P - first - count, histogram=probe(film, 0, first + count, histogram=start))
        assert np.array_equal(two, model_histogram(film, splat, histogram=start)) and np.array_equal(two - start, whole), name
        assert np.array_equal(probe(film, 5, 0, histogram=start), start), name   # count = 0
    wrap = np.full(BINS, 2 ** 32 - 1, np.uint32)   # counts wrap like any unsigned integer
    got = ptss.probe_meter_linear(bin_film([25, 25, 40, 0]), histogram=wrap)
    assert got[25] == 1 and got[40] == 0 and got[0] == 0 and got[41] == 2 ** 32 - 1


def test_a_histogram_is_the_same_for_every_order_and_every_split():
    g = np.random.default_rng(8)
    for name, film, splat in adversarial_films()[:3]:
        probe = ptss.probe_meter_splat if splat else ptss.probe_meter_linear
        whole = probe(film)
        for _ in range(3):
            shuffled = film[g.permutation(len(film))]
            assert np.array_equal(probe(shuffled), whole), name
            cuts = np.sort(g.integers(0, len(film) + 1, 3))
            h = None
            for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [len(film)]])):
                h = probe(shuffled, int(a), int(b - a), histogram=h)
            assert np.array_equal(h, whole), name


def test_a_film_doubled_moves_eight_bins_up_and_halves_the_exposure():
    g = np.random.default_rng(6)
    P = 400
    film = linear_film(P)
    film["samples"] = g.integers(1, 6, P)
    for c in "rgb":   # means of at least 2^10, so that doubling a sum doubles the luminance to within its own rounding
        film[c] = (g.integers(1 << 12, 1 << 30, P) * film["samples"]).astype(np.uint64)
    film["samples"][::17] = 0
    film["r"][::23] = film["g"][::23] = film["b"][::23] = 0
    twice = film.copy()
    for c in "rgb":
        twice[c] *= 2
    h1, h2 = ptss.probe_meter_linear(film), ptss.probe_meter_linear(twice)
    # a mean m doubles exactly (the sums are multiples of N), and (54, 183, 19) . 2m + 128 >> 8 is 2Y or 2Y - 1: at Y >= 2^10 the bin moves by
    # eight unless Y sat on a bin's lower edge; the model is the judge of those
    assert np.array_equal(h2, model_histogram(twice)) and h1[0] == h2[0] > 0 and h1[1:].sum() == h2[1:].sum()
    moved = np.zeros(BINS, np.int64)
    moved[9:] = h1[1:-8]
    assert np.abs(moved[1:].astype(np.int64) - h2[1:]).sum() <= 2 * int(h1[1:].sum()) // 64   # a bin is at least 128 wide here: edges are rare
    exact = film.copy()   # grey pixels whose luminance is the mean itself: every count moves by exactly eight bins
    exact["g"], exact["b"] = exact["r"], exact["r"]
    twice = exact.copy()
    for c in "rgb":
        twice[c] *= 2
    h1, h2 = ptss.probe_meter_linear(exact), ptss.probe_meter_linear(twice)
    assert np.array_equal(h2[9:], h1[1:-8]) and h2[0] == h1[0] and not h2[1:9].any()
    meter = ptss.meter_params(rate=1.0)
    s1, s2 = ptss.probe_meter_exposure(h1, meter=meter), ptss.probe_meter_exposure(h2, meter=meter)
    assert state_equal(s1, model_exposure(h1, new_state(), ptss.linear_params(), meter)) and int(s2["sumLog"][0]) == int(s1["sumLog"][0]) + 16 * int(s1["counted"][0])
    # the quotients lie in [16, 64), where half a unit in the last place is at most 1.9e-6, and each is rounded once; taking scaleLog2 off is exact
    assert float(s2["meanLog2"][0]) == pytest.approx(float(s1["meanLog2"][0]) + 1.0, abs=4e-6)
    # 4e-6 * ln 2 in the exponent, its product's rounding and two exp of at most 2 ulp each
    assert float(s2["exposure"][0]) == pytest.approx(float(s1["exposure"][0]) / 2, rel=1e-5)


# ---- histogram -> exposure -------------------------------------------------------------------------------------------------------------------------
METERS = {
    "defaults": dict(),
    "no cuts": dict(low_permille=0, high_permille=0),
    "cuts inside a bin": dict(low_permille=333, high_permille=333),
    "cuts of 999": dict(low_permille=500, high_permille=499),
    "low 999": dict(low_permille=999, high_permille=0),
    "high 999": dict(low_permille=0, high_permille=999),
    "a key": dict(key=0.5),
}


@pytest.mark.parametrize("scale_log2", [0, 20, 32])
def test_exposure_equals_the_model(scale_log2):
    params = params_of(scale_log2, dict(SCALES[:3])[scale_log2])
    for hname, h in exposure_histograms():
        for mname, kw in METERS.items():
            meter = ptss.meter_params(**kw)
            got = ptss.probe_meter_exposure(h, params=params, meter=meter)
            want = model_exposure(h, new_state(), params, meter)
            assert state_equal(got, want), (hname, mname, got, want)
            T = int(h[1:].astype(np.uint64).sum())
            assert int(got["metered"][0]) == T and int(got["black"][0]) == int(h[0]) and int(got["updates"][0]) == 1
            assert (int(got["counted"][0]) >= 1) == (T >= 1)
            if T == 0:
                assert float(got["exposure"][0]) == float(got["target"][0]) == 1.0 and int(got["sumLog"][0]) == 0


def test_the_percentile_cuts_fall_where_the_ranks_say():
    h = np.zeros(BINS, np.uint32)
    h[5], h[300] = 1000, 333   # T = 1333
    s = ptss.probe_meter_exposure(h, meter=ptss.meter_params(low_permille=333, high_permille=333))
    lo, hi = 1333 * 333 // 1000, 1333 - 1333 * 333 // 1000   # 443, 890: both inside bin 5
    assert (lo, hi) == (443, 890) and int(s["counted"][0]) == 447 and int(s["sumLog"][0]) == 447 * 9
    s = ptss.probe_meter_exposure(h, meter=ptss.meter_params(low_permille=700, high_permille=100))
    lo, hi = 933, 1333 - 133   # [933, 1200): 67 ranks of bin 5 and 200 of bin 300
    assert int(s["counted"][0]) == 267 and int(s["sumLog"][0]) == 67 * 9 + 200 * 599
    one = np.zeros(BINS, np.uint32)
    one[40] = 1   # one pixel: every pair of cuts that sums to 999 leaves it
    for low in (0, 1, 500, 998, 999):
        s = ptss.probe_meter_exposure(one, meter=ptss.meter_params(low_permille=low, high_permille=999 - low))
        assert int(s["counted"][0]) == 1 and int(s["sumLog"][0]) == 79, low
    full = np.zeros(BINS, np.uint32)
    full[200] = 2 ** 32 - 1
    s = ptss.probe_meter_exposure(full, meter=ptss.meter_params(low_permille=0, high_permille=0))
    assert int(s["counted"][0]) == 2 ** 32 - 1 and int(s["sumLog"][0]) == (2 ** 32 - 1) * 399


def test_targets_hit_both_clamps():
    params = ptss.linear_params()
    dark, bright = np.zeros(BINS, np.uint32), np.zeros(BINS, np.uint32)
    dark[1], bright[321] = 10, 10   # mean log2 of about -20 and +20 at scaleLog2 = 20
    for h, meter, at in ((dark, ptss.meter_params(), 65536.0), (bright, ptss.meter_params(), 2.0 ** -16),
                         (dark, ptss.meter_params(min_exposure=0.5, max_exposure=4.0), 4.0), (bright, ptss.meter_params(min_exposure=0.5, max_exposure=4.0), 0.5),
                         (dark, ptss.meter_params(min_exposure=0.0, max_exposure=0.0), 0.0)):
        s = ptss.probe_meter_exposure(h, params=params, meter=meter)
        assert state_equal(s, model_exposure(h, new_state(), params, meter)) and float(s["target"][0]) == float(s["exposure"][0]) == at
    # adaptation is clamped as well: a state above the bounds comes down to them at any rate
    state = new_state()
    state["exposure"], state["updates"] = 100.0, 3
    meter = ptss.meter_params(rate=0.0, min_exposure=0.5, max_exposure=4.0)
    s = ptss.probe_meter_exposure(dark, state, params, meter)
    assert state_equal(s, model_exposure(dark, state, params, meter)) and float(s["exposure"][0]) == 4.0 and int(s["updates"][0]) == 4


@pytest.mark.parametrize("rate", [0.25, 0.0, 1.0, 0.7])
def test_a_chain_of_updates_adapts_at_the_rate(rate):
    params = ptss.linear_params()
    meter = ptss.meter_params(rate=rate)
    hists = [h for _, h in exposure_histograms()]
    chain = [hists[9], hists[2], hists[0], hists[3], hists[1], hists[9]]   # the empty and the black ones keep the exposure
    got = want = new_state()
    exposures = []
    for k, h in enumerate(chain):
        got = ptss.probe_meter_exposure(h, got, params, meter)
        want = model_exposure(h, want, params, meter)
        assert state_equal(got, want), (rate, k, got, want)
        assert int(got["updates"][0]) == k + 1
        exposures.append(float(got["exposure"][0]))
    assert exposures[2] == exposures[1] and exposures[4] == exposures[3]
    if rate == 0.0:
        assert len(set(exposures)) == 1   # the first update's target, kept
    if rate == 1.0:
        s = ptss.probe_meter_exposure(chain[3], None, params, meter)
        assert exposures[3] == float(s["exposure"][0])   # no memory
    sat = new_state()
    sat["updates"], sat["exposure"] = 2 ** 32 - 1, 2.0
    s = ptss.probe_meter_exposure(chain[0], sat, params, meter)
    assert int(s["updates"][0]) == 2 ** 32 - 1 and state_equal(s, model_exposure(chain[0], sat, params, meter))   # saturating
