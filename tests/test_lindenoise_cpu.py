"""The denoiser of the two linear films without a GPU (ptss_denoise_linear, ptss_probe_denoise_linear): the record
layout against the header, the symbols and the defaults, every refusal of the probe, prepare and finish of the host build of
csrc/ptlindn.h (the specification of the device's film) against Python integers, the passes against a float64 restatement of the
formulas, the filter's exact properties, and that it denoises.

The float tolerance, reasoned (not measured on the code under test). The film is built so that a pixel's tolerance tol_p is at least
a hundredth of its luminance. A tap's exponent then carries: e_lum, whose numerator |l_q - l_p| is a difference of two float32
luminances of three roundings each, 6 * 2^-24 l / tol <= 3.6e-5; e_normal, 1 - n.n of three roundings over sigmaNormal = 0.1, 1.8e-6;
e_depth, a difference of depths of one rounding each over a tolerance of at least 1e-3 z, 1.2e-4 at the worst; and the relative
roundings of the sums and of exp's argument, 87.3 * 5 * 2^-24 = 2.6e-5 where the weight does not vanish. A weight is therefore within
2e-4 of the model's, relatively, and the normalised sum of tap differences within 2 * 2e-4 of the taps' spread, which is at most the
film's largest colour CMAX: ONE_PASS = 4e-4 * CMAX. Five passes add up: FIVE_PASSES = 5 * ONE_PASS. An integer mean may differ from
the model's rounding by one fixed-point step only where the model's value lies within that tolerance of a tie; with scaleLog2 = 6
(a step of 1/64) that is at most 2 * 4e-4 * 4 * 64 = 21 % of the entries after one pass and all of them after five, and the share that
did differ is asserted to stay below 2 % and 6 % (the seeds are chosen so that the host build stays inside)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptss
from lindenoise_common import (F32, case, corner_holes, first_difference, model_counts, model_entry, model_finish_means, model_fixed_mean,
                               model_means, model_pass, model_prepare, model_run, same_bytes, sampled_film, scene_features, truth_of, words)
from linear_common import linear_film, params_of
from linstats_common import conversion_rows, inconsistent_rows, moments_of_rows, random_word_moments, row_of_ys, zero_moments
from ptss_types import DenoiseLinearParams
from splat_common import splat_film

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
CMAX = 4.0
ONE_PASS = 4e-4 * CMAX
FIVE_PASSES = 5 * ONE_PASS
MODEL_PARAMS = params_of(6, 64.0)   # a coarse fixed point: a step is 1/64, so the float tolerance is a fraction of a step
SIZES = ((1, 1), (31, 7), (33, 9), (70, 37))


def changed(make, **kw):
    p = make()
    for k, v in kw.items():
        if k == "reserved" and isinstance(v, tuple):
            p.reserved[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p


DENOISE_REFUSED = [dict(structSize=28), dict(structSize=0), dict(levels=-1), dict(levels=7), dict(sigmaLuminance=0.0), dict(sigmaLuminance=-1.0),
                   dict(sigmaLuminance=float("inf")), dict(sigmaLuminance=float("nan")), dict(sigmaNormal=0.0), dict(sigmaNormal=float("nan")),
                   dict(sigmaDepth=0.0), dict(sigmaDepth=float("inf")), dict(reserved=(0, 1)), dict(reserved=(1, 1)), dict(reserved=(2, 7))]
FILM_REFUSED = [dict(structSize=16), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=float("inf")),
                dict(scaleLog2=32, clampMax=257.0), dict(exposure=-0.5), dict(exposure=float("nan")), dict(reserved=1)]
BAD_SIDES = ((0, 4), (4, 0), (-1, 4), (2 ** 22 + 1, 1), (1, 2 ** 22 + 1), (2 ** 22, 512), (46341, 46341))


# ---- layout, symbols, defaults ------------------------------------------------------------------------------------------------------------------
def test_the_mirror_matches_the_c_layout(tmp_path):
    names = ["structSize", "levels", "sigmaLuminance", "sigmaNormal", "sigmaDepth", "reserved"]
    prints = "".join(f'printf(" %zu", offsetof(ptss_denoise_linear_params, {n}));' for n in names)
    src = (f'#include <stdio.h>\n#include <stddef.h>\n#include "ptss.h"\n'
           f'int main(void){{printf("%zu %d %d %d", sizeof(ptss_denoise_linear_params), PTSS_VERSION, PTSS_FILM_LINEAR, PTSS_FILM_SPLAT); {prints} return 0;}}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(DenoiseLinearParams) == 32
    assert got[1] == 300 and got[2:4] == [ptss.FILM_LINEAR, ptss.FILM_SPLAT] == [ptss.GLARE_FILM_LINEAR, ptss.GLARE_FILM_SPLAT]
    assert got[4:] == [getattr(DenoiseLinearParams, n).offset for n in names] == [0, 4, 8, 12, 16, 20]


def test_symbols_and_defaults():
    dev, host = C.CDLL(ptss.DEVICE_LIB), C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_default_denoise_linear_params", "ptss_denoise_linear_workspace", "ptss_denoise_linear", "ptss_denoise_linear_launches",
                 "ptss_debug_denoise_linear_form"):
        assert hasattr(dev, name), name
    for name in ("ptss_probe_denoise_linear", "ptss_probe_denoise_linear_finish"):
        assert hasattr(host, name), name
    p = DenoiseLinearParams()
    dev.ptss_default_denoise_linear_params.argtypes = [C.POINTER(DenoiseLinearParams)]
    assert dev.ptss_default_denoise_linear_params(C.byref(p)) == 0 and dev.ptss_default_denoise_linear_params(None) == -1
    q = ptss.denoise_linear_params()
    assert bytes(p) == bytes(q) and p.structSize == 32 and p.levels == 5 and list(p.reserved) == [0, 0, 0]
    assert (p.sigmaLuminance, p.sigmaNormal, p.sigmaDepth) == (3.0, float(F32(0.1)), 4.0)
    n = C.c_size_t(0)
    dev.ptss_denoise_linear_workspace.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    assert dev.ptss_denoise_linear_workspace(70, 37, C.byref(n)) == 0 and n.value == ptss.denoise_linear_workspace(70, 37) == 70 * 37 * 52 + 8
    assert n.value % 16 == 0 and dev.ptss_denoise_linear_workspace(1, 1, C.byref(n)) == 0 and n.value == 64
    assert dev.ptss_denoise_linear_workspace(70, 37, None) == -1
    for w, h in BAD_SIDES:
        assert dev.ptss_denoise_linear_workspace(w, h, C.byref(n)) == -5, (w, h)
    assert ptss.DENOISE_MAX_LEVELS == 6


def test_every_refusal_of_the_probe():
    L = ptss.host_lib()
    w, h = 6, 5
    params, good = ptss.linear_params(), ptss.denoise_linear_params(levels=2)
    film, moments, features = case(w, h, params)
    out = np.zeros((w * h, 4), np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None

    def run(f=film, kind=0, width=w, height=h, m=moments, ft=features, p=params, d=good, o=out):
        return L.ptss_probe_denoise_linear(ptr(f), kind, width, height, ptr(m), ptr(ft), ref(p), ref(d), ptr(o), None)

    assert run() == 0 and run(kind=1) == 0
    before = out.copy()
    assert run(f=None) != 0 and run(m=None) != 0 and run(ft=None) != 0 and run(o=None) != 0 and run(p=None) != 0 and run(d=None) != 0
    assert run(o=words(film)) != 0   # out == film
    for kind in (2, -1, 77):
        assert run(kind=kind) != 0
    for change in DENOISE_REFUSED:
        assert run(d=changed(lambda: ptss.denoise_linear_params(levels=2), **change)) != 0, change
    for change in FILM_REFUSED:
        assert run(p=changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change)) != 0, change
    for width, height in BAD_SIDES:
        assert run(width=width, height=height) != 0, (width, height)
    assert np.array_equal(out, before)
    for levels in (0, 6):   # the ends of the range are taken
        assert run(d=ptss.denoise_linear_params(levels=levels, sigma_luminance=1e-30, sigma_normal=1e30, sigma_depth=1e-30)) == 0
    c3, o4 = (C.c_float * 3)(1, 2, 3), (C.c_ulonglong * 4)()
    finish = L.ptss_probe_denoise_linear_finish
    assert finish(c3, 4, 0, ref(params), o4) == 0
    assert finish(None, 4, 0, ref(params), o4) != 0 and finish(c3, 4, 0, None, o4) != 0 and finish(c3, 4, 0, ref(params), None) != 0
    assert finish(c3, 4, 2, ref(params), o4) != 0 and finish(c3, 4, 0, ref(changed(ptss.linear_params, reserved=1)), o4) != 0


# ---- prepare and finish, exactly ----------------------------------------------------------------------------------------------------------------
def flat_features(P):
    f = np.zeros(P, dtype=ptss.FEATURE_DTYPE)
    f["normal"][:, 2], f["depth"] = 1.0, 2.0
    return f


def prepared(film, moments, params, width=None):
    P = len(film)
    return ptss.probe_denoise_linear(film, width or P, 1 if width is None else P // width, moments, flat_features(P), params,
                                     ptss.denoise_linear_params(levels=0), plane=True)


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_prepare_and_levels_zero_against_python_integers(splat):
    """The means of both film kinds, se from the moments over N = 0, 1, 2, D = 0, both conversion paths of sqrt128 and rows no film holds,
    and the output rows of levels = 0."""
    from glare_common import film_of
    g = np.random.default_rng(11)
    for params in (params_of(20, 65536.0), params_of(0, 2.0 ** 40), params_of(32, 256.0)):
        rows = [r for _, r in conversion_rows()] + [r for _, r in inconsistent_rows()] + [row_of_ys([]), row_of_ys([7]), row_of_ys([7, 9]),
                                                                                           row_of_ys([5, 5]), [9, 9, 9, 0], [9, 9, 9, 1]]
        moments = np.concatenate([moments_of_rows(rows), random_word_moments(64, g)])
        P = len(moments)
        film = film_of(P, 1, splat, params, seed=3)
        out, plane = prepared(film, moments, params)
        want = model_prepare(film, moments, params)
        assert plane.tobytes() == want.tobytes(), [(p, plane[p], want[p]) for p in range(P) if plane[p].tobytes() != want[p].tobytes()][:3]
        assert np.isinf(plane[:, 3]).any() and (plane[:, 3] == 0).any() and (plane[:, 3] == -1).any() and (plane[:, 3] > 0).any()
        assert same_bytes(out, model_finish_means(film)), first_difference(out, model_finish_means(film))


def test_the_counts_of_a_filtered_film_and_the_clamped_count():
    params = ptss.linear_params()
    for w3 in (0, 1, 32767, 32768, 32769, 65535, 65536, 98303, 98304, 3 << 16, ((1 << 23) - 1) << 16, (((1 << 23) - 1) << 16) + 32767,
               (((1 << 23) - 1) << 16) + 32768, 1 << 39, 1 << 62, (1 << 64) - 1, (1 << 64) - 32768, (1 << 64) - 32769):
        got = ptss.probe_denoise_linear_finish((0.5, 0.25, 2.0), w3, "splat", params)
        if w3 == 0:
            assert got == (0, 0, 0, 0)
            continue
        K, clamped = model_counts(w3, True)
        assert 1 <= K <= (1 << 23) - 1 and clamped == 0
        assert list(got) == model_entry([1 << 19, 1 << 18, 1 << 21], w3, True), w3
    assert model_counts(32767, True)[0] == 1 and model_counts(98303, True)[0] == 1 and model_counts(98304, True)[0] == 2
    for samples, clamped in ((1, 0), (7, 3), ((1 << 23) - 1, 9), ((1 << 32) - 1, (1 << 32) - 1), (0, 5)):
        w3 = samples | (clamped << 32)
        got = ptss.probe_denoise_linear_finish((0.5, 0.25, 2.0), w3, "linear", params)
        assert list(got) == ([0, 0, 0, 0] if samples == 0 else model_entry([1 << 19, 1 << 18, 1 << 21], w3, False)), (samples, clamped)
        if samples:
            assert got[3] & 0xffffffff == samples and got[3] >> 32 == clamped


def test_the_finish_rounds_ties_to_even_and_clamps():
    for params in (params_of(6, 64.0), params_of(20, 3.0), params_of(0, 2.0 ** 40), params_of(32, 256.0)):
        one = 2.0 ** -params.scaleLog2
        cs = [0.0, -0.0, -1.0, float("nan"), float("-inf"), float("inf"), 0.5 * one, 1.5 * one, 2.5 * one, 3.5 * one, 0.49999997 * one, 0.50000006 * one,
              1.25 * one, 1000.5 * one, 1001.5 * one, 8388607.5 * one, 8388608.0 * one, 16777216.0 * one, params.clampMax, params.clampMax * 2,
              float(np.nextafter(F32(params.clampMax), F32(0))), 1e-40]
        for c in cs:
            got = ptss.probe_denoise_linear_finish((c, c, c), 3, "linear", params)
            c32 = float(F32(c))
            want = 0 if c32 != c32 else model_fixed_mean(c32, params)
            assert got[:3] == (3 * want,) * 3 and got[3] == 3, (params.scaleLog2, c, got, want)
    assert ptss.probe_denoise_linear_finish((0.5 / 64, 1.5 / 64, 2.5 / 64), 1, "linear", params_of(6, 64.0))[:3] == (0, 2, 2)


# ---- the passes against the float64 model -------------------------------------------------------------------------------------------------------
def check_against_model(width, height, levels, splat, seed, tolerance, share, single=True):
    params = MODEL_PARAMS
    denoise = ptss.denoise_linear_params(levels=levels)
    film, moments, features = case(width, height, params, seed=seed, splat=splat, noise=0.3, single=single)
    out, plane = ptss.probe_denoise_linear(film, width, height, moments, features, params, denoise, plane=True)
    want = model_run(film, moments, features, width, height, params, denoise)
    assert float(np.nanmax(want[:, :3])) <= CMAX
    empty = want[:, 3] < 0
    assert np.array_equal(plane[:, 3] < 0, empty) and (width * height < 16 or (empty.any() and np.isinf(want[:, 3]).any() == single))
    diff = np.abs(plane[~empty, :3].astype(np.float64) - want[~empty, :3])
    finite = np.isfinite(want[~empty, 3]) & (want[~empty, 3] > 0)
    assert np.array_equal(np.isfinite(plane[~empty, 3]), np.isfinite(want[~empty, 3]))
    vdiff = np.abs(plane[~empty, 3][finite].astype(np.float64) - want[~empty, 3][finite]) / want[~empty, 3][finite]
    worst, vworst = float(diff.max(initial=0.0)), float(vdiff.max(initial=0.0))
    print(f"{width} x {height}, {levels} levels, splat {splat}: largest |host - model| = {worst:.3g} of {tolerance:.3g}, variance relative {vworst:.3g}")
    assert worst <= tolerance and vworst <= 1e-3
    one = 1 << params.scaleLog2
    allowed = used = 0
    splat_words = words(film)
    for p, row in enumerate(words(out)):
        if empty[p]:
            assert not row.any(), p
            continue
        K, clamped = model_counts(int(splat_words[p, 3]), splat)
        assert int(row[3]) == K | (clamped << 32), p
        for ch in range(3):
            x = min(max(want[p, ch], 0.0), float(params.clampMax)) * one
            m = model_fixed_mean(want[p, ch], params)
            near_tie = abs(x - np.floor(x) - 0.5) <= tolerance * one
            got = int(row[ch]) // K
            assert int(row[ch]) == got * K
            allowed += near_tie
            if got != m:
                assert near_tie and abs(got - m) == 1, (p, ch, got, m, x)
                used += 1
    total = 3 * int((~empty).sum())
    print(f"    entries that may differ by one step {allowed} of {total}, that did {used}")
    assert used <= share * total


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_one_pass_equals_the_model(size, splat):
    check_against_model(size[0], size[1], 1, splat, 1, ONE_PASS, 0.02)


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_five_levels_equal_the_model(splat):
    check_against_model(70, 37, 5, splat, 2, FIVE_PASSES, 0.06, single=False)   # (an infinite variance spreads with every pass)


def test_every_level_of_the_model_by_itself():
    """Each spacing alone, from the same prepared plane: the probe's pass at level i is reached through levels = i + 1, so the model is
    fed the probe's own plane of levels = i (its float32 rows) and must land within one pass's tolerance."""
    params, (w, h) = MODEL_PARAMS, (70, 37)
    film, moments, features = case(w, h, params, seed=3)
    for i in range(6):
        src = ptss.probe_denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params(levels=i), plane=True)[1]
        got = ptss.probe_denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params(levels=i + 1), plane=True)[1]
        want = model_pass(src, features, w, h, 1 << i, params, ptss.denoise_linear_params())
        keep = want[:, 3] >= 0
        assert np.abs(got[keep, :3] - want[keep, :3]).max() <= ONE_PASS, i


# ---- properties -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_a_constant_film_stays_constant_exactly(splat):
    w, h = 37, 21
    params = ptss.linear_params()
    g = np.random.default_rng(5)
    features = scene_features(w, h, 1)
    film = splat_film(w * h) if splat else linear_film(w * h)
    N = g.integers(1, 9, w * h)
    mean = (123457, 998877, 5)
    for ch, m in zip("rgb", mean):
        film[ch] = m * N
    film["weight" if splat else "samples"] = N << 16 if splat else N
    for moments in (random_word_moments(w * h, g), zero_moments(w * h)):
        for levels in (1, 3, 6):
            out = ptss.probe_denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params(levels=levels))
            for ch, m in zip("rgb", mean):
                assert np.array_equal(out[ch], m * out["samples"].astype(np.uint64)), (levels, ch)
            assert np.array_equal(out["samples"], N)


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_levels_zero_leaves_the_resolve_the_meter_and_the_glare_unchanged(splat):
    from glare_common import film_of
    w, h = 37, 21
    params = params_of(20, 65536.0, exposure=0.75)
    film = film_of(w, h, splat, params, seed=4)   # adversarial means, the largest a library film holds, pixels without samples
    moments = random_word_moments(w * h, np.random.default_rng(2))
    out = ptss.probe_denoise_linear(film, w, h, moments, scene_features(w, h), params, ptss.denoise_linear_params(levels=0))
    resolve, meter = (ptss.probe_resolve_splat, ptss.probe_meter_splat) if splat else (ptss.probe_resolve_linear, ptss.probe_meter_linear)
    a, b = resolve(film, params=params), ptss.probe_resolve_linear(out, params=params)
    assert a[1].tobytes() == b[1].tobytes()
    for ch in "rgb" if splat else ("r", "g", "b", "weight"):   # (a filtered film's weight is a float, the output's a sample count)
        assert a[0][ch].tobytes() == b[0][ch].tobytes() and a[2][ch].tobytes() == b[2][ch].tobytes(), ch
    assert np.array_equal(meter(film), ptss.probe_meter_linear(out))
    glare = ptss.glare_params(levels=5, threshold=0.125)
    assert same_bytes(ptss.probe_glare_build(film, w, h, params, glare), ptss.probe_glare_build(out, w, h, params, glare))
    if not splat:
        full = film["samples"] != 0   # (an empty pixel's output row is all zero, whatever its clamped count was)
        assert same_bytes(out["samples"], film["samples"]) and same_bytes(out["clamped"][full], film["clamped"][full]) and not out["clamped"][~full].any()


def test_empty_pixels_stay_empty_and_never_leak():
    """The empty pixels hold enormous sums: were one read as a tap, its neighbours would show it."""
    w, h = 70, 37
    params = MODEL_PARAMS
    film, moments, features = case(w, h, params, seed=4)
    holes = corner_holes(w, h)
    loud = film.copy()
    for ch in "rgb":
        loud[ch][holes] = 1 << 45
    moments2 = moments.copy()
    moments2[holes] = random_word_moments(len(holes), np.random.default_rng(1))
    for levels in (1, 5):
        d = ptss.denoise_linear_params(levels=levels)
        a = ptss.probe_denoise_linear(film, w, h, moments, features, params, d)
        b = ptss.probe_denoise_linear(loud, w, h, moments2, features, params, d)
        assert same_bytes(a, b) and not words(a)[holes].any() and words(a)[[p for p in range(w * h) if p not in holes]][:, 3].all()


def test_a_material_boundary_is_never_crossed():
    w, h = 70, 37
    params = ptss.linear_params()
    features = scene_features(w, h, misses=True)
    features["normal"], features["depth"] = (0.0, 0.0, 1.0), 3.0   # only the material tells the regions apart (misses keep their index)
    mat = features["materialIdx"]
    film = linear_film(w * h)
    film["samples"] = 4
    value = {0: 4 * 900000, 1: 4 * 100000, -1: 4 * 100001}
    for ch in "rgb":
        film[ch] = [value[int(m)] for m in mat]
    out = ptss.probe_denoise_linear(film, w, h, random_word_moments(w * h, np.random.default_rng(3)), features, params,
                                    ptss.denoise_linear_params(levels=6, sigma_luminance=1e30))
    assert same_bytes(out, film)


def test_without_information_the_geometry_alone_filters():
    """All N = 1: v = inf everywhere, the luminance term vanishes — the result does not depend on sigmaLuminance and equals the float64
    model without that term."""
    w, h = 33, 9
    params = MODEL_PARAMS
    film, _, features = case(w, h, params, seed=6, holes=False)
    moments = moments_of_rows([[5, 25, 0, 1]] * (w * h))
    outs = [ptss.probe_denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params(levels=2, sigma_luminance=s), plane=True)
            for s in (1e-20, 3.0, 1e20)]
    assert same_bytes(outs[0][0], outs[1][0]) and same_bytes(outs[1][0], outs[2][0]) and np.isinf(outs[0][1][:, 3]).all()
    want = model_run(film, moments, features, w, h, params, ptss.denoise_linear_params(levels=2))
    assert np.abs(outs[1][1][:, :3] - want[:, :3]).max() <= 2 * ONE_PASS
    none = ptss.probe_denoise_linear(film, w, h, zero_moments(w * h), features, params, ptss.denoise_linear_params(levels=2))
    assert same_bytes(none, outs[1][0])       # N = 0 rows say as little as N = 1 rows
    sure = ptss.probe_denoise_linear(film, w, h, moments_of_rows([row_of_ys([5, 5])] * (w * h)), features, params, ptss.denoise_linear_params(levels=2))
    assert not same_bytes(sure, outs[1][0])   # a measured variance of 0 stops what infinity lets through


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_output_means_lie_within_the_hull_of_the_input_means(splat):
    w, h = 65, 17
    params = ptss.linear_params()
    film, moments, features = case(w, h, params, seed=8, splat=splat)
    means = np.array([m for m in model_means(film) if m is not None], dtype=np.float64)
    for levels in (1, 4):
        out = ptss.probe_denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params(levels=levels))
        got = np.array([m for m in model_means(out) if m is not None], dtype=np.float64)
        assert (got.min(axis=0) >= means.min(axis=0)).all() and (got.max(axis=0) <= means.max(axis=0)).all(), levels


def test_it_denoises_and_keeps_the_step():
    """Two regions of one material each around a luminance step, eight samples a pixel with a known relative noise, moments to match: the
    filtered film is closer to the truth than the unfiltered one, and the step keeps its height to within the filtered noise."""
    w, h = 64, 32
    params = ptss.linear_params()
    features = scene_features(w, h, misses=False)
    truth = truth_of(features, w, h)
    film, moments = sampled_film(truth, np.full(w * h, 8), params, seed=9, noise=0.4)
    out = ptss.probe_denoise_linear(film, w, h, moments, features, params, ptss.denoise_linear_params())
    scale = 2.0 ** -params.scaleLog2
    before = np.array(model_means(film), dtype=np.float64) * scale
    after = np.array(model_means(out), dtype=np.float64) * scale
    mse_before, mse_after = ((before - truth) ** 2).mean(), ((after - truth) ** 2).mean()
    left = np.ascontiguousarray(features)["materialIdx"] == 0
    step_truth = truth[left].mean(axis=0) - truth[~left].mean(axis=0)
    step_after = after[left].mean(axis=0) - after[~left].mean(axis=0)
    noise_after = np.sqrt(mse_after)
    print(f"mean squared error {mse_before:.3g} -> {mse_after:.3g} (ratio {mse_after / mse_before:.3g}); step {step_truth} -> {step_after}")
    assert mse_after < mse_before
    assert (np.abs(step_after - step_truth) <= noise_after).all()


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------------------
def test_the_probe_runs_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/lindenoise_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host
    build of csrc/ptlindn.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "lindenoise_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "lindenoise_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("lindenoise_sanitize ok"), r.stdout + r.stderr
