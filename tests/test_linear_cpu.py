"""The linear film without a GPU (ptss_accumulate_paths_linear / ptss_resolve_linear): the record layouts against the
header, the exported symbols and the defaults, and the host build of csrc/ptlinear.h (the specification of the device's film) against a
model in Python integers, exact fractions and numpy float32 (tests/linear_common.py): the fixed-point sample over the adversarial
rows, the resolve over the rows where an integer mean or its conversion rounds, the tone map of the mean against the oracle's, and order
freedom as a property."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from film_common import quant_thresholds, results_of
from linear_common import (SCALES, adversarial_results, down, entry, film_words, high_film, linear_film, model_accumulate, model_fixed, model_resolve,
                           params_of, resolve_rows, same_words, up)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_structs_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes mirrors and the numpy record."""
    ef = ("r", "g", "b", "samples", "clamped")
    pf = ("structSize", "scaleLog2", "clampMax", "exposure", "reserved")
    body = "".join('printf("%%zu\\n", offsetof(ptss_linear_entry, %s));' % f for f in ef)
    body += "".join('printf("%%zu\\n", offsetof(ptss_linear_params, %s));' % f for f in pf)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { printf("%zu\\n%zu\\n", sizeof(ptss_linear_entry), '
                   'sizeof(ptss_linear_params)); ' + body + ' return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    E, Pm = ptss_types.LinearEntry, ptss_types.LinearParams
    assert got[:2] == [C.sizeof(E), C.sizeof(Pm)] == [32, 20] and ptss.LINEAR_DTYPE.itemsize == 32
    assert got[2:7] == [getattr(E, f).offset for f in ef] == [ptss.LINEAR_DTYPE.fields[f][1] for f in ef] == [0, 8, 16, 24, 28]
    assert got[7:] == [getattr(Pm, f).offset for f in pf] == [0, 4, 8, 12, 16]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_libraries_export_the_symbols_and_the_defaults():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_linear_params", "ptss_accumulate_paths_linear", "ptss_resolve_linear", "ptss_linear_launches"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_accumulate_linear", "ptss_probe_resolve_linear"):
        assert hasattr(ptss.host_lib(), name), name
    assert L.ptss_version() == 300
    p = ptss_types.LinearParams()
    assert L.ptss_default_linear_params(C.byref(p)) == 0 and L.ptss_default_linear_params(None) == -1
    assert (p.structSize, p.scaleLog2, p.clampMax, p.exposure, p.reserved) == (20, 20, 65536.0, 1.0, 0)
    assert bytes(ptss.linear_params()) == bytes(p)
    # refused before anything touches a device
    assert L.ptss_accumulate_paths_linear(None, None, None, 0, 0, None, 16, C.byref(p), None) == -1
    assert L.ptss_resolve_linear(None, None, 0, 0, C.byref(p), None, None, None, None) == -1
    assert L.ptss_linear_launches(None, (C.c_ulonglong * 2)()) == -1


def test_the_probes_refuse_what_the_calls_refuse():
    H = ptss.host_lib()
    film, res = linear_film(4), results_of(np.zeros((4, 3), np.float32))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    acc = lambda params: H.ptss_probe_accumulate_linear(vp(res), None, 0, 4, vp(film), 4, C.byref(params) if params is not None else None, None)
    rsv = lambda params: H.ptss_probe_resolve_linear(vp(film), 0, 4, C.byref(params) if params is not None else None, None, None, None)
    assert acc(ptss.linear_params()) == 0 and rsv(ptss.linear_params()) == 0 and acc(None) != 0 and rsv(None) != 0
    for change in (dict(structSize=16), dict(structSize=0), dict(scaleLog2=-1), dict(scaleLog2=33), dict(clampMax=0.0), dict(clampMax=-1.0),
                   dict(clampMax=float("inf")), dict(clampMax=float("nan")), dict(clampMax=float(up(2.0 ** 20))), dict(scaleLog2=32, clampMax=257.0),
                   dict(scaleLog2=0, clampMax=float(up(2.0 ** 40))), dict(exposure=-0.5), dict(exposure=float("inf")), dict(exposure=float("nan")),
                   dict(reserved=1)):
        params = ptss.linear_params(clamp_max=2.0 ** 20)
        for k, v in change.items():
            setattr(params, k, v)
        assert acc(params) != 0 and rsv(params) != 0, change
    for s, cm in SCALES:   # the boundary is allowed
        assert acc(params_of(s, cm, exposure=0.0)) == 0 and rsv(params_of(s, cm, exposure=3e38)) == 0
    assert not film_words(film)[:, :3].any() and (film["samples"] == 1 + len(SCALES)).all()
    assert H.ptss_probe_accumulate_linear(vp(res), None, 2, 3, vp(film), 4, C.byref(ptss.linear_params()), None) != 0   # leaves the film


# ---- the fixed-point sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_log2, clamp_max", SCALES)
def test_probe_accumulate_equals_the_model_on_the_adversarial_rows(scale_log2, clamp_max):
    params = params_of(scale_log2, clamp_max)
    res = adversarial_results(params)
    M = len(res)
    g = np.random.default_rng(scale_log2)

    def check(what, rows, start, **kw):
        film, dropped = ptss.probe_accumulate_linear(rows, start, params=params, **kw)
        want, want_dropped = model_accumulate(rows, start, params, **kw)
        assert np.array_equal(film_words(film), want) and dropped == want_dropped, what
        return film

    film = check("identity map", res, linear_film(M))
    assert (film["samples"] == 1).all() and 0 < film["clamped"].sum() < M
    film = check("identity map from pixel 7", res[:40], linear_film(60), first_pixel=7)
    assert film["samples"].sum() == 40 and not film_words(film)[:7].any() and not film_words(film)[47:].any()
    check("a permuted index", res, linear_film(M), index=g.permutation(M).astype(np.uint32))
    film = check("300 rays on one pixel", res[:300], linear_film(9), index=np.full(300, 4, np.uint32))
    assert film["samples"][4] == 300 and film["samples"].sum() == 300
    wild = g.integers(0, 50, M).astype(np.uint32)
    wild[::7] = 50
    wild[3::11] = 2 ** 32 - 1
    check("entries beyond the film", res, linear_film(50), index=wild)
    assert ptss.probe_accumulate_linear(res, linear_film(50), index=wild, params=params)[1] == int((wild >= 50).sum()) > 0
    film = want = linear_film(M)   # a film carried over four calls, with and without an index
    for k in range(4):
        rows = res[g.permutation(M)]
        index = None if k % 2 == 0 else np.sort(g.integers(0, M, M)).astype(np.uint32)
        film, _ = ptss.probe_accumulate_linear(rows, film, index=index, params=params)
        want, _ = model_accumulate(rows, want, params, index=index)
        assert np.array_equal(film_words(film), want), k
    assert film["samples"].sum() == 4 * M


def test_single_values_round_as_stated():
    """The rule itself on the values the issue names, with the model's answers spelled out (scaleLog2 = 20: one unit is 2^-20)."""
    params = params_of(20, 65536.0)
    unit = 2.0 ** -20
    cases = ((np.nan, 0, 1), (np.inf, 1 << 36, 1), (-np.inf, 0, 0), (-0.0, 0, 0), (-3.0, 0, 0), (1e-45, 0, 0), (65536.0, 1 << 36, 0),
             (float(up(65536.0)), 1 << 36, 1), (float(down(65536.0)), (1 << 36) - (1 << 12), 0), (0.5 * unit, 0, 0), (1.5 * unit, 2, 0),
             (2.5 * unit, 2, 0), (3.5 * unit, 4, 0), (float(up(0.5 * unit)), 1, 0), (float(down(1.5 * unit)), 1, 0), (float(up(2.5 * unit)), 3, 0),
             (1.0, 1 << 20, 0), (40.0, 40 << 20, 0))
    for x, q, counted in cases:
        assert model_fixed(x, params) == (q, counted), x
        film, _ = ptss.probe_accumulate_linear(results_of(np.array([[x, 0.25, -1.0]], np.float32)), linear_film(1), params=params)
        assert (int(film["r"][0]), int(film["g"][0]), int(film["b"][0]), int(film["samples"][0]), int(film["clamped"][0])) == (q, 1 << 18, 0, 1, counted), x


@pytest.mark.parametrize("scale_log2, clamp_max", SCALES[:3])
def test_sums_from_2_to_the_62_take_2_to_the_40_per_sample(scale_log2, clamp_max):
    params = params_of(scale_log2, clamp_max)
    res = results_of(np.full((364, 3), clamp_max, np.float32))
    index = np.concatenate([np.full(64, 1), np.full(300, 3)]).astype(np.uint32)
    film, _ = ptss.probe_accumulate_linear(res, high_film(5), index=index, params=params)
    want, _ = model_accumulate(res, high_film(5), params, index=index)
    assert np.array_equal(film_words(film), want)
    assert int(film["r"][1]) == (1 << 62) + (64 << 40) and int(film["b"][3]) == (1 << 62) + (300 << 40) and int(film["g"][0]) == 1 << 62
    assert list(film["samples"]) == [5, 69, 5, 305, 5] and (film["clamped"] == 1).all()


# ---- the resolve -------------------------------------------------------------------------------------------------------------------------------
def check_resolve(film, params, what):
    linear, pixels, history = ptss.probe_resolve_linear(film, params=params)
    want_linear, want_pixels, want_history = model_resolve(film, params)
    assert same_words(linear, want_linear), what
    assert np.array_equal(pixels, want_pixels), what
    assert same_words(history, want_history), what
    return linear, pixels, history


@pytest.mark.parametrize("scale_log2, clamp_max", SCALES)
@pytest.mark.parametrize("exposure", [0.0, 1.0, 0.37, 40.0])
def test_probe_resolve_equals_the_model(scale_log2, clamp_max, exposure):
    params = params_of(scale_log2, clamp_max, exposure)
    film = resolve_rows(params)
    linear, pixels, history = check_resolve(film, params, (scale_log2, exposure))
    empty = film["samples"] == 0
    assert empty.sum() == 2 and not linear.view(np.float32).reshape(-1, 4)[empty].any() and not history.view(np.float32).reshape(-1, 4)[empty].any()
    assert (pixels[empty] == (0, 0, 0, 255)).all() and (pixels[:, 3] == 255).all()
    assert np.array_equal(linear["weight"], film["samples"].astype(np.float32)) and np.array_equal(history["weight"], linear["weight"])
    if exposure == 0.0:
        assert not pixels[:, :3].any() and not history["r"].any()
    # the linear means do not depend on the exposure
    assert same_words(linear, ptss.probe_resolve_linear(film, params=params_of(scale_log2, clamp_max, 1.0))[0])


def test_the_conversion_of_a_large_mean_rounds_to_even():
    params = params_of(0, 2.0 ** 40)
    big = 1 << 25
    film = np.concatenate([entry(big + 1, big + 2, big + 3, 1), entry(big + 6, big + 5, (1 << 40), 1), entry(3 * big + 2, 3 * big + 1, 0, 3)])
    linear, _, _ = check_resolve(film, params, "large means")
    assert [float(linear[c][0]) for c in "rgb"] == [big, big, big + 4] and [float(linear[c][1]) for c in "rgb"] == [big + 8, big + 4, 2.0 ** 40]
    assert float(linear["r"][2]) == big and float(linear["g"][2]) == big   # m = (3 big + 2 + 1) / 3 = big + 1, which rounds to big; m = (3 big + 1 + 1) / 3 = big


def test_an_exposure_that_puts_the_mean_on_a_threshold():
    """mean = 1 exactly (sum = 2^s, N = 1), exposure = a threshold of the table and its two neighbours: e = the exposure itself."""
    T = quant_thresholds()
    for k in (1, 2, 18, 128, 201, 255):
        for x, byte in ((down(T[k]), k - 1), (T[k], k), (up(T[k]), k)):
            params = params_of(20, 65536.0, float(x))
            _, pixels, _ = check_resolve(entry(1 << 20, 2 << 20, 1 << 19, 1), params, (k, float(x)))
            assert pixels[0, 0] == byte, (k, float(x))


def test_the_tone_map_of_the_mean_is_not_the_mean_of_tone_maps():
    """What the film is for: a sample of radiance 40 counts as 40, and the exposure is chosen afterwards."""
    res = results_of(np.array([[40.0, 0.0, 0.5], [0.0, 0.0, 0.5]], np.float32))
    film, _ = ptss.probe_accumulate_linear(res, linear_film(1), index=np.zeros(2, np.uint32))
    linear, pixels, _ = ptss.probe_resolve_linear(film)
    assert (float(linear["r"][0]), float(linear["g"][0]), float(linear["b"][0]), float(linear["weight"][0])) == (20.0, 0.0, 0.5, 2.0)
    assert pixels[0, 0] == 255 and pixels[0, 1] == 0
    _, dim, _ = ptss.probe_resolve_linear(film, params=ptss.linear_params(exposure=1.0 / 80))
    assert 0 < dim[0, 0] < 255   # 20 / 80 = 0.25
    tone_mapped, _, _, _ = ptss.probe_accumulate(res, np.zeros(1, ptss.FILM_DTYPE), index=np.zeros(2, np.uint32))
    assert tone_mapped["r"][0] == 255   # the 8-bit film saw 1 + 0


# ---- order freedom -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_any_permutation_and_any_split_give_the_same_film(seed):
    g = np.random.default_rng(100 + seed)
    params = params_of(*SCALES[seed % len(SCALES)])
    res = adversarial_results(params, seed=seed)
    n, P = len(res), 37
    index = g.integers(0, P + 3, n).astype(np.uint32)   # duplicates everywhere, some entries beyond the film
    start = high_film(P) if seed % 2 else linear_film(P)
    whole, dropped = ptss.probe_accumulate_linear(res, start, index=index, params=params)
    for _ in range(4):
        order = g.permutation(n)
        film, d = ptss.probe_accumulate_linear(res[order], start, index=index[order], params=params)
        assert film.tobytes() == whole.tobytes() and d == dropped
        cut = int(g.integers(0, n + 1))
        first, d1 = ptss.probe_accumulate_linear(res[order][:cut], start, index=index[order][:cut], params=params)
        both, d2 = ptss.probe_accumulate_linear(res[order][cut:], first, index=index[order][cut:], params=params)
        assert both.tobytes() == whole.tobytes() and d1 + d2 == dropped
