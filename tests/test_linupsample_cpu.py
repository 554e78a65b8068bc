"""Upsampling the two linear films without a GPU (ptss_upsample_linear, ptss_probe_upsample_linear): the record layouts
against the header, the symbols and the defaults, every refusal of the probe, the host build of csrc/ptlinup.h (the specification of
the device's film) byte for byte against a model in Python integers and numpy float32 (tests/linupsample_common.py), and the call's
exact properties, each a test of its own.

Every comparison here is exact; no tolerance is used. The synthetic cases must filter: at least half of a case's hi pixels are
`filtered`, and at least one is `fallback` and one `empty` — asserted on the probe's info (covered()), so that no test passes by
filtering nothing. The seeds in CASES were picked so that this holds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptss
from linupsample_common import (BAD_SIDES, BIG_PARAMS, COARSE_PARAMS, DEFAULT_PARAMS, FACTORS, FILM_REFUSED, UP_REFUSED, case, changed, features_of,
                                film_of, first_difference, integer_means, model_lo, model_upsample, same_bytes, words, wrapped_sums_film)
from ptss_types import UpsampleLinearParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
W, H = 9, 6   # the lo film of the synthetic cases
KINDS = (False, True)


def covered(info, pixels):
    """The coverage condition of the synthetic cases, on the probe's counters."""
    assert int(info["filtered"]) + int(info["fallback"]) + int(info["empty"]) == pixels
    assert 2 * int(info["filtered"]) >= pixels and int(info["fallback"]) >= 1 and int(info["empty"]) >= 1, info


def probe(film, w, h, flo, fhi, params, up):
    return ptss.probe_upsample_linear(film, w, h, flo, fhi, params, up)


# ---- layout, symbols, defaults ------------------------------------------------------------------------------------------------------------------
def test_the_mirrors_match_the_c_layout(tmp_path):
    names = ["structSize", "factor", "sigmaNormal", "sigmaDepth", "flags", "reserved"]
    counters = ["filtered", "fallback", "empty"]
    prints = "".join(f'printf(" %zu", offsetof(ptss_upsample_linear_params, {n}));' for n in names)
    prints += "".join(f'printf(" %zu", offsetof(ptss_upsample_linear_info, {n}));' for n in counters)
    src = (f'#include <stdio.h>\n#include <stddef.h>\n#include "ptss.h"\n#include "ptss_host.h"\n'
           f'int main(void){{printf("%zu %zu %u %d", sizeof(ptss_upsample_linear_params), sizeof(ptss_upsample_linear_info), '
           f'PTSS_UPSAMPLE_LINEAR_WRAP_X, PTSS_HOST_ERANGE); {prints} return 0;}}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(UpsampleLinearParams) == 24 and got[1] == ptss.UPSAMPLE_LINEAR_INFO_DTYPE.itemsize == 24
    assert got[2] == ptss.UPSAMPLE_LINEAR_WRAP_X == 1 and got[3] == -3
    assert got[4:10] == [getattr(UpsampleLinearParams, n).offset for n in names] == [0, 4, 8, 12, 16, 20]
    assert got[10:] == [ptss.UPSAMPLE_LINEAR_INFO_DTYPE.fields[n][1] for n in counters] == [0, 8, 16]


def test_symbols_and_defaults():
    dev, host = C.CDLL(ptss.DEVICE_LIB), C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_default_upsample_linear_params", "ptss_upsample_linear", "ptss_upsample_linear_launches", "ptss_debug_upsample_linear_form"):
        assert hasattr(dev, name), name
    assert hasattr(host, "ptss_probe_upsample_linear")
    p = UpsampleLinearParams()
    dev.ptss_default_upsample_linear_params.argtypes = [C.POINTER(UpsampleLinearParams)]
    assert dev.ptss_default_upsample_linear_params(C.byref(p)) == 0 and dev.ptss_default_upsample_linear_params(None) == -1
    assert bytes(p) == bytes(ptss.upsample_linear_params())
    assert (p.structSize, p.factor, p.sigmaNormal, p.sigmaDepth, p.flags, p.reserved) == (24, 2, float(np.float32(0.1)), 4.0, 0, 0)
    assert ptss.upsample_linear_params(3, 0.2, 5.0, wrap_x=True).flags == ptss.UPSAMPLE_LINEAR_WRAP_X
    for name in ("upsample_linear", "upsample_linear_launches", "debug_upsample_linear_form"):
        assert callable(getattr(ptss.Renderer, name))


# ---- the refusal lists: defined here against the probe, imported by the GPU test ----------------------------------------------------------------
def test_every_refusal_of_the_probe():
    L = ptss.host_lib()
    params = DEFAULT_PARAMS
    film, flo, fhi, good = case(W, H, 2, params)
    f4 = words(film)
    out = np.zeros((4 * W * H, 4), np.uint64)
    info = np.zeros(1, ptss.UPSAMPLE_LINEAR_INFO_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None

    def run(f=f4, kind=0, width=W, height=H, lo=flo, hi=fhi, p=params, u=good, o=out, i=info):
        return L.ptss_probe_upsample_linear(ptr(f), kind, width, height, ptr(lo), ptr(hi), ref(p), ref(u), ptr(o), ptr(i))

    assert run() == 0 and run(kind=1) == 0 and run(i=None) == 0
    before, counted = out.copy(), info.copy()
    assert run(f=None) == -1 and run(lo=None) == -1 and run(hi=None) == -1 and run(o=None) == -1 and run(p=None) == -1 and run(u=None) == -1
    for kind in (2, -1, 77):
        assert run(kind=kind) == -1
    for change in UP_REFUSED:
        assert run(u=changed(lambda: ptss.upsample_linear_params(2), **change)) == -1, change
    for change in FILM_REFUSED:
        assert run(p=changed(lambda: ptss.linear_params(clamp_max=2.0 ** 20), **change)) == -1, change
    for width, height, factor in BAD_SIDES:
        assert run(width=width, height=height, u=ptss.upsample_linear_params(factor)) == -3, (width, height, factor)
    # an output range that overlaps the input film: the same block, and a block that starts inside it
    both = np.zeros((5 * W * H, 4), np.uint64)
    both[:W * H] = f4
    assert run(f=both[:W * H], o=both[:4 * W * H]) == -1 and run(f=both[:W * H], o=both[W * H - 1:]) == -1
    assert run(f=both[4 * W * H:], o=both[:4 * W * H], i=None) == 0   # side by side is fine
    assert np.array_equal(out, before) and info.tobytes() == counted.tobytes()
    for factor in (1, 4):   # the ends of the range are taken, and both flags values
        o = np.zeros((factor * factor * W * H, 4), np.uint64)
        hi = features_of(W * factor, H * factor)
        assert run(hi=hi, o=o, u=ptss.upsample_linear_params(factor, 1e-30, 1e30, wrap_x=factor == 4)) == 0


# ---- the probe against the model, byte for byte ------------------------------------------------------------------------------------------------
CASES = [(splat, f, wrap) for splat in KINDS for f in FACTORS for wrap in (False, True)]


@pytest.mark.parametrize("splat,f,wrap", CASES)
def test_probe_equals_the_model(splat, f, wrap):
    """Both film kinds, factors 1..4, with and without the wrap, features with misses and NaN, films with empty pixels, means up to 2^40."""
    params = BIG_PARAMS
    film, flo, fhi, up = case(W, H, f, params, seed=f, splat=splat, wrap=wrap, bad=True, big=True)
    got, info = probe(film, W, H, flo, fhi, params, up)
    want, counts, _ = model_upsample(film, W, H, flo, fhi, params, up)
    assert first_difference(got, want) is None
    assert [int(info[k]) for k in ("filtered", "fallback", "empty")] == counts
    covered(info, f * f * W * H)
    assert max(max(m) for m in integer_means(film) if m is not None) == 1 << 40


@pytest.mark.parametrize("splat", KINDS)
def test_probe_equals_the_model_on_words_no_film_holds(splat):
    """Entries whose sums wrap, another scale, a size of one pixel and a film one column wide under the wrap."""
    for (w, h), f, wrap, params in (((5, 4), 2, True, COARSE_PARAMS), ((1, 1), 3, True, DEFAULT_PARAMS), ((1, 5), 4, True, COARSE_PARAMS),
                                    ((4, 1), 3, False, DEFAULT_PARAMS)):
        film = wrapped_sums_film(w * h, splat, seed=w)
        flo, fhi = features_of(w, h, bad=True), features_of(w * f, h * f, bad=True)
        up = ptss.upsample_linear_params(f, 0.1, 4.0, wrap_x=wrap)
        got, info = probe(film, w, h, flo, fhi, params, up)
        want, counts, _ = model_upsample(film, w, h, flo, fhi, params, up)
        assert first_difference(got, want) is None, (w, h, f)
        assert [int(info[k]) for k in ("filtered", "fallback", "empty")] == counts


# ---- properties, each its own test ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splat", KINDS)
def test_factor_one_leaves_every_integer_mean_unchanged(splat):
    params = BIG_PARAMS
    for wrap in (False, True):
        film, flo, fhi, up = case(W, H, 1, params, splat=splat, wrap=wrap, big=True)
        fhi = fhi.copy()
        fhi["materialIdx"][::4] = 5   # some hi features disagree with their lo pixel: the fallback copies too
        got, info = probe(film, W, H, flo, fhi, params, up)
        assert integer_means(got) == integer_means(film)
        assert int(info["fallback"]) >= 1 and int(info["empty"]) >= 1 and int(info["filtered"]) >= 1


@pytest.mark.parametrize("splat", KINDS)
@pytest.mark.parametrize("f", FACTORS)
def test_a_constant_film_stays_exactly_constant(splat, f):
    """m >= 2^24, where the float of a mean is no longer the mean: every non-empty hi pixel holds m itself."""
    params = BIG_PARAMS
    film, flo, fhi, up = case(W, H, f, params, seed=3, splat=splat)
    m = ((1 << 40) - 1, (1 << 24) + 1, (1 << 33) + 12345)
    for p in range(W * H):
        n = int(film[p]["weight"]) >> 16 if splat else int(film[p]["samples"])   # (film_of's weights are at least 62,536)
        if int(film[p]["weight"] if splat else film[p]["samples"]):
            n = max(n, 1)
            film[p] = (m[0] * n, m[1] * n, m[2] * n, n << 16) if splat else (m[0] * n, m[1] * n, m[2] * n, n, 0)
    assert {e for e in integer_means(film) if e is not None} == {m}
    got, info = probe(film, W, H, flo, fhi, params, up)
    covered(info, f * f * W * H)
    assert {e for e in integer_means(got) if e is not None} == {m}


@pytest.mark.parametrize("splat", KINDS)
@pytest.mark.parametrize("f", (2, 3, 4))
def test_every_channel_lies_in_the_hull_of_its_counted_taps_and_no_colour_crosses_a_material(splat, f):
    params = DEFAULT_PARAMS
    film, flo, fhi, up = case(W, H, f, params, seed=f, splat=splat, wrap=True)
    got, info = probe(film, W, H, flo, fhi, params, up)
    covered(info, f * f * W * H)
    _, _, counted = model_upsample(film, W, H, flo, fhi, params, up)
    lo, hi_means = model_lo(film), integer_means(got)
    for P, taps in enumerate(counted):
        if not taps:
            continue
        for q in taps:   # a counted tap has the hi pixel's material
            assert int(flo[q]["materialIdx"]) == int(fhi[P]["materialIdx"])
        for ch in range(3):
            ms = [lo[q][0][ch] for q in taps]
            assert min(ms) <= hi_means[P][ch] <= max(ms), (P, ch)


@pytest.mark.parametrize("splat", KINDS)
def test_no_colour_crosses_a_material_boundary(splat):
    """Material 0 holds one colour, every other material another: a hi pixel of material 0 comes out with material 0's colour exactly."""
    params, f = DEFAULT_PARAMS, 2
    film, flo, fhi, up = case(W, H, f, params, seed=1, splat=splat, holes=False)
    a, b = (1000, 2000, 3000), (900000, 800000, 700000)
    for p in range(W * H):
        n = max(1, int(film[p]["weight"]) >> 16) if splat else int(film[p]["samples"])
        m = a if int(flo[p]["materialIdx"]) == 0 else b
        film[p] = (m[0] * n, m[1] * n, m[2] * n, n << 16) if splat else (m[0] * n, m[1] * n, m[2] * n, n, 0)
    got, info = probe(film, W, H, flo, fhi, params, up)
    means = integer_means(got)
    nearest = lambda P: ((P // (f * W)) // f) * W + (P % (f * W)) // f
    some = 0
    for P in range(f * f * W * H):
        if int(fhi[P]["materialIdx"]) == 0 and int(flo[nearest(P)]["materialIdx"]) == 0:
            assert means[P] == a, P
            some += 1
    assert some > 20 and int(info["filtered"]) * 2 >= f * f * W * H


@pytest.mark.parametrize("splat", KINDS)
def test_the_row_gives_back_its_mean_and_the_counters_sum(splat):
    """(m' K + K / 2) / K = m' on every row, clamped = 0, and filtered + fallback + empty = f^2 W H, added to what info held."""
    params = BIG_PARAMS
    for f in FACTORS:
        film, flo, fhi, up = case(W, H, f, params, seed=f, splat=splat, big=True, bad=True)
        start = np.zeros(1, ptss.UPSAMPLE_LINEAR_INFO_DTYPE)
        start[0] = (5, 7, 11)
        got, info = ptss.probe_upsample_linear(film, W, H, flo, fhi, params, up, info=start[0])
        assert int(info["filtered"]) + int(info["fallback"]) + int(info["empty"]) == f * f * W * H + 23
        assert int(info["filtered"]) >= 5 and int(info["fallback"]) >= 7 and int(info["empty"]) >= 11
        assert got.dtype == ptss.LINEAR_DTYPE and not got["clamped"].any()
        for e in got:
            K = int(e["samples"])
            if K == 0:
                assert (int(e["r"]), int(e["g"]), int(e["b"])) == (0, 0, 0)
                continue
            for ch in "rgb":
                s = int(e[ch])
                assert s % K == 0 and (s + K // 2) // K == s // K


def test_a_box_filtered_film_gives_the_linear_films_means():
    """A filtered film made by the box at radius 0.5 — every sample lands in its own pixel with weight 65536 — is the linear film with
    weight = samples << 16 and sums that hold the same means; its output means are the linear film's."""
    params = DEFAULT_PARAMS
    for f in (2, 3):
        film, flo, fhi, up = case(W, H, f, params, seed=2)
        box = np.zeros(W * H, dtype=ptss.SPLAT_DTYPE)
        for p in range(W * H):
            n = int(film[p]["samples"])
            box[p] = (int(film[p]["r"]), int(film[p]["g"]), int(film[p]["b"]), n << 16)   # S = sum (q * 65536) >> 16
        a, ia = probe(film, W, H, flo, fhi, params, up)
        b, ib = probe(box, W, H, flo, fhi, params, up)
        covered(ia, f * f * W * H)
        assert ia.tobytes() == ib.tobytes() and integer_means(a) == integer_means(b)
        assert same_bytes(a, b)   # K = samples on both, clamped = 0 on both


@pytest.mark.parametrize("splat", KINDS)
@pytest.mark.parametrize("f", FACTORS)
def test_with_the_wrap_a_roll_of_the_inputs_rolls_the_output(splat, f):
    params = DEFAULT_PARAMS
    film, flo, fhi, up = case(W, H, f, params, seed=5, splat=splat, wrap=True, bad=True)
    base, info = probe(film, W, H, flo, fhi, params, up)
    covered(info, f * f * W * H)
    roll = lambda a, w, h, k: np.roll(np.ascontiguousarray(a).reshape(h, w), k, axis=1).reshape(-1)
    for k in (1, 4, W - 1):
        got, moved = probe(roll(film, W, H, k), W, H, roll(flo, W, H, k), roll(fhi, W * f, H * f, f * k), params, up)
        assert same_bytes(got, roll(base, W * f, H * f, f * k)), k
        assert moved.tobytes() == info.tobytes()


@pytest.mark.parametrize("f", (2, 3, 4))
def test_the_wrap_takes_the_seams_taps_from_the_other_side(f):
    """One flat surface, column x of the film holding the mean 1000 (x + 1): with the flag the first hi column mixes lo columns 0 and
    W - 1, without it that tap is outside the film and the column keeps lo column 0's mean."""
    params = DEFAULT_PARAMS
    flat = lambda n: np.array([((0.0, 0.0, 1.0), 2.0, (0.5, 0.5, 0.5), 0)] * n, dtype=ptss.FEATURE_DTYPE)
    film = np.zeros(W * H, dtype=ptss.LINEAR_DTYPE)
    for p in range(W * H):
        film[p] = (1000 * (p % W + 1),) * 3 + (1, 0)
    with_flag, _ = probe(film, W, H, flat(W * H), flat(f * f * W * H), params, ptss.upsample_linear_params(f, 0.1, 4.0, wrap_x=True))
    without, _ = probe(film, W, H, flat(W * H), flat(f * f * W * H), params, ptss.upsample_linear_params(f, 0.1, 4.0))
    a, b = np.asarray(integer_means(with_flag)).reshape(f * H, f * W, 3), np.asarray(integer_means(without)).reshape(f * H, f * W, 3)
    assert (b[:, 0] == 1000).all() and (b[:, -1] == 1000 * W).all()
    assert ((a[:, 0] > 1000) & (a[:, 0] < 1000 * W)).all() and ((a[:, -1] > 1000) & (a[:, -1] < 1000 * W)).all()
    inner = slice(f, -f)
    assert np.array_equal(a[:, inner], b[:, inner])


# ---- the sanitizers ---------------------------------------------------------------------------------------------------------------------------
def test_the_probe_runs_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/linupsample_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host
    build of csrc/ptlinup.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "linupsample_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "linupsample_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("linupsample_sanitize ok"), r.stdout + r.stderr
