"""Glare for the two linear films without a GPU (ptss_glare_build, ptss_resolve_linear_glare / ptss_resolve_splat_glare):
the record layouts against the header, the exported symbols, the defaults and the layout function of both libraries, what the probes
refuse, and the host build of csrc/ptglare.h (the specification of the device's pyramid and resolve) against the model of
tests/glare_common.py: the pyramid for every level count at sizes from one pixel to ones that cross a tile, on both films, with pixels
without samples, three thresholds and films whose words wrap; the resolve in both modes at four strengths with and without a meter's
state; and the properties the design rests on — a constant film, strength 0, the four bounds, and impulses whose pyramid is known."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from glare_common import (LEVELS, MODES, SIZES, STRENGTHS, TOP, default_params, film_of, first_difference, impulse_film, model_downs, model_layout,
                          model_means, model_mixed, model_pyramid, model_resolve_glare, model_threshold, model_ups, pyramid_of, same_bytes, strength_word,
                          thresholds_for)
from linear_common import SCALES, linear_film, params_of, same_words
from meter_common import new_state
from splat_common import splat_film

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")


def test_structs_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes mirrors and the numpy record."""
    fields = (("ptss_glare_params", ("structSize", "levels", "mode", "threshold", "strength", "reserved")),
              ("ptss_glare_entry", ("r", "g", "b", "zero")), ("ptss_glare_level", ("width", "height", "first")))
    body = "".join('printf("%%zu\\n", sizeof(%s));' % s for s, _ in fields)
    body += "".join('printf("%%zu\\n", offsetof(%s, %s));' % (s, f) for s, fs in fields for f in fs)
    body += 'printf("%d %d %d %d %d\\n", PTSS_GLARE_MAX_LEVELS, PTSS_GLARE_ADD, PTSS_GLARE_MIX, PTSS_GLARE_FILM_LINEAR, PTSS_GLARE_FILM_SPLAT);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { ' + body + ' return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Par, Lev = ptss_types.GlareParams, ptss_types.GlareLevel
    assert got[:3] == [C.sizeof(Par), ptss.GLARE_DTYPE.itemsize, C.sizeof(Lev)] == [24, 32, 16]
    assert got[3:9] == [getattr(Par, f).offset for f in fields[0][1]] == [0, 4, 8, 12, 16, 20]
    assert got[9:13] == [ptss.GLARE_DTYPE.fields[f][1] for f in fields[1][1]] == [0, 8, 16, 24]
    assert got[13:16] == [getattr(Lev, f).offset for f in fields[2][1]] == [0, 4, 8]
    assert got[16:] == [ptss_types.GLARE_MAX_LEVELS, ptss_types.GLARE_ADD, ptss_types.GLARE_MIX, ptss_types.GLARE_FILM_LINEAR,
                        ptss_types.GLARE_FILM_SPLAT] == [8, 0, 1, 0, 1]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed
    header = open(os.path.join(CSRC, "ptglare.h")).read()   # the shapes the GPU tests size their films by
    assert int(re.search(r"kTile = (\d+);", header).group(1)) == ptss_types.GLARE_TILE
    assert int(re.search(r"kTailEntries = (\d+);", header).group(1)) == ptss_types.GLARE_TAIL_ENTRIES
    assert ptss_types.GLARE_TAIL_ENTRIES * 24 <= 65536   # the tail's levels fit the LDS one workgroup may ask for


def test_libraries_export_the_symbols_and_the_defaults():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_glare_params", "ptss_glare_layout", "ptss_glare_build", "ptss_resolve_linear_glare", "ptss_resolve_splat_glare",
                 "ptss_glare_launches"):
        assert hasattr(L, name), name
    for name in ("ptss_glare_layout", "ptss_probe_glare_build", "ptss_probe_resolve_glare"):
        assert hasattr(ptss.host_lib(), name), name
    assert L.ptss_version() == 300
    g = ptss_types.GlareParams()
    assert L.ptss_default_glare_params(C.byref(g)) == 0 and L.ptss_default_glare_params(None) == -1
    assert (g.structSize, g.levels, g.mode, g.threshold, g.strength, g.reserved) == (24, 6, ptss.GLARE_MIX, 0.0, float(np.float32(0.1)), 0)
    assert bytes(ptss.glare_params()) == bytes(g)
    # refused before anything touches a device
    p = ptss.linear_params()
    assert L.ptss_glare_build(None, None, 0, 4, 4, C.byref(p), C.byref(g), None, None) == -1
    assert L.ptss_resolve_linear_glare(None, None, 0, 0, C.byref(p), 4, 4, C.byref(g), None, None, None, None, None, None) == -1
    assert L.ptss_resolve_splat_glare(None, None, 0, 0, C.byref(p), 4, 4, C.byref(g), None, None, None, None, None, None) == -1
    assert L.ptss_glare_launches(None, (C.c_ulonglong * 3)()) == -1


@pytest.mark.parametrize("which", ["device", "host"])
def test_the_layout_function_of_both_libraries(which):
    L = ptss.device_lib() if which == "device" else ptss.host_lib()
    out, n = (ptss_types.GlareLevel * 8)(), C.c_size_t(77)
    for (w, h) in SIZES + ((1920, 1080), (2 ** 22, 1), (1, 2 ** 22), (46340, 46340), (2 ** 22, 511)):
        for levels in LEVELS:
            assert L.ptss_glare_layout(w, h, levels, out, C.byref(n)) == 0
            want, entries = model_layout(w, h, levels)
            assert [(out[k].width, out[k].height, out[k].first) for k in range(levels)] == want and n.value == entries, (w, h, levels)
    assert ptss.glare_layout(1920, 1080, 8)[0][4] == (60, 34, 518400 + 129600 + 32400 + 8160)
    assert ptss.glare_layout(1, 1, 8) == ([(1, 1, k) for k in range(8)], 8)
    einval, erange = (-1, -5) if which == "device" else (-1, -1)
    n.value = 77
    for levels in (0, -1, 9):
        assert L.ptss_glare_layout(4, 4, levels, out, C.byref(n)) == einval
    assert L.ptss_glare_layout(4, 4, 3, None, C.byref(n)) == einval and L.ptss_glare_layout(4, 4, 3, out, None) == einval
    for w, h in ((0, 4), (4, 0), (-3, 4), (2 ** 22 + 1, 1), (1, 2 ** 22 + 1), (2 ** 22, 512), (46341, 46341)):   # 2^22 * 512 = 2^31
        assert L.ptss_glare_layout(w, h, 3, out, C.byref(n)) == erange, (w, h)
    assert n.value == 77   # a refused call writes nothing


def changed(make, **change):
    s = make()
    for k, v in change.items():
        setattr(s, k, v)
    return s


GLARE_REFUSED = (dict(structSize=20), dict(structSize=0), dict(levels=0), dict(levels=9), dict(levels=-1), dict(mode=2), dict(mode=-1),
                 dict(strength=-0.01), dict(strength=1.01), dict(strength=float("nan")), dict(threshold=-1.0), dict(threshold=float("nan")),
                 dict(threshold=float("inf")), dict(threshold=2.0 ** 20 * 1.001), dict(reserved=1))   # at scaleLog2 = 20: threshold * 2^20 > 2^40
LINEAR_REFUSED = (dict(structSize=16), dict(scaleLog2=33), dict(clampMax=0.0), dict(exposure=-0.5), dict(reserved=1))


def test_the_probes_refuse_what_the_calls_refuse():
    H = ptss.host_lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    lin, good = ptss.linear_params(), ptss.glare_params(levels=3)
    film = film_of(5, 4, False, lin)
    pyr = np.full((ptss.glare_layout(5, 4, 3)[1], 4), 7, np.uint64)
    untouched = pyr.copy()
    out = np.full((20, 4), 3.0, np.float32)

    def build(params=lin, glare=good, f=film, kind=0, w=5, h=4, p=pyr):
        return H.ptss_probe_glare_build(vp(f), kind, w, h, ref(params), ref(glare), vp(p))

    def resolve(params=lin, glare=good, f=film, kind=0, w=5, h=4, p=pyr, first=0, count=20):
        return H.ptss_probe_resolve_glare(vp(f), kind, first, count, ref(params), w, h, ref(glare), vp(p), None, vp(out), None, None)

    for call in (build, resolve):
        assert call(params=None) != 0 and call(glare=None) != 0 and call(f=None) != 0 and call(p=None) != 0 and call(kind=2) != 0 and call(kind=-1) != 0
        for change in GLARE_REFUSED:
            assert call(glare=changed(lambda: ptss.glare_params(levels=3), **change)) != 0, change
        for change in LINEAR_REFUSED:
            assert call(params=changed(ptss.linear_params, **change)) != 0, change
        for w, h in ((0, 4), (5, 0), (2 ** 22 + 1, 1), (2 ** 22, 512)):
            assert call(w=w, h=h) != 0, (w, h)
    for first, count in ((0, 21), (20, 1), (21, 0 + 1), (2 ** 63, 2 ** 63)):
        assert resolve(first=first, count=count) != 0, (first, count)
    assert np.array_equal(pyr, untouched) and (out == 3.0).all()   # nothing refused wrote anything
    assert resolve(count=0) == 0 and resolve(first=20, count=0) == 0 and resolve(f=None, p=None, count=0) == 0 and (out == 3.0).all()
    # the boundaries are allowed
    for glare in (ptss.glare_params(levels=1), ptss.glare_params(levels=8), ptss.glare_params(strength=0.0), ptss.glare_params(strength=1.0),
                  ptss.glare_params(threshold=2.0 ** 20), ptss.glare_params(mode="add")):
        big = np.zeros((ptss.glare_layout(5, 4, glare.levels)[1], 4), np.uint64)
        assert build(glare=glare, p=big) == 0 and resolve(glare=glare, p=big) == 0
    assert build() == 0 and not np.array_equal(pyr, untouched) and not pyr[:, 3].any()   # the fourth word is written, as 0


def test_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/glare_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host build
    of csrc/ptglare.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "glare_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "glare_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("glare_sanitize ok"), r.stdout + r.stderr


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------------------------
def check_pyramids(film, w, h, params, thresholds, modes=("mix",)):
    """The probe's pyramid against the model for every level count; the downs are taken once per threshold."""
    for th in thresholds:
        downs = model_downs(film, w, h, model_threshold(th, params), 8)
        for levels in LEVELS:
            glare = ptss.glare_params(levels=levels, threshold=th)
            got = ptss.probe_glare_build(film, w, h, params, glare)
            want = model_pyramid(film, w, h, params, glare, downs)
            assert len(got) == ptss.glare_layout(w, h, levels)[1] and same_bytes(got, want), (w, h, levels, th, first_difference(got, want))


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_the_pyramid_equals_the_model(size, splat):
    w, h = size
    params = default_params()
    film = film_of(w, h, splat, params)
    assert (film["weight"] == 0).any() if splat else (film["samples"] == 0).any()
    check_pyramids(film, w, h, params, thresholds_for(film, params))
    above = ptss.probe_glare_build(film, w, h, params, ptss.glare_params(levels=3, threshold=2.0 ** 20))
    rows = above.view(np.uint64).reshape(-1, 4)
    assert not rows[:, 3].any()
    if w * h > 1:   # (the pool holds rows beyond a library film, whose means pass any threshold; the library's own do not)
        top = film_of(w, h, splat, params, kind="top")
        assert not ptss.probe_glare_build(top, w, h, params, ptss.glare_params(levels=3, threshold=2.0 ** 20)).view(np.uint64).any()


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
@pytest.mark.parametrize("scale", SCALES[:3], ids=lambda s: "scale%d" % s[0])
def test_the_pyramid_at_every_scale(scale, splat):
    params = params_of(*scale)
    film = film_of(37, 21, splat, params, seed=5)
    check_pyramids(film, 37, 21, params, thresholds_for(film, params)[1:2] + (0.0,))


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_films_the_library_did_not_fill_wrap_on_both_sides_alike(splat):
    params = default_params()
    for w, h in ((3, 3), (37, 21)):
        film = film_of(w, h, splat, params, kind="high")
        check_pyramids(film, w, h, params, (0.0, 1.5))
        glare = ptss.glare_params(levels=4, mode="add", strength=1.0)
        pyr = ptss.probe_glare_build(film, w, h, params, glare)
        got = ptss.probe_resolve_glare(film, w, h, pyr, params=params, glare=glare)
        want = model_resolve_glare(film, w, h, pyr, params, glare)
        assert all(same_words(a, b) for a, b in zip(got, want))
    # sums that wrap inside a down: 64 * 2^60 is 2^66
    film = linear_film(9)
    film["r"], film["g"], film["b"], film["samples"] = (1 << 60) + 5, (1 << 63) + 1, (1 << 64) - 1, 1
    check_pyramids(film, 3, 3, params, (0.0,))
    assert int(ptss.probe_glare_build(film, 3, 3, params, ptss.glare_params(levels=1))["r"][0]) == (((64 * ((1 << 60) + 5) + 32) & (2 ** 64 - 1)) >> 6)


# ---- the resolve ------------------------------------------------------------------------------------------------------------------------------------
def a_state(exposure):
    s = new_state()
    s["exposure"], s["target"], s["updates"] = exposure, exposure, 2
    return s


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
@pytest.mark.parametrize("mode", MODES)
def test_the_resolve_equals_the_model(mode, splat):
    w, h = 13, 9
    params = params_of(20, 65536.0, exposure=0.75)
    film = film_of(w, h, splat, params, seed=2)
    for strength in STRENGTHS:
        glare = ptss.glare_params(levels=3, mode=mode, threshold=0.125, strength=strength)
        pyr = ptss.probe_glare_build(film, w, h, params, glare)
        for state in (None, a_state(2.5)):
            got = ptss.probe_resolve_glare(film, w, h, pyr, params=params, glare=glare, state=state)
            want = model_resolve_glare(film, w, h, pyr, params, glare, state)
            for name, a, b in zip(("linear", "pixels", "history"), got, want):
                assert same_words(a, b), (mode, strength, state is not None, name)
    # a sub-range leaves the rest alone; NULL outputs are not written
    ln, px, hs = ptss.probe_resolve_glare(film, w, h, pyr, 17, 40, params, glare, linear=np.full((w * h, 4), 9.0, np.float32), pixels=None)
    assert px is None and same_words(ln[17:57], want[0][17:57]) and (ln.view(np.float32).reshape(-1, 4)[:17] == 9.0).all()
    assert (ln.view(np.float32).reshape(-1, 4)[57:] == 9.0).all() and same_words(hs[17:57], want[2][17:57]) and not hs.view(np.float32).reshape(-1, 4)[57:].any()


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_strength_zero_is_the_plain_resolve(splat):
    """Every pixel, the ones without samples included, whatever the pyramid holds — on every film whose means stay below 2^48, far beyond
    what the library leaves (2^40): m * 65536 is taken in 64 bits."""
    params = params_of(20, 65536.0, exposure=1.5)
    for (w, h), kind in (((37, 21), "pool"), ((5, 7), "top")):
        film = film_of(w, h, splat, params, kind=kind)
        beyond = [p for p, e in enumerate(model_means(film)) if max(e[:3]) >= 1 << 48]
        film[beyond] = film_of(w, h, splat, params, kind="top")[beyond]
        assert kind == "top" or (film["weight" if splat else "samples"] == 0).any()
        plain = (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(film, params=params)
        for mode in MODES:
            glare = ptss.glare_params(levels=4, mode=mode, strength=0.0)
            pyr = ptss.probe_glare_build(film, w, h, params, glare)
            assert pyr.view(np.uint64).any()
            got = ptss.probe_resolve_glare(film, w, h, pyr, params=params, glare=glare)
            assert all(same_bytes(a, b) for a, b in zip(got, plain)), (kind, mode)


def test_a_pixel_without_samples_takes_the_glare_and_keeps_its_weight():
    params = default_params()
    film = impulse_film(6, 6, 3, 3, 1000 << 20)
    film["samples"][2 * 6 + 3] = 0   # the impulse's neighbour holds nothing
    film["r"][2 * 6 + 3] = 99
    glare = ptss.glare_params(levels=2, mode="add", strength=1.0)
    pyr = ptss.probe_glare_build(film, 6, 6, params, glare)
    ln, px, hs = ptss.probe_resolve_glare(film, 6, 6, pyr, params=params, glare=glare)
    assert ln["r"][15] > 0 and ln["weight"][15] == 0 and hs["weight"][15] == 0 and px[15, 0] == 255 and ln["weight"][14] == 1
    want = model_resolve_glare(film, 6, 6, pyr, params, glare)
    assert all(same_words(a, b) for a, b in zip((ln, px, hs), want))


# ---- the properties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_a_constant_film_gives_a_constant_pyramid_and_itself_back(splat):
    params = default_params()
    for (w, h), c in (((1, 1), 12345), ((7, 5), 1), ((37, 21), (1 << 40) - 1), ((64, 48), 1 << 40), ((65, 34), 987654321)):
        P = w * h
        film = splat_film(P) if splat else linear_film(P)
        film["r"], film["g"], film["b"] = (c * 3, 2 * c * 3, (c // 2) * 3) if not splat else (3 * c, 6 * c, 3 * (c // 2))   # means c, 2c (c where that leaves a film), c / 2
        if c * 2 > TOP:
            film["g"] = film["r"]
        if splat:
            film["weight"] = 3 << 16
        else:
            film["samples"] = 3
        means = (c, c if c * 2 > TOP else 2 * c, c // 2)
        for levels in LEVELS:
            glare = ptss.glare_params(levels=levels, strength=0.37)
            rows = ptss.probe_glare_build(film, w, h, params, glare).view(np.uint64).reshape(-1, 4)
            for k, (lw, lh, first) in enumerate(ptss.glare_layout(w, h, levels)[0], start=1):
                assert (rows[first:first + lw * lh, :3] == np.array([(levels - k + 1) * m for m in means], np.uint64)).all(), (w, h, levels, k)
            mixed = model_mixed(film, w, h, rows, glare)   # MIX: m' = m, and the resolve is the plain one
            assert all(e[:3] == means for e in mixed)
            got = ptss.probe_resolve_glare(film, w, h, rows, params=params, glare=glare)
            plain = (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(film, params=params)
            assert all(same_bytes(a, b) for a, b in zip(got, plain)), (w, h, levels)


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_the_four_bounds_hold_on_the_largest_film(splat):
    """d <= 2^40, u_k <= (L - k + 1) 2^40, g <= 2^40, m' <= 2^41 on films the library filled, and they are reached."""
    params = default_params()
    w, h = 37, 21
    for kind in ("top", "pool"):
        film = film_of(w, h, splat, params, kind=kind)
        if kind == "pool":   # keep what the library can leave: m <= 2^40
            bad = [p for p, e in enumerate(model_means(film)) if max(e[:3]) > TOP]
            film[bad] = film_of(w, h, splat, params, kind="top")[bad]
        downs = model_downs(film, w, h, 0, 8)
        assert max(max(t) for texels, _, _ in downs for t in texels) <= TOP
        for levels in LEVELS:
            ups = model_ups(downs, levels)
            for k, (texels, _, _) in enumerate(ups, start=1):
                assert max(max(t) for t in texels) <= (levels - k + 1) * TOP, (levels, k)
            glare = ptss.glare_params(levels=levels, mode="add", strength=1.0)
            pyr = ptss.probe_glare_build(film, w, h, params, glare)
            assert same_bytes(pyr, pyramid_of(ups))
            L = levels
            u1 = pyr.view(np.uint64).reshape(-1, 4)[:19 * 11, :3]
            assert int(u1.max()) <= L * TOP and all(((int(v) + L // 2) // L) <= TOP for v in (u1.max(),))
            mixed = model_mixed(film, w, h, pyr, glare)
            assert max(max(e[:3]) for e in mixed) <= 2 * TOP
            if kind == "top":
                assert int(u1.min()) == L * TOP and all(e[:3] == (2 * TOP,) * 3 for e in mixed)   # every bound is reached
                mix = model_mixed(film, w, h, pyr, ptss.glare_params(levels=levels, mode="mix", strength=1.0))
                assert all(e[:3] == (TOP,) * 3 for e in mix)
    assert strength_word(1.0) == 65536 and strength_word(0.0) == 0 and strength_word(2.0 ** -16) == 1 and strength_word(2.0 ** -17) == 1 and strength_word(2.0 ** -18) == 0   # + 0.5, truncated: halves go up


def test_impulses_at_a_corner_and_at_the_centre():
    """One level: the down's weights themselves. Texel i takes pixels 2i-1 .. 2i+2 with (1, 3, 3, 1): pixel 4 is tap 3 of texel 1 and tap 1
    of texel 2; pixel 0 is taps 0 and 1 of texel 0 (the clamp) and nobody else's."""
    params = default_params()
    K = 5 << 20
    for splat in (False, True):
        one = ptss.glare_params(levels=1)
        centre = ptss.probe_glare_build(impulse_film(8, 8, 4, 4, 64 * K, splat), 8, 8, params, one)["g"].reshape(4, 4)
        want = np.zeros((4, 4), np.uint64)
        want[1:3, 1:3] = np.array([[1, 3], [3, 9]], np.uint64) * K
        assert np.array_equal(centre, want)
        corner = ptss.probe_glare_build(impulse_film(8, 8, 0, 0, 64 * K, splat), 8, 8, params, one)["b"].reshape(4, 4)
        want = np.zeros((4, 4), np.uint64)
        want[0, 0] = 16 * K
        assert np.array_equal(corner, want)
        far = ptss.probe_glare_build(impulse_film(8, 8, 7, 7, 64 * K, splat), 8, 8, params, one)["r"].reshape(4, 4)
        want = np.zeros((4, 4), np.uint64)
        want[3, 3] = 16 * K   # pixel 7: taps 2 and 3 (the clamped one) of texel 3
        assert np.array_equal(far, want)
        # two levels, by hand: d_2 of the corner impulse is (16 * 16 K + 32) >> 6 = 4 K at texel (0, 0) of 2 x 2, and up(d_2) at texel (0, 0)
        # of level 1 takes 9 + 3 + 3 + 1 = 16 sixteenths of it (all four taps clamp to texel 0 .. but one): the model is the judge
        for x, y in ((0, 0), (4, 4), (7, 0)):
            for levels in (2, 3, 4):
                film = impulse_film(8, 8, x, y, 64 * K + 1, splat)
                glare = ptss.glare_params(levels=levels)
                assert same_bytes(ptss.probe_glare_build(film, 8, 8, params, glare), model_pyramid(film, 8, 8, params, glare)), (x, y, levels)
        two = ptss.probe_glare_build(impulse_film(8, 8, 0, 0, 64 * K, splat), 8, 8, params, ptss.glare_params(levels=2))
        d2 = two["r"][16:].reshape(2, 2)
        assert d2[0, 0] == 4 * K and not d2[0, 1] and not d2[1, 0] and not d2[1, 1]
        u1 = two["r"][:16].reshape(4, 4)
        assert u1[0, 0] == 16 * K + 4 * K and u1[0, 1] == (9 * 4 * K + 3 * 4 * K + 8) >> 4 and u1[1, 1] == (9 * 4 * K + 8) >> 4 and u1[3, 3] == 0


def test_the_threshold_is_rounded_as_a_sample_is():
    params = default_params()
    for th, want in ((0.0, 0), (2.0 ** -21, 0), (3 * 2.0 ** -21, 2), (2.0 ** -20, 1), (1.0, 1 << 20), (2.0 ** 20, 1 << 40), (0.3, None)):
        t = model_threshold(th, params)
        assert want is None or t == want
        film = impulse_film(2, 2, 0, 0, t + 64)
        got = ptss.probe_glare_build(film, 2, 2, params, ptss.glare_params(levels=1, threshold=th))
        assert int(got["r"][0]) == 16   # pixel 0 is taps 0 and 1 of the one texel on both axes, 16 of its 64: (m - t) = 64 is left
        film = impulse_film(2, 2, 0, 0, t)
        assert not ptss.probe_glare_build(film, 2, 2, params, ptss.glare_params(levels=1, threshold=th)).view(np.uint64).any()   # m = t: nothing
