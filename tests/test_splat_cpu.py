"""The filtered linear film without a GPU (ptss_generate_rays_positions / ptss_splat_paths / ptss_splat_paths_homed / ptss_resolve_splat;
DESIGN.md §3.30): the record layouts against the header, the exported symbols and the defaults, and the host build of csrc/ptsplat.h
(the specification of the device's film) against the model of tests/splat_common.py: sample positions recomputed from the streams, the
three filters at four radii over positions on and around every edge that matters, the resolve with the wide division, and the
properties the design rests on — order freedom, homed = scatter, and the box at radius 0.5 = the linear film."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from film_common import advance, films, quant_thresholds, results_of, seeded_states, words
from linear_common import SCALES, params_of
from splat_common import (FH, FW, JITTER_SEED, Model, down, entry, film_words, filters, high_film, homed_positions, model_resolve_splat,
                          model_splat, name_of, positions_of, radiance_rows, resolve_rows, same_words, scatter_case, splat_film, up)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FILTERS = filters()


def test_structs_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes mirrors and the numpy records."""
    fields = (("ptss_film_position", ("x", "y")), ("ptss_splat_filter", ("structSize", "kind", "radius", "alpha", "reserved")),
              ("ptss_splat_entry", ("r", "g", "b", "weight")))
    body = "".join('printf("%%zu\\n", sizeof(%s));' % s for s, _ in fields)
    body += "".join('printf("%%zu\\n", offsetof(%s, %s));' % (s, f) for s, fs in fields for f in fs)
    body += 'printf("%d %d %d\\n", PTSS_SPLAT_BOX, PTSS_SPLAT_TENT, PTSS_SPLAT_GAUSSIAN);'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { ' + body + ' return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Pos, Flt, Ent = ptss_types.FilmPosition, ptss_types.SplatFilter, ptss_types.SplatEntry
    assert got[:3] == [C.sizeof(Pos), C.sizeof(Flt), C.sizeof(Ent)] == [8, 20, 32]
    assert ptss.POSITION_DTYPE.itemsize == 8 and ptss.SPLAT_DTYPE.itemsize == 32
    assert got[3:5] == [Pos.x.offset, Pos.y.offset] == [ptss.POSITION_DTYPE.fields[f][1] for f in ("x", "y")] == [0, 4]
    assert got[5:10] == [getattr(Flt, f).offset for f in fields[1][1]] == [0, 4, 8, 12, 16]
    assert got[10:14] == [getattr(Ent, f).offset for f in fields[2][1]] == [ptss.SPLAT_DTYPE.fields[f][1] for f in fields[2][1]] == [0, 8, 16, 24]
    assert got[14:] == [ptss_types.SPLAT_BOX, ptss_types.SPLAT_TENT, ptss_types.SPLAT_GAUSSIAN] == [0, 1, 2]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_libraries_export_the_symbols_and_the_defaults():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_splat_filter", "ptss_generate_rays_positions", "ptss_splat_paths", "ptss_splat_paths_homed", "ptss_resolve_splat",
                 "ptss_splat_stats"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_film_positions", "ptss_probe_splat_paths", "ptss_probe_resolve_splat"):
        assert hasattr(ptss.host_lib(), name), name
    assert L.ptss_version() == 300
    f = ptss_types.SplatFilter()
    assert L.ptss_default_splat_filter(C.byref(f)) == 0 and L.ptss_default_splat_filter(None) == -1
    assert (f.structSize, f.kind, f.radius, f.alpha, f.reserved) == (20, ptss_types.SPLAT_TENT, 1.0, 2.0, 0)
    assert bytes(ptss.splat_filter()) == bytes(f)
    # refused before anything touches a device
    p = ptss.linear_params()
    cam = ptss.film_camera("pinhole", 4, 4)
    assert L.ptss_generate_rays_positions(None, C.byref(cam), 0, None, 0, None, None, None, None) == -1
    assert L.ptss_splat_paths(None, None, None, 0, None, 4, 4, C.byref(f), C.byref(p), None) == -1
    assert L.ptss_splat_paths_homed(None, None, None, 0, 0, None, 4, 4, C.byref(f), C.byref(p), None) == -1
    assert L.ptss_resolve_splat(None, None, 0, 0, C.byref(p), None, None, None, None) == -1
    assert L.ptss_splat_stats(None, (C.c_ulonglong * 5)()) == -1


def test_the_probes_refuse_what_the_calls_refuse():
    H = ptss.host_lib()
    film, res, pos = splat_film(12), results_of(np.zeros((4, 3), np.float32)), positions_of([(0.5, 0.5)] * 4)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ref = lambda s: C.byref(s) if s is not None else None

    def spl(flt, params=ptss.linear_params(), width=4, height=3, first=None, n=4, results=res, positions=pos, into=film):
        return H.ptss_probe_splat_paths(vp(results) if results is not None else None, vp(positions) if positions is not None else None,
                                        C.byref(C.c_size_t(first)) if first is not None else None, n, vp(into) if into is not None else None,
                                        width, height, ref(flt), ref(params), None, None)

    rsv = lambda params: H.ptss_probe_resolve_splat(vp(film), 0, 12, ref(params), None, None, None)
    good = ptss.splat_filter()
    assert spl(good) == 0 and rsv(ptss.linear_params()) == 0 and spl(None) != 0 and spl(good, None) != 0 and rsv(None) != 0
    for change in (dict(structSize=16), dict(structSize=0), dict(kind=3), dict(kind=-1), dict(radius=float(down(0.5))), dict(radius=float(up(2.0))),
                   dict(radius=0.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(reserved=1), dict(kind=2, alpha=0.0),
                   dict(kind=2, alpha=-1.0), dict(kind=2, alpha=float("inf")), dict(kind=2, alpha=float("nan"))):
        flt = ptss.splat_filter()
        for k, v in change.items():
            setattr(flt, k, v)
        assert spl(flt) != 0, change
    for kind in ("box", "tent"):   # alpha belongs to the Gaussian alone
        for alpha in (0.0, -1.0, float("nan")):
            assert spl(ptss.splat_filter(kind, 1.0, alpha)) == 0
    for radius in (0.5, 2.0):   # the boundary is allowed
        assert spl(ptss.splat_filter("gaussian", radius, 1e-3)) == 0
    for change in (dict(structSize=16), dict(scaleLog2=33), dict(clampMax=0.0), dict(scaleLog2=32, clampMax=257.0), dict(exposure=-0.5), dict(reserved=1)):
        params = ptss.linear_params(clamp_max=2.0 ** 20)
        for k, v in change.items():
            setattr(params, k, v)
        assert spl(good, params) != 0 and rsv(params) != 0, change
    assert spl(good, width=0) != 0 and spl(good, height=0) != 0 and spl(good, width=-4) != 0
    assert spl(good, width=2 ** 22 + 1, height=1, n=0) != 0 and spl(good, width=1, height=2 ** 22 + 1, n=0) != 0
    assert spl(good, width=2 ** 22, height=2 ** 10, n=0) != 0   # 2^32 pixels
    assert spl(good, width=2 ** 22, height=1, n=0) == 0
    assert spl(good, results=None) != 0 and spl(good, positions=None) != 0 and spl(good, into=None) != 0
    assert spl(good, n=0, results=None, positions=None, into=None) == 0
    assert spl(good, first=8) == 0 and spl(good, first=9) != 0 and spl(good, first=13, n=0) != 0   # the homed form: firstPixel + n inside the film
    cam = ptss.film_camera("pinhole", 4, 3)
    rng = seeded_states(1, 4)
    rays, out = np.zeros((4, 8), np.float32), np.zeros((4, 2), np.float32)
    fp = lambda positions: H.ptss_probe_film_positions(C.byref(cam), 0, None, 4, vp(rng), vp(rays), positions, None)
    assert fp(vp(out)) == 0 and fp(None) != 0


def test_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/splat_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host build
    of csrc/ptsplat.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "splat_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "splat_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc"), "-I", host] + srcs +
                   ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("splat_sanitize ok"), r.stdout + r.stderr


# ---- sample positions ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width, height", [(5, 3), (FW, FH)])
def test_positions_are_the_jittered_coordinates_the_ray_is_made_from(width, height):
    n = width * height
    s0 = seeded_states(JITTER_SEED, n)
    for cam in films(width, height):
        rays, rng, pos, dropped = ptss.probe_film_positions(cam, s0)
        want_rays, want_rng, _ = ptss.probe_film_rays(cam, s0)
        assert words(rays).tobytes() == words(want_rays).tobytes() and words(rng).tobytes() == words(want_rng).tobytes() and dropped == 0
        for p in range(n):
            x, y = p % width, p // width
            if cam.jitter:
                _, uni = advance(s0[p], 2)   # the probe's own stream: jx, jy are its first two draws for every model
                want = (np.float32(x) + uni[0], np.float32(y) + uni[1])
            else:
                want = (np.float32(x + 0.5), np.float32(y + 0.5))
            assert (pos["x"][p], pos["y"][p]) == want, (cam.kind, cam.jitter, p)
    # an index: entries that leave the film get NaN positions and keep their ray and stream
    cam = ptss.film_camera("pinhole", width, height, jitter=1)
    index = np.arange(n, dtype=np.uint32)[::-1].copy()
    index[::4] = n + np.arange(len(index[::4]))
    before = np.full((n, 8), 7.0, np.float32)
    rays, rng, pos, dropped = ptss.probe_film_positions(cam, s0, index=index, rays=before)
    want_rays, want_rng, want_dropped = ptss.probe_film_rays(cam, s0, index=index, rays=before)
    out = index >= n
    assert dropped == want_dropped == out.sum() and words(rays).tobytes() == words(want_rays).tobytes() and words(rng).tobytes() == words(want_rng).tobytes()
    assert np.isnan(pos["x"][out]).all() and np.isnan(pos["y"][out]).all() and not np.isnan(pos["x"][~out]).any()


def test_the_seed_of_the_gpu_identity_puts_no_sample_on_an_integer():
    """jitter = 1 draws from (0, 1]: a draw of exactly 1 would put a sample on the next pixel's edge, which a box at radius 0.5 gives to
    that pixel. The GPU test's box identity with jitter uses JITTER_SEED on the FW x FH film and leaves out no sample because of this."""
    s0 = seeded_states(JITTER_SEED, FW * FH)
    for cam in films(FW, FH):
        _, _, pos, _ = ptss.probe_film_positions(cam, s0)
        assert (pos["x"] != np.floor(pos["x"])).all() and (pos["y"] != np.floor(pos["y"])).all()
        assert (np.floor(pos["x"]) == np.arange(FW * FH) % FW).all() and (np.floor(pos["y"]) == np.arange(FW * FH) // FW).all()


# ---- the splat -----------------------------------------------------------------------------------------------------------------------------------
def check_splat(what, res, pos, start, flt, params, model=None, **kw):
    film, dropped, clamped = ptss.probe_splat_paths(res, pos, start, FW, FH, filter=flt, params=params, **kw)
    want, want_dropped, want_clamped = model_splat(res, pos, start, FW, FH, model or flt, params, **kw)
    assert np.array_equal(film_words(film), want), what
    assert (dropped, clamped) == (want_dropped, want_clamped), what
    return film, dropped, clamped


@pytest.mark.parametrize("flt", FILTERS, ids=name_of)
def test_probe_splat_equals_the_model(flt):
    params = ptss.linear_params()
    res, pos = scatter_case()
    model = Model(flt)
    film, dropped, clamped = check_splat("the scatter rows", res, pos, splat_film(), flt, params, model)
    assert dropped >= 13 and clamped > 0 and film["weight"].sum() > 0
    assert dropped < len(pos) - 40
    # q = 2^40 on a film whose sums start at 2^62
    params = params_of(20, 2.0 ** 20)
    top = results_of(np.full((len(pos), 3), 2.0 ** 20, np.float32))
    film, _, clamped = check_splat("2^40 per sample from 2^62", top, pos, high_film(), flt, params, model)
    assert clamped == 0 and int(film["r"].max()) > (1 << 62) + (1 << 37)   # (the narrowest Gaussian's centre tap weighs 0.15)
    over = results_of(np.full((len(pos), 3), 2.0 ** 20 + 1, np.float32))
    assert check_splat("clamped to 2^40", over, pos, high_film(), flt, params, model)[0].tobytes() == film.tobytes()


def test_taps_are_what_the_issue_states_for_single_samples():
    """The rule itself, spelled out: a box at 0.5 owns [i, i + 1); a tent at radius 1 splits a sample bilinearly; integer weights."""
    params = ptss.linear_params()
    one = results_of(np.array([[1.0, 0.5, 0.0]], np.float32))

    def weights(kind, radius, x, y):
        film, dropped, _ = ptss.probe_splat_paths(one, positions_of([(x, y)]), splat_film(), FW, FH, filter=ptss.splat_filter(kind, radius), params=params)
        assert dropped == 0
        return {(int(p) % FW, int(p) // FW): int(film["weight"][p]) for p in np.flatnonzero(film["weight"])}, film

    assert weights("box", 0.5, 3.5, 2.5)[0] == {(3, 2): 65536}
    assert weights("box", 0.5, 3.0, 2.0)[0] == {(3, 2): 65536}                      # on an integer: the pixel at or above
    assert weights("box", 0.5, float(down(3.0)), 2.0)[0] == {(2, 2): 65536}
    assert weights("box", 0.5, float(FW), 2.5)[0] == {}                             # on the film's far edge: the tap is outside
    assert weights("box", 0.5, 0.0, 0.0)[0] == {(0, 0): 65536}
    w, film = weights("tent", 1.0, 3.0, 2.0)                                        # on a corner: four equal taps
    assert w == {(2, 1): 16384, (3, 1): 16384, (2, 2): 16384, (3, 2): 16384}
    assert int(film["r"][2 * FW + 3]) == 1 << 18 and int(film["g"][2 * FW + 3]) == 1 << 17
    assert weights("tent", 1.0, 3.5, 2.5)[0] == {(3, 2): 65536}                     # on a centre: one tap
    assert weights("tent", 1.0, 3.25, 2.5)[0] == {(2, 2): 16384, (3, 2): 49152}
    assert weights("tent", 1.0, 0.0, 0.0)[0] == {(0, 0): 16384}                     # on the film's corner: three taps fall outside
    assert len(weights("box", 2.0, 10.0, 10.0)[0]) == 16 and len(weights("box", 2.0, 10.5, 10.5)[0]) == 16   # at most 4 x 4
    assert len(weights("box", 1.5, 10.25, 10.25)[0]) == 9 and len(weights("gaussian", 2.0, 10.0, 10.0)[0]) <= 16
    q40 = results_of(np.array([[2.0 ** 20, 2.0 ** 20, 2.0 ** 20]], np.float32))
    film, _, _ = ptss.probe_splat_paths(q40, positions_of([(3.5, 2.5)]), splat_film(), FW, FH, filter=ptss.splat_filter("box", 0.5),
                                        params=params_of(20, 2.0 ** 20))
    assert int(film["r"][2 * FW + 3]) == 1 << 40                                     # W = 65536 passes q through


@pytest.mark.parametrize("scale_log2, clamp_max", SCALES[:3])
def test_adversarial_rows_at_every_scale(scale_log2, clamp_max):
    from linear_common import adversarial_results
    params = params_of(scale_log2, clamp_max)
    res = adversarial_results(params)
    g = np.random.default_rng(scale_log2)
    xy = np.stack([g.uniform(-1.0, FW + 1.0, len(res)), g.uniform(-1.0, FH + 1.0, len(res))], axis=1).astype(np.float32)
    xy[::9] = np.round(xy[::9])
    for flt in (ptss.splat_filter("tent", 1.0), ptss.splat_filter("gaussian", 2.0, 1.0), ptss.splat_filter("box", 1.5)):
        _, _, clamped = check_splat((scale_log2, name_of(flt)), res, positions_of(xy), splat_film(), flt, params)
        assert clamped > 0


# ---- the homed form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", FILTERS, ids=name_of)
def test_the_homed_probe_equals_the_model_and_the_scatter_probe_on_the_non_strays(flt):
    params = ptss.linear_params()
    model = Model(flt)
    for first, n in ((0, FW * FH), (FW * 5 + 17, FW * 9 + 11), (3, 1), (FW * FH - 1, 1), (FW * 2 - 1, 2)):
        pos, stray = homed_positions(first, n)
        res = radiance_rows(n, seed=n)
        start = high_film() if n == 1 else splat_film()
        film, dropped, _ = check_splat(("homed", first, n), res, pos, start, flt, params, model, homed_first_pixel=first)
        assert dropped == stray.sum()
        keep = ~stray
        scatter, scatter_dropped, _ = ptss.probe_splat_paths(res[keep], pos[keep], start, FW, FH, filter=flt, params=params)
        assert scatter.tobytes() == film.tobytes() and scatter_dropped == 0, (first, n)


# ---- the resolve ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_log2, clamp_max", SCALES)
@pytest.mark.parametrize("exposure", [0.0, 1.0, 0.37, 40.0])
def test_probe_resolve_equals_the_model(scale_log2, clamp_max, exposure):
    params = params_of(scale_log2, clamp_max, exposure)
    film = resolve_rows(params)
    linear, pixels, history = ptss.probe_resolve_splat(film, params=params)
    want_linear, want_pixels, want_history = model_resolve_splat(film, params)
    assert same_words(linear, want_linear) and np.array_equal(pixels, want_pixels) and same_words(history, want_history)
    empty = film["weight"] == 0
    assert empty.sum() == 2 and not linear.view(np.float32).reshape(-1, 4)[empty].any() and not history.view(np.float32).reshape(-1, 4)[empty].any()
    assert (pixels[empty] == (0, 0, 0, 255)).all() and (pixels[:, 3] == 255).all()
    assert (film["weight"] % 65536 != 0).sum() > 10 and np.array_equal(history["weight"], linear["weight"])
    assert same_words(linear, ptss.probe_resolve_splat(film, params=params_of(scale_log2, clamp_max, 1.0))[0])   # the means do not depend on the exposure
    sub = ptss.probe_resolve_splat(film, first_pixel=3, count=5, params=params, linear=np.full((len(film), 4), -3.0, np.float32), pixels=None)
    rows = sub[0].view(np.float32).reshape(-1, 4)
    assert sub[1] is None and (rows[:3] == -3).all() and (rows[8:] == -3).all() and same_words(sub[0][3:8], linear[3:8])


def test_the_split_division_is_the_wide_one():
    """m = floor((S 2^16 + Wt / 2) / Wt) through the probe, where the mean is exact in float32 (m below 2^24 at scaleLog2 = 0)."""
    params = params_of(0, 2.0 ** 40)
    g = np.random.default_rng(4)
    S = [int(v) for v in g.integers(0, 2 ** 20, 200)] + [0, 1, 255, 2 ** 20]
    Wt = [int(v) for v in g.integers(1, 2 ** 39, 100)] + [int(v) for v in g.integers(1, 2 ** 17, 100)] + [1, 2, 65535, 65536]
    S = [s * w >> 16 if (s * w >> 16) < 2 ** 63 else s for s, w in zip(S, Wt)]
    film = np.concatenate([entry(s, s // 2, min(s + 1, 2 ** 63 - 1), w) for s, w in zip(S, Wt)])
    linear, _, _ = ptss.probe_resolve_splat(film, params=params)
    for k, (s, w) in enumerate(zip(S, Wt)):
        m = ((s << 16) + w // 2) // w
        if m < 2 ** 24:
            assert float(linear["r"][k]) == m, (s, w)


def test_an_exposure_that_puts_the_mean_on_a_threshold():
    T = quant_thresholds()
    for k in (1, 2, 18, 128, 201, 255):
        for x, byte in ((down(T[k]), k - 1), (T[k], k), (up(T[k]), k)):
            params = params_of(20, 65536.0, float(x))
            film = entry((1 << 20) * 3 >> 2, 2 << 20, 1 << 19, 49152)   # mean = 1 exactly, from a weight of 0.75
            _, pixels, _ = ptss.probe_resolve_splat(film, params=params)
            assert pixels[0, 0] == byte and np.array_equal(pixels, model_resolve_splat(film, params)[1]), (k, float(x))


# ---- properties ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_any_permutation_and_any_split_give_the_same_film(seed):
    g = np.random.default_rng(100 + seed)
    flt = FILTERS[(seed * 5 + 1) % len(FILTERS)]
    params = params_of(*SCALES[seed % len(SCALES)])
    res, pos = scatter_case(seed)
    n = len(res)
    start = high_film() if seed % 2 else splat_film()
    whole, dropped, clamped = ptss.probe_splat_paths(res, pos, start, FW, FH, filter=flt, params=params)
    for _ in range(4):
        order = g.permutation(n)
        film, d, c = ptss.probe_splat_paths(res[order], pos[order], start, FW, FH, filter=flt, params=params)
        assert film.tobytes() == whole.tobytes() and (d, c) == (dropped, clamped)
        cut = int(g.integers(0, n + 1))
        first, d1, c1 = ptss.probe_splat_paths(res[order][:cut], pos[order][:cut], start, FW, FH, filter=flt, params=params)
        both, d2, c2 = ptss.probe_splat_paths(res[order][cut:], pos[order][cut:], first, FW, FH, filter=flt, params=params)
        assert both.tobytes() == whole.tobytes() and (d1 + d2, c1 + c2) == (dropped, clamped)


@pytest.mark.parametrize("jitter", [0, 1])
def test_the_box_at_half_a_pixel_is_the_linear_film(jitter):
    """One tap of W = 65536 per sample: r, g, b are ptss_probe_accumulate_linear's sums, weight = 65536 samples, and the resolve gives
    ptss_probe_resolve_linear's bytes — for N = 1 .. 5 samples per pixel, even and odd."""
    P = FW * FH
    box = ptss.splat_filter("box", 0.5)
    params = ptss.linear_params(exposure=0.8)
    cam = ptss.film_camera("pinhole", FW, FH, jitter=jitter)
    rng = seeded_states(JITTER_SEED, P)
    film, linear = splat_film(), np.zeros(P, ptss.LINEAR_DTYPE)
    for k in range(5):
        _, rng, pos, _ = ptss.probe_film_positions(cam, rng)
        assert (pos["x"] != np.floor(pos["x"])).all() and (pos["y"] != np.floor(pos["y"])).all()   # strictly inside the pixels
        res = radiance_rows(P, seed=k)
        for homed in (None, 0):
            got, dropped, clamped = ptss.probe_splat_paths(res, pos, film, FW, FH, filter=box, params=params, homed_first_pixel=homed)
            assert dropped == 0
            if homed is None:
                scatter = got
        assert got.tobytes() == scatter.tobytes()
        film = got
        before = int(linear["clamped"].sum())
        linear, _ = ptss.probe_accumulate_linear(res, linear, params=params)
        assert clamped == int(linear["clamped"].sum()) - before
        assert all(np.array_equal(film[c], linear[c]) for c in "rgb") and np.array_equal(film["weight"], linear["samples"].astype(np.uint64) << 16)
        for a, b in zip(ptss.probe_resolve_splat(film, params=params), ptss.probe_resolve_linear(linear, params=params)):
            assert a.tobytes() == b.tobytes(), k
