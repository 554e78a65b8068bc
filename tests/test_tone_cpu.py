"""Tone curves for the two linear films without a GPU (ptss_tone_build, ptss_resolve_toned): the record layout against the
header, the exported symbols and the defaults, what the probes refuse, and the host build of csrc/pttone.h (the specification of the
device's table and resolve): the anchor (the clamp with the 2.2 power at 8 bits is ptquant.h's table and the plain, filtered and glare
resolves, byte for byte), the table's order and the bisection's postcondition at every threshold of every curve x transfer x depth over a
grid of white points and filmic coefficients, the literal display value against a float64 restatement of the formulas, and the properties
of the luminance mode, the white point, special inputs and the 10-bit word."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ptss
import ptss_types
from glare_common import film_of
from linear_common import linear_film, params_of, same_words
from meter_common import new_state
from splat_common import splat_film

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
F32 = np.float32

CURVES, TRANSFERS, DEPTHS = ("clamp", "reinhard", "filmic"), ("gamma22", "srgb"), (8, 10)
CONFIGS = [(c, t, b, False) for c in CURVES for t in TRANSFERS for b in DEPTHS]   # (curve, transfer, bits, luminance), default white and filmic[]
LUMINANCE_CONFIGS = [("clamp", "gamma22", 8, True), ("reinhard", "gamma22", 8, True), ("filmic", "srgb", 10, True), ("reinhard", "srgb", 10, True)]
WHITES = (0.25, 1.0, 4.0, 11.2, 128.0)
FILMICS = (ptss.TONE_DEFAULT_FILMIC, (1.0, 0.0, 1.0, 0.0, 1.0), (4.0, 0.5, 3.0, 1.0, 0.2), (1.0, 1.0, 0.0, 1.0, 1.0))
NAN, INF = float("nan"), float("inf")
TONE_REFUSED = (dict(structSize=44), dict(structSize=0), dict(curve=3), dict(curve=-1), dict(transfer=2), dict(transfer=-1), dict(bits=9), dict(bits=0),
                dict(bits=12), dict(flags=2), dict(flags=3), dict(reserved=1), dict(curve=1, white=0.0), dict(curve=1, white=-1.0),
                dict(curve=1, white=65537.0), dict(curve=1, white=NAN), dict(curve=1, white=INF), dict(curve=1, white=1e-30),
                dict(filmic=(-1.0, 0.03, 2.43, 0.59, 0.14)), dict(filmic=(2.51, NAN, 2.43, 0.59, 0.14)), dict(filmic=(2.51, 0.03, INF, 0.59, 0.14)),
                dict(filmic=(2.51, 0.03, 2.43, -0.5, 0.14)), dict(filmic=(2.51, 0.03, 2.43, 0.59, 0.0)), dict(filmic=(2.51, 0.03, 2.43, 0.59, -0.14)),
                dict(filmic=(3e38, 0.03, 3e38, 0.59, 0.14)))   # the last: inf / inf at the saturation bound


def changed(make, **change):
    s = make()
    for k, v in change.items():
        if k == "filmic":
            s.filmic[:] = list(v)
        else:
            setattr(s, k, v)
    return s


def tone_of(cfg, **kw):
    curve, transfer, bits, luminance = cfg
    return ptss.tone_params(curve, transfer, bits, luminance, **kw)


_TABLES = {}


def table_of(cfg):
    """The probe's table of a configuration, built once and left unchanged."""
    if cfg not in _TABLES:
        _TABLES[cfg] = ptss.probe_tone_build(tone_of(cfg))
        _TABLES[cfg].setflags(write=False)
    return _TABLES[cfg]


def literal_level(stage, x):
    """L(x) = (uint)clamp(K v + 0.5, 0, K) in float32 from the probe's literal display value; stage: a tone_params without the flag."""
    K = F32((1 << stage.bits) - 1)
    v = ptss.probe_tone_value(stage, x)
    with np.errstate(invalid="ignore"):
        q = np.minimum(np.maximum(K * v + F32(0.5), F32(0)), K)
    return np.where(np.isnan(q), 0, q).astype(np.uint32)


def stage_of(tone):
    """What a table encodes: the parameters' own curve, or the clamp in luminance mode."""
    s = ptss.tone_params(tone.curve, tone.transfer, tone.bits, False, tone.white, tuple(tone.filmic))
    if tone.flags & ptss.TONE_LUMINANCE:
        s.curve = ptss.TONE_CLAMP
    return s


# ---- layout, symbols, defaults, refusals -------------------------------------------------------------------------------------------------------------
def test_the_struct_equals_the_header(tmp_path):
    fields = ("structSize", "curve", "transfer", "bits", "flags", "white", "filmic", "reserved")
    body = 'printf("%zu\\n", sizeof(ptss_tone_params));' + "".join('printf("%%zu\\n", offsetof(ptss_tone_params, %s));' % f for f in fields)
    body += ('printf("%d %d %d %d %d %u\\n", PTSS_TONE_CLAMP, PTSS_TONE_REINHARD, PTSS_TONE_FILMIC, PTSS_TRANSFER_GAMMA22, PTSS_TRANSFER_SRGB, '
             'PTSS_TONE_LUMINANCE);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { ' + body + ' return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Par = ptss_types.ToneParams
    assert got[0] == C.sizeof(Par) == 48
    assert got[1:9] == [getattr(Par, f).offset for f in fields] == [0, 4, 8, 12, 16, 20, 24, 44]
    assert got[9:] == [ptss.TONE_CLAMP, ptss.TONE_REINHARD, ptss.TONE_FILMIC, ptss.TRANSFER_GAMMA22, ptss.TRANSFER_SRGB, ptss.TONE_LUMINANCE] == [0, 1, 2, 0, 1, 1]
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_libraries_export_the_symbols_and_the_defaults():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_default_tone_params", "ptss_tone_table_floats", "ptss_tone_build", "ptss_resolve_toned", "ptss_tone_launches", "ptss_debug_tone_form"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_tone_build", "ptss_probe_tone_value", "ptss_probe_tone_level", "ptss_probe_resolve_toned"):
        assert hasattr(ptss.host_lib(), name), name
    p = ptss_types.ToneParams()
    assert L.ptss_default_tone_params(C.byref(p)) == 0 and L.ptss_default_tone_params(None) != 0
    assert bytes(p) == bytes(ptss.tone_params())
    assert (p.structSize, p.curve, p.transfer, p.bits, p.flags, p.white, p.reserved) == (48, ptss.TONE_FILMIC, ptss.TRANSFER_SRGB, 8, 0, 4.0, 0)
    assert list(p.filmic) == [float(F32(v)) for v in (2.51, 0.03, 2.43, 0.59, 0.14)]
    assert [L.ptss_tone_table_floats(b) for b in (8, 10, 9, 0)] == [260, 1028, 0, 0] == [ptss.tone_table_floats(8), ptss.tone_table_floats(10), 0, 0]


def test_the_probes_refuse_what_the_calls_refuse():
    Hl = ptss.host_lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    ref = lambda s: C.byref(s) if s is not None else None
    lin, good, glare = ptss.linear_params(), ptss.tone_params(), ptss.glare_params(levels=3)
    film = film_of(5, 4, False, lin)
    pyr = np.zeros((ptss.glare_layout(5, 4, 3)[1], 4), np.uint64)
    table = np.full(260, 7.0, F32)
    x, v, lv = np.ones(4, F32), np.full(4, 3.0, F32), np.full(4, 9, np.uint32)
    out = np.full((20, 4), 3.0, F32)

    def resolve(f=film, kind=0, first=0, count=20, params=lin, tone=good, t=table, w=5, h=4, g=None, p=None):
        return Hl.ptss_probe_resolve_toned(vp(f), kind, first, count, ref(params), ref(tone), vp(t), None, w, h, ref(g), vp(p), vp(out), None, None)

    for change in TONE_REFUSED:
        bad = changed(ptss.tone_params, **change)
        assert Hl.ptss_probe_tone_build(ref(bad), vp(table)) != 0 and Hl.ptss_probe_tone_value(ref(bad), vp(x), vp(v), 4) != 0 and resolve(tone=bad) != 0, change
    assert Hl.ptss_probe_tone_build(None, vp(table)) != 0 and Hl.ptss_probe_tone_build(ref(good), None) != 0
    assert Hl.ptss_probe_tone_value(None, vp(x), vp(v), 4) != 0 and Hl.ptss_probe_tone_value(ref(good), None, vp(v), 4) != 0
    assert Hl.ptss_probe_tone_value(ref(good), vp(x), None, 4) != 0 and Hl.ptss_probe_tone_value(ref(good), None, None, 0) == 0
    for bits in (0, 9, 12):
        assert Hl.ptss_probe_tone_level(vp(table), bits, vp(x), vp(lv), 4) != 0
    assert Hl.ptss_probe_tone_level(None, 8, vp(x), vp(lv), 4) != 0 and Hl.ptss_probe_tone_level(vp(table), 8, None, vp(lv), 4) != 0
    assert Hl.ptss_probe_tone_level(vp(table), 8, vp(x), None, 4) != 0 and Hl.ptss_probe_tone_level(None, 8, None, None, 0) == 0
    assert resolve(f=None) != 0 and resolve(t=None) != 0 and resolve(params=None) != 0 and resolve(tone=None) != 0
    assert resolve(kind=2) != 0 and resolve(kind=-1) != 0 and resolve(g=glare) != 0 and resolve(p=pyr) != 0   # glare and pyramid come together
    for change in (dict(structSize=16), dict(scaleLog2=33), dict(clampMax=0.0), dict(exposure=-0.5), dict(reserved=1)):
        assert resolve(params=changed(ptss.linear_params, **change)) != 0, change
    assert resolve(g=changed(lambda: ptss.glare_params(levels=3), levels=9), p=pyr) != 0
    for w, h in ((0, 4), (5, 0), (2 ** 22 + 1, 1)):
        assert resolve(g=glare, p=pyr, w=w, h=h) != 0
    for first, count in ((0, 21), (20, 1), (2 ** 63, 2 ** 63)):
        assert resolve(g=glare, p=pyr, first=first, count=count) != 0
    assert resolve(first=2 ** 31, count=1) != 0 and resolve(first=0, count=2 ** 31) != 0
    assert (table == 7.0).all() and (v == 3.0).all() and (lv == 9).all() and (out == 3.0).all()   # nothing refused wrote anything
    assert resolve(count=0) == 0 and resolve(f=None, t=None, count=0) == 0 and (out == 3.0).all()
    for tone in (ptss.tone_params("reinhard", white=65536.0), ptss.tone_params("reinhard", white=2.0 ** -60), ptss.tone_params("filmic", filmic=(0, 0, 0, 0, 1e-30)),
                 ptss.tone_params("filmic", filmic=(3e38, 3e38, 0.0, 0.0, 1.0)), ptss.tone_params("clamp", white=NAN, filmic=(NAN,) * 5)):   # unused fields are not looked at
        ptss.probe_tone_build(tone)
    assert resolve(t=ptss.probe_tone_build(good)) == 0 and not (out == 3.0).all()
    assert resolve(t=ptss.probe_tone_build(good), g=glare, p=pyr, w=-1, h=0) != 0 and resolve(t=ptss.probe_tone_build(good), w=-1, h=0) == 0   # read only with a pyramid


def test_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/tone_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host build of
    csrc/pttone.h, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "tone_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "tone_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("tone_sanitize ok"), r.stdout + r.stderr


# ---- the anchor --------------------------------------------------------------------------------------------------------------------------------------
def test_the_anchor_table_is_the_quantisation_table():
    T = table_of(("clamp", "gamma22", 8, False))
    Q = np.zeros(260, F32)
    assert ptss.host_lib().ptss_probe_quant_table(Q.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert T[1:256].tobytes() == Q[1:256].tobytes() and T[0] == -np.inf and np.isnan(T[256]) and T[257] == 0.0 and np.isnan(T[258]) and np.isnan(T[259]) and len(T) == 260


@pytest.mark.parametrize("splat", [False, True], ids=["linear", "splat"])
def test_the_anchor_resolve_is_the_plain_and_the_glare_resolve(splat):
    cfg = ("clamp", "gamma22", 8, False)
    tone, table = tone_of(cfg), table_of(cfg)
    g = np.random.default_rng(11)
    for seed, (w, h) in enumerate(((37, 21), (64, 48), (1, 1))):
        params = params_of(20, 65536.0, exposure=float(F32(g.uniform(0.1, 4.0))))
        film = film_of(w, h, splat, params, seed=seed)
        P = w * h
        words = g.integers(0, 1 << 36, (P, 4), dtype=np.uint64)   # random films beside the adversarial pool
        words[:, 3] = g.integers(0, 5, P, dtype=np.uint64) * (65536 if splat else 1)
        rnd = words.view(ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE).reshape(-1)
        state = new_state()
        state["exposure"] = 0.6
        glare = ptss.glare_params(levels=3, mode="add", threshold=0.25, strength=0.3)
        for f in (film, rnd):
            plain = (ptss.probe_resolve_splat if splat else ptss.probe_resolve_linear)(f, params=params)
            for a, b in zip(ptss.probe_resolve_toned(f, tone, table, params=params), plain):
                assert a.tobytes() == b.tobytes(), (w, h)
            pyr = ptss.probe_glare_build(f, w, h, params, glare)
            for st in (None, state):
                want = ptss.probe_resolve_glare(f, w, h, pyr, params=params, glare=glare, state=st)
                for a, b in zip(ptss.probe_resolve_toned(f, tone, table, params=params, state=st, glare=(w, h, glare, pyr)), want):
                    assert a.tobytes() == b.tobytes(), (w, h, st is None)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------
def check_table(tone, what):
    K = (1 << tone.bits) - 1
    T = ptss.probe_tone_build(tone)
    th = T[1:K + 1]
    nans = np.isnan(th)
    n = int(K - nans.sum())
    assert not nans[:n].any() and nans[n:].all(), what                     # NaNs only at the tail
    assert (np.diff(th[:n]) >= 0).all() and (th[:n] >= 0).all(), what      # non-decreasing, in [+0, +inf]
    assert T[0] == -np.inf and np.isnan(T[K + 1]) and T[K + 2] == 0.0 and np.isnan(T[K + 3]) and np.isnan(T[K + 4]) and ptss.tone_table_sorted(T), what
    stage = stage_of(tone)
    k = np.arange(1, n + 1, dtype=np.uint32)
    below = np.nextafter(th[:n], F32(-np.inf))
    inside = th[:n] > 0   # +0 has no predecessor in [+0, +inf]
    assert (literal_level(stage, th[:n]) >= k).all() and (literal_level(stage, below[inside]) < k[inside]).all(), what   # the bisection's postcondition
    assert (literal_level(stage, F32(np.inf)) == n) or n == K, what          # NaN exactly where L(+inf) < k
    count = lambda v: np.searchsorted(th[:n], v, side="right")                # the number of k with v >= T[k], T sorted
    assert (ptss.probe_tone_level(T, tone.bits, th[:n]) == count(th[:n])).all() and (ptss.probe_tone_level(T, tone.bits, below) == count(below)).all(), what
    if n and (np.diff(th[:n]) > 0).all():   # thresholds all different: level(T[k]) = k, level(prev(T[k])) = k - 1
        assert (ptss.probe_tone_level(T, tone.bits, th[:n]) == k).all() and (ptss.probe_tone_level(T, tone.bits, below[inside]) == k[inside] - 1).all(), what
    return T, n


def test_every_table_is_sorted_and_meets_the_bisections_postcondition():
    for transfer in TRANSFERS:
        for bits in DEPTHS:
            for luminance in (False, True):
                tones = [ptss.tone_params("clamp", transfer, bits, luminance)]
                tones += [ptss.tone_params("reinhard", transfer, bits, luminance, white=w) for w in WHITES]
                tones += [ptss.tone_params("filmic", transfer, bits, luminance, filmic=f) for f in FILMICS]
                for tone in tones:
                    what = (tone.curve, transfer, bits, luminance, tone.white, tuple(tone.filmic))
                    T, n = check_table(tone, what)
                    K = (1 << bits) - 1
                    assert n == K and T[K] < 256.0 and (np.diff(T[1:K + 1]) > 0).all() and T[1] > 0, what   # every level 0 .. K is reachable below 2^8
                    assert (ptss.probe_tone_level(T, bits, np.array([0.0, 256.0], F32)) == [0, K]).all(), what
    for tone in (ptss.tone_params("filmic", "gamma22", 10, filmic=(1.0, 10.0, 2.0, 0.0, 1.0)), ptss.tone_params("filmic", filmic=(0.0, 1.0, 0.0, 1.0, 1.0)),
                 ptss.tone_params("reinhard", white=65536.0, bits=10)):   # curves that end below 1, or reach it late: a NaN tail or large thresholds
        check_table(tone, tuple(tone.filmic))


# ---- the literal display value against float64 ----------------------------------------------------------------------------------------------------------
def model_value(tone, x):
    """transfer(curve(x)) in float64 from the float32 parameters and constants."""
    x = np.minimum(np.maximum(np.asarray(x, np.float64), 0.0), 2.0 ** 40)
    if tone.curve == ptss.TONE_REINHARD:
        r = 1.0 / (float(F32(tone.white)) ** 2)
        c = x * (x * r + 1.0) / (1.0 + x)
    elif tone.curve == ptss.TONE_FILMIC:
        a, b, cc, d, e = (float(v) for v in tone.filmic)
        c = x * (a * x + b) / (x * (cc * x + d) + e)
    else:
        c = x
    c = np.minimum(np.maximum(c, 0.0), 1.0)
    if tone.transfer == ptss.TRANSFER_SRGB:
        return np.where(c <= float(F32(0.0031308)), float(F32(12.92)) * c, float(F32(1.055)) * c ** float(F32(1) / F32(2.4)) - float(F32(0.055)))
    return c ** float(F32(1) / F32(2.2))


# The tolerance, absolute on v in [0, 1]. The curve takes at most 6 float32 roundings (div(1, white * white): 2; fma, multiply, add, divide, or
# three fmas, a multiply and a divide), all of positive terms: a relative error of at most 6 * 2^-24 = 3.6e-7 in c. The power, at most 1 / 2.2,
# shrinks that to 1.7e-7; ptm::pow adds its own relative 1e-6 (tests/test_ptmath.py test_pow_gamma_and_phong); sRGB scales the sum by 1.055
# and adds one rounding of the fma, 6e-8: 1.055 * 1.17e-6 + 6e-8 < 1.3e-6. At the sRGB knee the two branches differ by less than 1e-7.
VALUE_TOLERANCE = 1.5e-6


def test_the_literal_value_equals_the_float64_model():
    g = np.random.default_rng(7)
    x = np.concatenate([np.exp(g.uniform(np.log(1e-7), np.log(100.0), 20000)), [0.0, 1.0, 0.0031308, 4.0, 1e6, 2.0 ** 40, 3e38]]).astype(F32)
    for curve in CURVES:
        for transfer in TRANSFERS:
            for white in (WHITES if curve == "reinhard" else (4.0,)):
                for filmic in (FILMICS if curve == "filmic" else (ptss.TONE_DEFAULT_FILMIC,)):
                    for bits in DEPTHS:
                        tone = ptss.tone_params(curve, transfer, bits, white=white, filmic=filmic)
                        v, m = ptss.probe_tone_value(tone, x).astype(np.float64), model_value(tone, x)
                        what = (curve, transfer, bits, white, filmic)
                        assert np.abs(v - m).max() <= VALUE_TOLERANCE, (what, float(np.abs(v - m).max()))
                        K = (1 << bits) - 1
                        got = ptss.probe_tone_level(ptss.probe_tone_build(tone), bits, x).astype(np.int64)
                        q = K * m + 0.5
                        want = np.floor(np.minimum(np.maximum(q, 0.0), K)).astype(np.int64)
                        near = np.abs(q - np.round(q)) <= K * VALUE_TOLERANCE + K * 2.0 ** -23   # K v + 0.5 in float32: two more roundings
                        assert (np.abs(got - want) <= 1).all() and (got == want)[~near].all(), what


# ---- properties ------------------------------------------------------------------------------------------------------------------------------------------
def one_pixel(r, g, b, scale_log2=20, splat=False):
    f = splat_film(1) if splat else linear_film(1)
    f["r"], f["g"], f["b"] = (int(round(v * (1 << scale_log2))) for v in (r, g, b))
    f["weight" if splat else "samples"] = 65536 if splat else 1
    return f


def test_luminance_mode_keeps_grey_grey_and_channel_ratios():
    params = params_of(20, 65536.0, exposure=1.0)
    g = np.random.default_rng(3)
    for cfg in LUMINANCE_CONFIGS:
        tone, table = tone_of(cfg), table_of(cfg)
        greys = np.concatenate([one_pixel(v, v, v) for v in np.exp(g.uniform(np.log(1e-4), np.log(50.0), 200))])
        px = ptss.probe_resolve_toned(greys, tone, table, params=params)[1]
        lv = ptss.unpack_pixels10(px) if cfg[2] == 10 else px
        assert (lv[:, 0] == lv[:, 1]).all() and (lv[:, 1] == lv[:, 2]).all() and len(np.unique(lv[:, 0])) > 50, cfg
        # the ratios of x_c: history is 255 transfer(clamp(x_c)); below the clamp and on the 2.2 power, (hist_r / hist_g)^2.2 = e_r / e_g
        if cfg[1] == "gamma22":
            rgb = g.uniform(0.05, 0.6, (100, 3))
            film = np.concatenate([one_pixel(*row) for row in rgb])
            lin, _, hist = ptss.probe_resolve_toned(film, tone, table, params=params)
            below = (hist["r"] < 250) & (hist["g"] < 250) & (hist["b"] < 250)
            assert below.sum() > 50
            for a, b in (("r", "g"), ("b", "g")):
                shown = (hist[a][below].astype(np.float64) / hist[b][below]) ** 2.2
                assert np.allclose(shown, lin[a][below].astype(np.float64) / lin[b][below], rtol=2e-5), cfg   # two powers of 1e-6 each, times 2.2, and the products


def test_reinhard_reaches_the_top_level_exactly_at_its_white_point():
    for white in WHITES + (65536.0,):
        for transfer in TRANSFERS:
            for bits in DEPTHS:
                tone = ptss.tone_params("reinhard", transfer, bits, white=white)
                K = (1 << bits) - 1
                T = ptss.probe_tone_build(tone)
                w = F32(white)
                assert ptss.probe_tone_value(tone, np.array([w], F32))[0] >= 1.0 - 2.0 ** -22 and ptss.probe_tone_level(T, bits, np.array([w], F32))[0] == K, (white, transfer, bits)
                assert T[K] <= w and (white > 11.2 or ptss.probe_tone_level(T, bits, np.array([w * F32(0.9)], F32))[0] < K)   # and not much earlier


def test_special_inputs():
    x = np.array([NAN, -0.0, -1.0, -INF, INF, 0.0], F32)
    for cfg in CONFIGS:
        tone, table = tone_of(cfg), table_of(cfg)
        K = (1 << cfg[2]) - 1
        assert ptss.probe_tone_level(table, cfg[2], x).tolist() == [0, 0, 0, 0, K, 0], cfg
        v = ptss.probe_tone_value(tone, x)
        assert np.isnan(v[0]) and v[[1, 2, 3, 5]].tolist() == [0.0, 0.0, 0.0, 0.0] and 1.0 - 2.0 ** -23 <= v[4] <= 1.0, cfg   # curve(+inf) is curve(2^40) (sRGB's 1.055f - 0.055f is an ulp below 1); a negative input shows as 0
        assert not np.isnan(ptss.probe_tone_value(tone, np.array([1e-45, 1e-30, 1e30, 3.4e38], F32))).any(), cfg
    params = params_of(20, 65536.0)
    for cfg in CONFIGS + LUMINANCE_CONFIGS:   # a pixel without samples or weight: the empty row, the alpha bits set
        for splat in (False, True):
            f = splat_film(2) if splat else linear_film(2)
            f["r"], f["g"], f["b"] = 5, 6, 7
            lin, px, hist = ptss.probe_resolve_toned(f, tone_of(cfg), table_of(cfg), params=params)
            assert not lin.view(F32).any() and not hist.view(F32).any(), cfg
            assert (px.view(np.uint32).reshape(-1) == (3 << 30 if cfg[2] == 10 else 255 << 24)).all(), cfg
    state = new_state()
    for exposure in (NAN, 0.0, INF):   # a state's exposure of anything: NaN inputs show level 0, nothing else depends on it
        state["exposure"] = exposure
        for cfg in (("filmic", "srgb", 10, False), ("reinhard", "gamma22", 8, True)):
            lin, px, hist = ptss.probe_resolve_toned(one_pixel(0.5, 0.25, 2.0), tone_of(cfg), table_of(cfg), params=params, state=state)
            lv = (ptss.unpack_pixels10(px) if cfg[2] == 10 else px)[0, :3].tolist()
            K = (1 << cfg[2]) - 1
            assert lin["r"][0] == 0.5 and lv == ([0, 0, 0] if exposure != INF or cfg[3] else [K, K, K]), (exposure, cfg, lv)


def test_ten_bit_words_round_trip():
    g = np.random.default_rng(5)
    rgba = np.concatenate([g.integers(0, 1024, (1000, 3)), g.integers(0, 4, (1000, 1))], axis=1)
    rgba[0], rgba[1] = (1023, 1023, 1023, 3), (0, 0, 0, 0)
    words = ptss.pack_pixels10(rgba)
    assert words.shape == (1000, 4) and words.dtype == np.uint8 and np.array_equal(ptss.unpack_pixels10(words), rgba)
    assert np.array_equal(ptss.unpack_pixels10(words.view(np.uint32).reshape(-1)), rgba)
    cfg = ("filmic", "srgb", 10, False)
    film = film_of(37, 21, False, params_of(20, 65536.0))
    px = ptss.probe_resolve_toned(film, tone_of(cfg), table_of(cfg), params=params_of(20, 65536.0))[1]
    un = ptss.unpack_pixels10(px)
    assert (un[:, 3] == 3).all() and np.array_equal(ptss.pack_pixels10(un), px) and un[:, :3].max() == 1023
    px8 = ptss.probe_resolve_toned(film, tone_of(("filmic", "srgb", 8, False)), table_of(("filmic", "srgb", 8, False)), params=params_of(20, 65536.0))[1]
    assert (px8[:, 3] == 255).all()
