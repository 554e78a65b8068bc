"""Features behind mirrors and glass, without a GPU (ptss_render_features_specular): the new C-ABI symbols, the argument
checks that must not touch a device, the class csrc/ptspecular.h gives every material of every preset against a table derived here
from the rule, and one step of the chain through ptss_probe_specular_step against an independent float64 restatement.

The float64 model is written from the rule (class, sign flip, reflection, Snell's ratio and the refraction vector), not from the
header. Its inputs are random unit directions and normals on both sides of the surface with indices of refraction 1.0 .. 5.8, chosen
with sinT2 outside [0.99, 1.01] so that the branch taken (refraction or total internal reflection) is the model's branch; the
threshold itself is pinned by device = host (tests/test_gpu_specular_features.py). Measured on the host build (x86-64), largest
|host - model| over the 4 x 20,000 cases: direction 2.70e-07 per component (reflection alone 2.58e-07), origin 4.77e-07 (half an
ulp of the |point| <= 10 it is added to). At a front hit a reflection keeps | |d'|^2 - 1 | <= 5.2e-07 and |d' . n + d . n| <=
2.7e-07, a refraction |sin(i) - ior sin(t)| <= 4.9e-07 and | |d'|^2 - 1 | <= 3.1e-07. The tolerances are four times these figures
(DESIGN.md §3.21).

The invariants hold where the reference's expressions are a reflection and a refraction: at a hit from the FRONT (d . n < 0). At a
hit from behind scatter() flips cosI but not the normal, so its reflRay gives d' = d + 2 (d . n) n (d' . n = 3 d . n, |d'|^2 = 1 +
8 (d . n)^2) and its refrRay a direction that is not Snell's; the chain follows the path tracer there too, and the model states it."""
import ctypes as C

import numpy as np
import pytest

import ptss
from ptss_types import Material, Vec3

MEASURED_MAX_DIRECTION = 2.70e-07
MEASURED_MAX_ORIGIN = 4.77e-07
DIRECTION_TOLERANCE = 4 * MEASURED_MAX_DIRECTION
ORIGIN_TOLERANCE = 4 * MEASURED_MAX_ORIGIN
# reflection at a front hit: | |d'|^2 - 1 | and |d' . n + d . n|; refraction at a front hit: |n1 sin(i) - n2 sin(t)| (recorded in §3.21)
MEASURED_MAX_REFLECT_NORM = 5.2e-07
MEASURED_MAX_REFLECT_FLIP = 2.7e-07
MEASURED_MAX_SNELL = 4.9e-07
INF = float("inf")

PRESETS = ("default", "cornell", "lambert", "mixed", "stress", "mesh", "pointlight")


# ---- symbols and argument checks ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    dev, host = C.CDLL(ptss.DEVICE_LIB), C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_render_features_specular", "ptss_specular_feature_launches"):
        assert hasattr(dev, name), name
    assert hasattr(host, "ptss_probe_specular_step")
    assert ptss.device_lib().ptss_version() == 300


def test_argument_checks_without_a_device():
    L = ptss.device_lib()
    buf, steps = (C.c_float * 64)(), (C.c_uint32 * 16)()
    ctx = C.c_void_p(1)   # never dereferenced: every call below fails before the context is looked at
    assert C.addressof(buf) % 16 == 0 and C.addressof(steps) % 4 == 0
    assert L.ptss_render_features_specular(None, 1, buf, steps, None) == -1
    assert L.ptss_render_features_specular(ctx, 1, None, steps, None) == -1
    for bad in (-1, 9, 1 << 20):
        assert L.ptss_render_features_specular(ctx, bad, buf, steps, None) == -1, bad
        assert b"maxSteps" in L.ptss_last_error_detail()
    assert L.ptss_render_features_specular(ctx, 1, C.c_void_p(C.addressof(buf) + 4), steps, None) == -1
    assert L.ptss_render_features_specular(ctx, 1, buf, C.c_void_p(C.addressof(steps) + 2), None) == -1
    out = (C.c_ulonglong * 2)()
    assert L.ptss_specular_feature_launches(None, out) == -1
    assert L.ptss_specular_feature_launches(ctx, None) == -1


def material(diff=0.0, spec=0.0, refr=0.0, exponent=INF, ior=1.5, flags=0):
    m = Material()
    m.diffuseColor = Vec3(1, 1, 1)
    m.specularColor = Vec3(1, 1, 1)
    m.diffAvg, m.specAvg, m.refrAvg, m.specularExponent, m.indexOfRefraction = diff, spec, refr, exponent, ior
    m.flags = bytes([flags])
    return m


def hits_of(normals, material_idx=0, points=None, kind=1):
    h = np.zeros(len(normals), dtype=ptss.HIT_DTYPE)
    h["normal"], h["kind"], h["materialIdx"], h["distance"] = normals, kind, material_idx, 1.0
    if points is not None:
        h["point"] = points
    return h


def test_probe_argument_checks():
    Hh = ptss.host_lib()
    mats = (Material * 2)(material(spec=0.9), material(diff=0.7))
    rays = ptss.make_rays(np.zeros((3, 3)), np.tile([0, 0, -1.0], (3, 1)))
    hits = hits_of(np.tile([0, 0, 1.0], (3, 1)))
    nxt, follows = rays.copy(), (C.c_int * 3)()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)

    def call(r=vp(rays), h=vp(hits), n=3, m=mats, count=2, out=vp(nxt), f=follows):
        return Hh.ptss_probe_specular_step(r, h, n, m, count, out, f)

    assert call() == 0 and list(follows) == [1, 1, 1]
    assert call(r=None, h=None, out=None, f=None, n=0) == 0
    for kw in (dict(r=None), dict(h=None), dict(out=None), dict(f=None), dict(count=0), dict(m=None)):
        assert call(**kw) < 0, kw
    for bad in (2, -1, 1 << 30):
        hits["materialIdx"][1] = bad
        before = nxt.copy()
        assert call() < 0, bad
        assert np.array_equal(nxt, before)
    hits["materialIdx"][1] = 7
    hits["kind"][1] = 0          # a miss is never looked up
    assert call() == 0 and list(follows) == [1, 0, 1]


# ---- the class of every material of every preset ---------------------------------------------------------------------------------
def rule(m):
    """The table of DESIGN.md §3.21, from the material's words."""
    flags = m.flags[0] if isinstance(m.flags, bytes) else int(m.flags)
    if flags & 0x03 == 0x03 or m.diffAvg > 0:
        return "terminal"
    if m.refrAvg > 0:
        return "transmit"
    if m.specAvg > 0 and m.specularExponent == INF:
        return "mirror"
    return "terminal"


def test_class_of_every_preset_material():
    seen = {}
    for preset in PRESETS:
        for k, m in enumerate(ptss.Scene(preset).materials):
            assert ptss.specular_class(m) == rule(m), (preset, k)
            seen[(preset, k)] = ptss.specular_class(m)
    # the named ones (host/Scene.cpp): cornell = the two defined spheres' materials, then the box's five
    assert seen[("cornell", 0)] == "terminal"    # the red Phong sphere (diffAvg 0.35, exponent 250)
    assert seen[("cornell", 1)] == "transmit"    # the Phong-glass of addDefinedSpheres (exponent 300, refrAvg 0.9)
    cornell = ptss.Scene("cornell").materials
    assert cornell[6].flags == b"\x00" and cornell[6].specAvg > 0 and cornell[6].specularExponent == INF
    assert seen[("cornell", 6)] == "mirror"      # the Fresnel-weighted mirror panel: no pure-reflection flag
    default = ptss.Scene("default").materials
    assert [seen[("default", k)] for k in range(3)] == ["terminal"] * 3     # Cook-Torrance
    assert all(default[k].flags == b"\x03" and default[k].specularExponent == INF for k in range(3))
    assert [seen[("default", k)] for k in range(3, 6)] == ["transmit"] * 3  # the three glass() materials
    assert default[10].flags == b"\x01" and seen[("default", 10)] == "mirror"   # the flagged mirror of the mirror box
    assert seen[("default", 6)] == "terminal" and seen[("default", 9)] == "terminal"   # the box's Lambert white, its emitter
    assert set(seen[("lambert", k)] for k in range(len(ptss.Scene("lambert").materials))) == {"terminal"}
    # what no preset has
    assert ptss.specular_class(material(spec=0.5, exponent=40.0)) == "terminal"           # a glossy Phong lobe only
    assert ptss.specular_class(material()) == "terminal"                                     # an absorber
    assert ptss.specular_class(material(spec=0.5, refr=0.5, flags=3)) == "terminal"        # Cook-Torrance wins over glass
    assert ptss.specular_class(material(diff=1e-30, refr=0.5)) == "terminal"
    assert ptss.specular_class(material(refr=0.5)) == "transmit"                           # spec-less glass
    assert ptss.specular_class(material(spec=0.5, flags=1)) == "mirror"


# ---- one step against float64 ---------------------------------------------------------------------------------------------------------
MATERIALS = [material(spec=0.9, flags=1),                  # 0 mirror
             material(spec=0.7, refr=0.7),                 # 1 glass with a specular lobe
             material(refr=0.7),                           # 2 spec-less glass
             material(spec=0.9, refr=0.9, exponent=300)]   # 3 Phong-glass


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cases(seed, n=20000):
    """Unit directions and normals (both sides), points within 10 units, one index of refraction per case in 1.0 .. 5.8."""
    rng = np.random.default_rng(seed)
    return unit(rng, n), unit(rng, n), rng.uniform(-10, 10, size=(n, 3)).astype(np.float32), rng.uniform(1.0, 5.8, size=n).astype(np.float32)


def model(d, nrm, point, ior, spec, refr, exponent):
    """float64: (follows, origin, direction, sinT2, front) per case for a material without a diffuse lobe or Cook-Torrance flag."""
    d, nrm, point, ior = (np.asarray(a, dtype=np.float64) for a in (d, nrm, point, ior))
    cos = -(d * nrm).sum(1)
    front = cos > 0
    n1 = np.where(front, 1.0, ior)
    n2 = np.where(front, ior, 1.0)
    cos = np.abs(cos)
    refl_d = d + 2 * cos[:, None] * nrm
    refl_o = point + nrm * 1e-4
    if refr > 0:
        eta = n1 / n2
        sin_t2 = eta * eta * (1 - cos * cos)
        tir = sin_t2 > 1
        cos_t = np.sqrt(np.where(tir, 0.0, 1 - sin_t2))
        v = eta[:, None] * d + (eta * cos - cos_t)[:, None] * nrm
        w = v / np.linalg.norm(v, axis=1, keepdims=True)
        follows = ~tir | (spec > 0)
        direction = np.where(tir[:, None], refl_d, w)
        origin = np.where(tir[:, None], refl_o, point + w * 1e-4)
        return follows, origin, direction, sin_t2, front
    follows = np.full(len(d), spec > 0 and exponent == INF)
    return follows, refl_o, refl_d, np.zeros(len(d)), front


@pytest.fixture(scope="module")
def stepped():
    """Every material over its own cases, once: (material index, inputs, probe outputs, model outputs, kept)."""
    out = []
    for k, m in enumerate(MATERIALS):
        d, nrm, point, ior = cases(100 + k)
        mats = [material(spec=m.specAvg, refr=m.refrAvg, exponent=m.specularExponent, ior=float(x), flags=m.flags[0]) for x in ior]
        rays = ptss.make_rays(np.zeros_like(d), d)
        hits = hits_of(nrm, np.arange(len(d)), point)
        nxt, follows = ptss.probe_specular_step(rays, hits, mats)
        want = model(d, nrm, point, ior, m.specAvg, m.refrAvg, m.specularExponent)
        kept = (want[3] < 0.99) | (want[3] > 1.01)
        out.append((k, (d, nrm, point, ior, rays), (nxt, follows), want, kept))
    return out


def test_probe_step_against_float64(stepped):
    worst_d = worst_o = worst_reflect = 0.0
    for k, (d, nrm, point, ior, rays), (nxt, follows), (want_f, want_o, want_d, sin_t2, front), kept in stepped:
        assert kept.mean() > 0.95, k
        assert np.array_equal(follows[kept], want_f[kept]), k
        go = kept & follows
        assert go.any()
        assert np.isposinf(nxt[go, 3]).all() and not nxt[go, 7].any()
        err_d = np.abs(nxt[go, 4:7].astype(np.float64) - want_d[go]).max()
        err_o = np.abs(nxt[go, 0:3].astype(np.float64) - want_o[go]).max()
        print(f"material {k}: {go.sum()} steps followed, max |host - model| direction {err_d:.3e}, origin {err_o:.3e}")
        worst_d, worst_o = max(worst_d, err_d), max(worst_o, err_o)
        if k == 0:
            worst_reflect = err_d
        stop = kept & ~follows
        assert nxt[stop].tobytes() == rays[stop].tobytes(), k   # a hit that ends the chain leaves next untouched
    print(f"largest deviation: direction {worst_d:.3e} (reflection alone {worst_reflect:.3e}), origin {worst_o:.3e}")
    assert worst_d <= DIRECTION_TOLERANCE and worst_o <= ORIGIN_TOLERANCE
    assert DIRECTION_TOLERANCE < 1e-3   # beyond that the model and the header are not the same arithmetic


def test_branches_are_all_taken(stepped):
    by = {k: (inp, got, want, kept) for k, inp, got, want, kept in stepped}
    for k in (1, 2, 3):
        _, (_, follows), (_, _, _, sin_t2, front), kept = by[k]
        tir = kept & (sin_t2 > 1)
        assert tir.sum() > 1000 and (kept & ~tir).sum() > 1000 and (tir & front).sum() == 0   # n1 / n2 <= 1 from the front
        assert follows[tir].all() == (k != 2) and (not follows[tir].any()) == (k == 2)   # TIR reflects with a specular lobe, stops without
        assert follows[kept & ~tir].all()
    _, (_, follows), _, _ = by[0]
    assert follows.all()


def test_reflection_invariants(stepped):
    """At a front hit: d' . n = -(d . n), |d'| = 1. At a hit from behind: the reference's d + 2 (d . n) n."""
    worst_norm = worst_flip = 0.0
    for k, (d, nrm, point, ior, rays), (nxt, follows), (_, _, _, sin_t2, front), kept in stepped:
        reflected = follows & kept & ((sin_t2 > 1) if k else np.ones(len(d), dtype=bool))
        d64, n64, got = d.astype(np.float64), nrm.astype(np.float64), nxt[:, 4:7].astype(np.float64)
        dn = (d64 * n64).sum(1)
        f = reflected & front
        if f.any():
            worst_norm = max(worst_norm, np.abs((got[f] ** 2).sum(1) - 1).max())
            worst_flip = max(worst_flip, np.abs((got[f] * n64[f]).sum(1) + dn[f]).max())
        b = reflected & ~front
        if b.any():
            assert np.abs((got[b] * n64[b]).sum(1) - 3 * dn[b]).max() <= 4 * MEASURED_MAX_REFLECT_FLIP * 3
            assert np.abs((got[b] ** 2).sum(1) - (1 + 8 * dn[b] ** 2)).max() <= 4 * MEASURED_MAX_REFLECT_NORM * 9
        if not reflected.any():
            continue
        # the origin leaves along the normal, whichever side
        assert np.abs(nxt[reflected, 0:3].astype(np.float64) - (point[reflected] + n64[reflected] * 1e-4)).max() <= ORIGIN_TOLERANCE
    print(f"reflection at a front hit: max | |d'|^2 - 1 | {worst_norm:.3e}, max |d' . n + d . n| {worst_flip:.3e}")
    assert worst_norm <= 4 * MEASURED_MAX_REFLECT_NORM and worst_flip <= 4 * MEASURED_MAX_REFLECT_FLIP


def test_refraction_satisfies_snell(stepped):
    """At a front hit: sin(t) = sin(i) / ior, d' on the far side, unit length. (From behind the reference's expression is not Snell's.)"""
    worst = worst_norm = 0.0
    for k, (d, nrm, point, ior, rays), (nxt, follows), (_, _, _, sin_t2, front), kept in stepped:
        if k == 0:
            continue
        f = follows & kept & ~(sin_t2 > 1) & front
        assert f.sum() > 1000
        d64, n64, got = d[f].astype(np.float64), nrm[f].astype(np.float64), nxt[f, 4:7].astype(np.float64)
        sin_i = np.linalg.norm(np.cross(d64, n64), axis=1)
        sin_t = np.linalg.norm(np.cross(got, n64), axis=1)
        worst = max(worst, np.abs(sin_i - ior[f].astype(np.float64) * sin_t).max())
        assert ((got * n64).sum(1) < 0).all()
        norm = np.abs((nxt[:, 4:7].astype(np.float64)[follows & kept & ~(sin_t2 > 1)] ** 2).sum(1) - 1).max()   # both sides: normalised
        worst_norm = max(worst_norm, norm)
    print(f"refraction: max |sin(i) - ior sin(t)| {worst:.3e} at a front hit, max | |d'|^2 - 1 | {worst_norm:.3e}")
    assert worst <= 4 * MEASURED_MAX_SNELL
    assert worst_norm <= 4 * MEASURED_MAX_REFLECT_NORM


def test_terminal_hits_misses_and_non_finite_directions_stop():
    mats = [material(spec=0.9, flags=1), material(diff=0.7), material(spec=0.6, diff=0.1, flags=3), material(spec=0.5, exponent=40.0),
            material(), material(spec=0.7, refr=0.7)]
    d = np.tile(np.float32([0.6, 0.0, -0.8]), (9, 1))
    nrm = np.tile(np.float32([0, 0, 1]), (9, 1))
    idx = np.array([0, 1, 2, 3, 4, 5, 0, 0, 5])
    d[6] = [INF, 0, -1]          # a mirror, but d' is not finite
    nrm[7] = [np.nan, 0, 1]
    d[8] = [0.6, np.nan, -0.8]   # glass with a NaN direction: sinT2 is NaN, refrRay's normalise gives NaN
    rays = ptss.make_rays(np.full((9, 3), 3.0), d, tmax=7.0)
    rays[:, 7] = 5.0   # the pad: shows that an untouched row is the caller's
    hits = hits_of(nrm, idx, np.ones((9, 3)))
    nxt, follows = ptss.probe_specular_step(rays, hits, mats)
    assert follows.tolist() == [True, False, False, False, False, True, False, False, False]
    assert nxt[~follows].tobytes() == rays[~follows].tobytes()
    assert np.isposinf(nxt[follows, 3]).all() and not nxt[follows, 7].any()
    assert np.allclose(nxt[0, 4:7], [0.6, 0.0, 0.8], atol=1e-6) and np.allclose(nxt[0, 0:3], [1, 1, 1.0001], atol=1e-6)
    hits["kind"] = 0   # misses
    nxt, follows = ptss.probe_specular_step(rays, hits, mats)
    assert not follows.any() and nxt.tobytes() == rays.tobytes()
