"""Ray queries that follow mirrors and glass, without a GPU (ptss_intersect_chain, ptss_lookup_lightmap_chain): the new
C-ABI symbols and the argument checks that must not touch a device; the link factor of csrc/ptspecular.h (ptss_probe_specular_link)
against a float64 model of the rule on four kinds of material; its `next` and `follows` against ptss_probe_specular_step's bytes; step 6
of csrc/ptlightmap.h (ptss_probe_lookup_lightmap_chain) against Python integers; and the sanitizers over a stand-alone program.

The factor's tolerance is a first-order running error bound, evaluated per case from the MODEL's own float64 intermediates and the
operations the header performs (eps = 2^-24, every float32 operation rounds once; model_factor states it line by line), plus one ulp of
the result for the second-order terms: a few ulps where the expressions are well conditioned, more where cosT is small. Cases within 10 %
of the critical angle (sinT2 in (0.9, 1.1)) are left out, so that the branch the float32 code takes is the model's and cosT >= 0.3;
the threshold itself is pinned by device = composition (tests/test_gpu_chain.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ptss
from lightmap_common import EMPTY, FILTERED, FILTERS, FLAGS, modulate_weight, random_map, surfel_hits
from ptss_types import Material
from surface_common import first_difference, same_bytes
from test_lightmap_cpu import lm_params, scattered_hits, sides  # noqa: F401  (sides: a module-scoped fixture)
from test_specular_cpu import hits_of, material

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
EPS = 2.0 ** -24
INF = float("inf")
F32 = np.float32


# ---- symbols and argument checks ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    dev, host = C.CDLL(ptss.DEVICE_LIB), C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_intersect_chain", "ptss_default_chain_options", "ptss_chain_launches", "ptss_lookup_lightmap_chain",
                 "ptss_lightmap_chain_launches"):
        assert hasattr(dev, name), name
    for name in ("ptss_probe_specular_link", "ptss_probe_lookup_lightmap_chain"):
        assert hasattr(host, name), name
    assert ptss.CHAIN_DTYPE.itemsize == 32 and ptss.CHAIN_DTYPE.names == ("throughput", "steps", "direction", "pathLength")
    o = ptss.chain_options()
    assert (o.structSize, o.schedule, o.maxWorkgroups, o.reserved) == (16, 0, 0, 0)
    d = ptss.ChainOptions()
    assert ptss.device_lib().ptss_default_chain_options(C.byref(d)) == 0 and bytes(d) == bytes(o)
    assert ptss.chain_options("refill", 3).schedule == ptss.CHAIN_REFILL == 1 and ptss.chain_options("lane").schedule == ptss.CHAIN_LANE_PER_RAY


def test_argument_checks_without_a_device():
    L = ptss.device_lib()
    buf = (C.c_float * 256)()
    base = C.addressof(buf)
    assert base % 16 == 0
    at = lambda k: C.c_void_p(base + k)
    ctx = C.c_void_p(1)   # never dereferenced: every call below fails before the context is looked at
    rays, hits, chain = at(0), at(256), at(512)   # 2 rays: 64 B, 96 B, 64 B apart
    call = lambda *a: L.ptss_intersect_chain(*a)
    ok = ptss.chain_options("refill", 2)
    assert call(None, rays, 2, 1, None, hits, chain, None) == -1
    assert call(ctx, None, 2, 1, None, hits, chain, None) == -1 and call(ctx, rays, 2, 1, None, None, chain, None) == -1
    for field, value in (("structSize", 12), ("schedule", 2), ("schedule", -1), ("reserved", 1), ("maxWorkgroups", -1)):
        bad = ptss.chain_options("refill", 2)
        setattr(bad, field, value)
        assert call(ctx, rays, 2, 1, C.byref(bad), hits, chain, None) == -1, field
    for k in (4, 8, 12):
        assert call(ctx, at(k), 2, 1, None, hits, chain, None) == -1 and call(ctx, rays, 2, 1, None, at(256 + k), chain, None) == -1
        assert call(ctx, rays, 2, 1, C.byref(ok), hits, at(512 + k), None) == -1
    assert call(ctx, rays, 2, 1, None, at(48), chain, None) == -1      # hits overlap the rays
    assert call(ctx, rays, 2, 1, None, hits, at(32), None) == -1       # chain overlaps the rays
    assert call(ctx, rays, 2, 1, None, hits, at(256 + 80), None) == -1   # chain overlaps the hits
    assert call(ctx, rays, 2, 1, None, hits, hits, None) == -1
    erange = L.ptss_intersect_chain(ctx, rays, 2, 9, None, hits, chain, None)
    assert erange not in (0, -1) and b"maxSteps" in L.ptss_last_error_detail()
    for bad in (-1, 1 << 20):
        assert call(ctx, rays, 2, bad, None, hits, chain, None) == erange
    assert call(ctx, rays, 1 << 31, 1, None, hits, chain, None) == erange
    assert call(ctx, None, 0, 1, None, None, None, None) == 0   # n = 0
    out = (C.c_ulonglong * 2)()
    assert L.ptss_chain_launches(None, out) == -1 and L.ptss_chain_launches(ctx, None) == -1
    assert L.ptss_default_chain_options(None) == -1


# ---- the link factor against a float64 model --------------------------------------------------------------------------------------------
KINDS = {   # (material, what its followed links are)
    "flagged mirror": dict(spec=0.9, flags=1),
    "unflagged mirror": dict(spec=0.8, flags=0),
    "glass with a specular lobe": dict(spec=0.4, refr=0.6),
    "glass without one": dict(refr=1.0),
}
COLOUR = (0.75, 0.5, 0.125)


def kind_material(name, ior):
    m = material(ior=ior, **KINDS[name])
    m.specularColor.x, m.specularColor.y, m.specularColor.z = COLOUR
    return m


def model_factor(m, d, n):
    """The rule in float64 from the float32 inputs -> (follows, reflected, factor (3,), bound (3,), sinT2).
    bound: the first-order running error of the float32 evaluation. Per operation one rounding of relative size eps:
      cosI    three products, two sums of terms whose absolute values add up to at most 1:                      5 eps
      n       one division:                                                                                     eps n
      sinT2   n n (1 - cosI cosI): the square 2 |cosI| dcosI + eps, the difference + eps, n n 3 eps, the product + eps
      cosT    sqrt(1 - sinT2): (dsinT2 + eps) / (2 cosT) + eps cosT
      r       (a - b) / (a + b), a = n1 cosI, b = n2 cosT: da = n1 dcosI + eps a, db = n2 dcosT + eps b; numerator and denominator
              da + db + eps |a -+ b| each; the quotient (dnum + |r| dden) / den + eps |r|
      F       (r_s r_s + r_p r_p) 0.5: 2 |r| dr + eps r r each, the sum + eps
      p       specAvg F: specAvg dF + eps p; refrAvg (1 - F): refrAvg (dF + eps (1 - F)) + eps p
      factor  colour p: colour dp + eps factor"""
    spec, refr, ior, flagged = float(m.specAvg), float(m.refrAvg), float(m.indexOfRefraction), bool(m.flags[0] & 1)
    d, n = d.astype(np.float64), n.astype(np.float64)
    cosI = -float(d @ n)
    d_cosI = 5 * EPS
    if cosI > 0:
        n1, n2 = 1.0, ior
    else:
        cosI, n1, n2 = -cosI, ior, 1.0
    F, dF, sinT2 = 1.0, 0.0, 0.0
    if (spec > 0 and not flagged) or refr > 0:
        eta = n1 / n2
        sinT2 = eta * eta * (1 - cosI * cosI)
        d_sinT2 = eta * eta * (2 * cosI * d_cosI + 2 * EPS) + 4 * EPS * sinT2
        if not sinT2 > 1:
            cosT = np.sqrt(1 - sinT2)
            d_cosT = (d_sinT2 + EPS) / (2 * cosT) + EPS * cosT
            F, dF = 0.0, 0.0
            for (a, da), (b, db) in (((n1 * cosI, n1 * d_cosI + EPS * n1 * cosI), (n2 * cosT, n2 * d_cosT + EPS * n2 * cosT)),
                                     ((n2 * cosI, n2 * d_cosI + EPS * n2 * cosI), (n1 * cosT, n1 * d_cosT + EPS * n1 * cosT))):
                r = (a - b) / (a + b)
                d_num, d_den = da + db + EPS * abs(a - b), da + db + EPS * (a + b)
                dr = (d_num + abs(r) * d_den) / (a + b) + EPS * abs(r)
                F += 0.5 * r * r
                dF += 0.5 * (2 * abs(r) * dr + EPS * r * r)
            dF += EPS * F
    colour = np.array(COLOUR)
    transmit, mirror = refr > 0, refr == 0 and spec > 0
    if mirror or (transmit and sinT2 > 1):
        if transmit and not spec > 0:
            return False, True, None, None, sinT2
        p, dp = (spec, 0.0) if flagged else (spec * F, spec * dF + EPS * spec * F)
        return True, True, colour * p, colour * dp + EPS * colour * p, sinT2
    p = refr * (1 - F)
    dp = refr * (dF + EPS * (1 - F)) + EPS * p
    return True, False, np.full(3, p), np.full(3, dp), sinT2


def link_cases(seed, count):
    """Unit directions and normals with the incidence swept over both sides: normal, oblique, grazing (|cosI| down to 1e-3)."""
    g = np.random.default_rng(seed)
    n = g.normal(size=(count, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    t = np.cross(n, g.normal(size=(count, 3)))
    t /= np.linalg.norm(t, axis=1)[:, None]
    cos = g.uniform(-1, 1, count)
    special = np.array([1.0, -1.0, 1e-3, -1e-3, 1e-2, -1e-2, 0.05, -0.05, 0.999, -0.999, 0.5, -0.5, 0.7, -0.7])
    cos[: 4 * len(special)] = np.tile(special, 4)
    d = -cos[:, None] * n + np.sqrt(1 - cos * cos)[:, None] * t
    d32, n32 = d.astype(F32), n.astype(F32)
    d32 /= np.linalg.norm(d32.astype(np.float64), axis=1)[:, None].astype(F32)
    return d32, n32


@pytest.mark.parametrize("name", list(KINDS))
def test_the_link_factor_equals_the_model(name):
    d, n = link_cases(7, 3000)
    points = np.random.default_rng(3).uniform(-5, 5, size=(len(d), 3)).astype(F32)
    seen = dict(reflected_outside=0, reflected_inside=0, refracted_outside=0, refracted_inside=0, tir_reflected=0, tir_stopped=0, grazing=0)
    worst = 0.0
    for ior in (1.1, 1.5, 2.4):
        m = kind_material(name, ior)
        rays = ptss.make_rays(np.zeros_like(d), d)
        hits = hits_of(n, points=points)
        nxt, follows, factors = ptss.probe_specular_link(rays, hits, [m])
        nxt0, follows0 = ptss.probe_specular_step(rays, hits, [m])
        assert nxt.tobytes() == nxt0.tobytes() and np.array_equal(follows, follows0)   # the very bytes of the step
        assert not factors[~follows].any()
        for i in range(len(d)):
            want_follows, reflected, want, bound, sinT2 = model_factor(m, d[i], n[i])
            cosI = -float(d[i].astype(np.float64) @ n[i].astype(np.float64))
            if 0.9 < sinT2 < 1.1 or abs(cosI) < 1e-4:
                continue   # the branch is the float32 code's to take (module docstring)
            assert bool(follows[i]) == want_follows, (name, ior, i)
            tir = sinT2 > 1 and KINDS[name].get("refr", 0) > 0
            if not want_follows:
                seen["tir_stopped"] += 1
                continue
            tolerance = bound + np.abs(want) * 2 * EPS   # first order, and an ulp of the result for the rest
            err = np.abs(factors[i].astype(np.float64) - want)
            assert (err <= tolerance).all(), (name, ior, i, factors[i], want, err, tolerance)
            worst = max(worst, float((err / np.maximum(tolerance, 1e-300)).max()))
            seen["tir_reflected" if tir else ("reflected" if reflected else "refracted") + ("_outside" if cosI > 0 else "_inside")] += 1
            seen["grazing"] += abs(cosI) < 0.02
            if reflected and KINDS[name].get("flags"):   # a flagged mirror: no Fresnel term at all, the float32 product itself
                assert factors[i].tobytes() == (np.array(COLOUR, dtype=F32) * F32(m.specAvg)).tobytes()
            if not reflected:
                assert factors[i][0] == factors[i][1] == factors[i][2]
    print(f"{name}: {seen}, largest error / bound {worst:.3f}")
    assert seen["grazing"] > 0
    if "mirror" in name:
        assert seen["reflected_outside"] > 1000 and seen["reflected_inside"] > 1000
    else:
        assert seen["refracted_outside"] > 1000 and seen["refracted_inside"] > 100
        assert seen["tir_reflected" if "with a" in name else "tir_stopped"] > 100


def test_a_terminal_material_and_a_miss_have_no_factor():
    d, n = link_cases(9, 64)
    rays = ptss.make_rays(np.zeros_like(d), d)
    nxt, follows, factors = ptss.probe_specular_link(rays, hits_of(n), [material(diff=0.5, spec=0.5)])
    assert not follows.any() and not factors.any() and nxt.tobytes() == rays.tobytes()
    nxt, follows, factors = ptss.probe_specular_link(rays, hits_of(n, kind=0), [kind_material("flagged mirror", 1.5)])
    assert not follows.any() and not factors.any()
    L = ptss.host_lib()
    assert L.ptss_probe_specular_link(None, None, 0, None, 0, None, None, None) == 0
    h = hits_of(n)
    f = np.zeros(len(n), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    mats = (Material * 1)(kind_material("flagged mirror", 1.5))
    assert L.ptss_probe_specular_link(p(rays), p(h), len(h), C.cast(mats, C.c_void_p), 1, p(rays.copy()), f.ctypes.data_as(C.POINTER(C.c_int)), None) != 0


# ---- step 6 of the lookup ----------------------------------------------------------------------------------------------------------------
THROUGHPUTS = [1.0, 0.5, 0.0, -0.0, -1.0, 2.0, 1.0000001, 1e30, INF, -INF, float("nan"), 1.0 / 65536, 0.5 / 65536, 0.25 / 65536, 0.999999,
               0.99999, 1e-30, 0.25, 1.0 / 3.0, 0.1]


def chain_rows(n, seed):
    g = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=ptss.CHAIN_DTYPE)
    rows["throughput"] = g.random((n, 3)).astype(F32)
    pick = g.integers(0, len(THROUGHPUTS), (n, 3))
    special = g.random((n, 3)) < 0.5
    rows["throughput"][special] = np.array(THROUGHPUTS, dtype=F32)[pick[special]]
    rows["steps"], rows["direction"], rows["pathLength"] = g.integers(0, 9, n), g.normal(size=(n, 3)), g.random(n)
    return rows


@pytest.mark.parametrize("filter", FILTERS)
@pytest.mark.parametrize("flags", FLAGS)
def test_step_six_against_python_integers(sides, filter, flags):  # noqa: F811
    s = sides
    params = lm_params(s["W"], s["H"], filter, flags)
    hits = np.concatenate([scattered_hits(len(s["bt"]), len(s["bs"]), 300, 12, len(s["mat"])), surfel_hits(s["tri"], s["sph"], s["points"][::9])])
    chain = chain_rows(len(hits), 5)
    for name, film in (("ordinary", random_map(s["W"], s["H"], s["texels"], 1, ones=0.2)),
                       ("above 2^48", random_map(s["W"], s["H"], s["texels"], 2, big=True, ones=0.2))):
        plain, counts = ptss.probe_lookup_lightmap(s["mat"], hits, film, params, s["bt"], s["bs"])
        got, info = ptss.probe_lookup_lightmap_chain(s["mat"], hits, chain, film, params, s["bt"], s["bs"])
        want = plain.copy()
        for i in np.nonzero(plain["samples"] == 1)[0]:
            for c, ch in enumerate("rgb"):
                want[ch][i] = (int(plain[ch][i]) * modulate_weight(chain["throughput"][i][c]) + 32768) >> 16
        assert same_bytes(got, want), (name, first_difference(got, want))
        assert np.array_equal(info, counts) and info[FILTERED] > 200 and info[EMPTY] > 0   # the four counts and verdicts are unchanged
        if name == "above 2^48":
            assert (got["r"][got["samples"] == 1] >> np.uint64(48)).any()
        # a throughput of exactly (1, 1, 1) gives the plain probe's bytes
        ones = chain.copy()
        ones["throughput"] = 1.0
        same, info1 = ptss.probe_lookup_lightmap_chain(s["mat"], hits, ones, film, params, s["bt"], s["bs"])
        assert same_bytes(same, plain) and np.array_equal(info1, counts), name
    # the counts are added to
    _, info2 = ptss.probe_lookup_lightmap_chain(s["mat"], hits, chain, film, params, s["bt"], s["bs"], info=info)
    assert np.array_equal(info2, 2 * info)


def test_throughputs_that_are_not_in_range(sides):  # noqa: F811
    """Not a number and negative: 0. Above 1: clamped to 1, the plain row."""
    s = sides
    params = lm_params(s["W"], s["H"])
    hits = surfel_hits(s["tri"], s["sph"], s["points"][::5])
    film = random_map(s["W"], s["H"], s["texels"], 4, ones=0.2)
    plain, _ = ptss.probe_lookup_lightmap(s["mat"], hits, film, params, s["bt"], s["bs"])
    assert (plain["samples"] == 1).all() and plain["r"].any()
    for value, what in ((float("nan"), "zero"), (-1.0, "zero"), (-INF, "zero"), (-0.0, "zero"), (0.0, "zero"), (0.25 / 65536, "zero"),
                        (2.0, "plain"), (INF, "plain"), (1.0000001, "plain"), (1e30, "plain"), (1.0, "plain")):
        chain = np.zeros(len(hits), dtype=ptss.CHAIN_DTYPE)
        chain["throughput"] = value
        got, _ = ptss.probe_lookup_lightmap_chain(s["mat"], hits, chain, film, params, s["bt"], s["bs"])
        if what == "plain":
            assert same_bytes(got, plain), value
        else:
            assert (got["samples"] == 1).all() and not (got["r"].any() or got["g"].any() or got["b"].any()), value
    # one channel at a time
    chain = np.zeros(len(hits), dtype=ptss.CHAIN_DTYPE)
    chain["throughput"] = (0.5, float("nan"), 7.0)
    got, _ = ptss.probe_lookup_lightmap_chain(s["mat"], hits, chain, film, params, s["bt"], s["bs"])
    assert np.array_equal(got["r"], (plain["r"] * np.uint64(32768) + np.uint64(32768)) >> np.uint64(16))
    assert not got["g"].any() and np.array_equal(got["b"], plain["b"])


def test_the_chain_probe_refuses_what_the_device_call_refuses(sides):  # noqa: F811
    s = sides
    hits = surfel_hits(s["tri"], s["sph"], s["points"][:8])
    film = random_map(s["W"], s["H"], s["texels"], 4)
    chain = chain_rows(len(hits), 1)
    with pytest.raises(ValueError):
        ptss.probe_lookup_lightmap_chain(s["mat"], hits, chain[:-1], film, lm_params(s["W"], s["H"]), s["bt"], s["bs"])
    bad = lm_params(s["W"], s["H"])
    bad.filter = 2
    with pytest.raises(ptss.PtssError):
        ptss.probe_lookup_lightmap_chain(s["mat"], hits, chain, film, bad, s["bt"], s["bs"])
    L = ptss.host_lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    params, lin = ptss._lightmap_counts(lm_params(s["W"], s["H"]), s["bt"], s["bs"]), ptss.linear_params()
    out = np.zeros((len(hits), 4), dtype=np.uint64)
    mat = np.ascontiguousarray(s["mat"])
    args = lambda chain_ptr, out_ptr: (p(mat), len(mat), C.byref(params), C.byref(lin), p(s["bt"]), p(s["bs"]), p(film), p(hits), chain_ptr, len(hits),
                                      out_ptr, None)
    assert L.ptss_probe_lookup_lightmap_chain(*args(p(chain), p(out))) == 0
    assert L.ptss_probe_lookup_lightmap_chain(*args(None, p(out))) != 0          # a null chain
    assert L.ptss_probe_lookup_lightmap_chain(*args(p(chain), p(chain))) != 0    # out overlaps the chain
    assert L.ptss_probe_lookup_lightmap_chain(*args(p(chain), p(hits))) != 0     # out overlaps the hits
    assert L.ptss_probe_lookup_lightmap_chain(*args(p(chain), p(film))) != 0     # out overlaps the map


# ---- the sanitizers ------------------------------------------------------------------------------------------------------------------
def test_the_probes_run_clean_under_the_sanitizers(tmp_path):
    """tests/csrc/chain_sanitize.cpp, a program of its own over host/*.cpp: address and undefined-behaviour sanitizers on the host builds
    of the link factor and of step 6, every buffer a heap block of the exact size. (Nothing loaded into Python runs under a sanitizer.)"""
    host = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "host")
    exe = tmp_path / "chain_sanitize"
    srcs = [os.path.join(ROOT, "tests", "csrc", "chain_sanitize.cpp")] + [os.path.join(host, f) for f in ("host_capi.cpp", "Scene.cpp", "HostOps.cpp")]
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, "-I", CSRC, "-I", host] + srcs + ["-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("chain_sanitize ok"), r.stdout + r.stderr
