"""Shared deterministic math (csrc/ptmath.h) pinned against libm in float64: the tracer's parity
argument needs these functions to be (a) the same bits on host and device — shown by exhaustion
on the GPU, against this very host build, in tests/test_gpu_math_identity.py — and (b) as accurate
as the CUDA libm the reference used (a few ulp). (b) is checked here on random samples to which the
worst case of every function over ALL float32 patterns of its domain is added: tools/math_accuracy.cpp
found them by exhaustion, profiles/math_accuracy/worst_cases.txt keeps its output (WORST below copies
the patterns, both signs where the function is odd or even). The vector layer's host probe is held
against a float64 model of each formula."""
import ctypes as C
import math

import numpy as np
import pytest

import ptss

_f32p = C.POINTER(C.c_float)
OPS = {"sin": 0, "cos": 1, "tan": 2, "atan": 3, "log": 4, "exp": 5, "pow": 6, "sqrt": 7}


def ev(op, x, y=None):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    yy = np.ascontiguousarray(y, np.float32) if y is not None else None
    rc = ptss.host_lib().ptss_probe_math(OPS[op], x.ctypes.data_as(_f32p),
                                         yy.ctypes.data_as(_f32p) if yy is not None else None,
                                         out.ctypes.data_as(_f32p), x.size)
    assert rc == 0
    return out


def ulp_err(got, ref64):
    ref32 = ref64.astype(np.float32)
    return np.abs(got.astype(np.float64) - ref64) / np.spacing(np.abs(ref32)).astype(np.float64)


RNG = np.random.default_rng(20261004)
RNG_WIDE = np.random.default_rng(20261020)   # the samples over |x| <= 1e4 (a stream of their own: the older samples stay what they were)


def bits(*patterns):
    return np.array(patterns, np.uint32).view(np.float32)


def both_signs(*patterns):
    return bits(*patterns, *(p ^ 0x80000000 for p in patterns))


# profiles/math_accuracy/worst_cases.txt: the pattern with the largest error in each domain (2 pi: |x| <= 2 pi; wide: |x| <= 1e4)
WORST = {
    "sin_2pi": both_signs(0x40697080), "sin_wide": both_signs(0x450efe63),
    "cos_2pi": both_signs(0x40175ae2), "cos_wide": both_signs(0x4530dd0c),
    "tan_2pi": both_signs(0x407aae01), "tan_wide": both_signs(0x4367b21d),
    "atan": both_signs(0x3edd381b), "log": bits(0x3fb4f239), "exp": bits(0xc0bc17a1),
}


def test_sincos_on_sampler_range():
    x = RNG.uniform(0, 2 * math.pi, 400_000).astype(np.float32)  # theta = u * 2 * pi (CudaTracer.cu:536)
    x = np.concatenate([x, WORST["sin_2pi"], WORST["cos_2pi"]])
    assert ulp_err(ev("sin", x), np.sin(x.astype(np.float64))).max() <= 2.0
    assert ulp_err(ev("cos", x), np.cos(x.astype(np.float64))).max() <= 2.0
    x = RNG.uniform(-60, 60, 200_000).astype(np.float32)
    assert np.abs(ev("sin", x) - np.sin(x.astype(np.float64))).max() < 2e-7
    assert np.abs(ev("cos", x) - np.cos(x.astype(np.float64))).max() < 2e-7


def test_sincos_on_the_whole_reduction_range():
    """ptmath.h: "<= 2 ulp for |x| <= 1e4". The exhaustive worst cases are 1.560 (sin) and 1.559 (cos)."""
    x = np.concatenate([RNG_WIDE.uniform(-1e4, 1e4, 400_000).astype(np.float32), WORST["sin_wide"], WORST["cos_wide"], bits(0x461c4000)])
    assert np.abs(x).max() == 1e4
    assert ulp_err(ev("sin", x), np.sin(x.astype(np.float64))).max() <= 2.0
    assert ulp_err(ev("cos", x), np.cos(x.astype(np.float64))).max() <= 2.0


def test_tan():
    """tan = ptm::div(sin, cos): two results of up to 1.56 ulp each and a division. The bounds are the worst cases over every float32
    pattern of the domain, 3.641 ulp for |x| <= 2 pi and 3.764 ulp for |x| <= 1e4 (tools/math_accuracy.cpp; recorded in
    profiles/math_accuracy/worst_cases.txt), rounded up to the next quarter ulp. Sampled as sin is, with those patterns added."""
    x = np.concatenate([RNG_WIDE.uniform(0, 2 * math.pi, 400_000).astype(np.float32), WORST["tan_2pi"]])
    assert np.abs(x).max() <= 2 * math.pi
    assert ulp_err(ev("tan", x), np.tan(x.astype(np.float64))).max() <= 3.75
    x = np.concatenate([RNG_WIDE.uniform(-60, 60, 200_000), RNG_WIDE.uniform(-1e4, 1e4, 400_000)]).astype(np.float32)
    x = np.concatenate([x, WORST["tan_2pi"], WORST["tan_wide"]])
    assert ulp_err(ev("tan", x), np.tan(x.astype(np.float64))).max() <= 4.0
    assert np.array_equal(ev("tan", -x), -ev("tan", x))
    assert ev("tan", [0.0])[0] == 0.0 and np.isnan(ev("tan", [np.inf, 1.0001e4, np.nan])).all()


def test_sincos_exact_points_and_pythagoras():
    assert ev("sin", [0.0])[0] == 0.0 and ev("cos", [0.0])[0] == 1.0
    x = RNG.uniform(0, 2 * math.pi, 100_000).astype(np.float32)
    s, c = ev("sin", x).astype(np.float64), ev("cos", x).astype(np.float64)
    assert np.abs(s * s + c * c - 1).max() < 3e-7


def test_atan():
    x = np.concatenate([RNG.uniform(0, 30, 200_000), 10 ** RNG.uniform(-6, 6, 200_000)]).astype(np.float32)
    x = np.concatenate([x, WORST["atan"]])   # 2.804 ulp: the worst of all finite patterns
    assert ulp_err(ev("atan", x), np.arctan(x.astype(np.float64))).max() <= 3.0
    assert np.array_equal(ev("atan", -x), -ev("atan", x))
    r = ev("atan", [np.inf, -np.inf, 0.0])
    assert r[0] == np.float32(math.pi / 2) and r[1] == -np.float32(math.pi / 2) and r[2] == 0


def test_log():
    x = np.concatenate([RNG.uniform(0, 1, 300_000), 10 ** RNG.uniform(-44, 4, 100_000)]).astype(np.float32)
    x = np.concatenate([x[x > 0], WORST["log"]])   # 0.827 ulp: the worst of all positive finite patterns
    assert ulp_err(ev("log", x), np.log(x.astype(np.float64))).max() <= 1.5
    r = ev("log", [0.0, -1.0, np.inf, 1.0])
    assert r[0] == -np.inf and np.isnan(r[1]) and r[2] == np.inf and r[3] == 0.0


def test_exp():
    x = np.concatenate([RNG.uniform(-87, 10, 400_000).astype(np.float32), WORST["exp"]])   # 1.010 ulp: the worst of [-87.3, 88.7]
    assert ulp_err(ev("exp", x), np.exp(x.astype(np.float64))).max() <= 1.5
    # Beer-Lambert uses exp(-d*a) <= 1: the implementation must never exceed 1 for x <= 0
    x = -(10 ** RNG.uniform(-10, 2, 200_000)).astype(np.float32)
    assert (ev("exp", x) <= 1.0).all()
    r = ev("exp", [0.0, -200.0, 100.0, -np.inf])
    assert r[0] == 1.0 and r[1] == 0.0 and r[2] == np.inf and r[3] == 0.0


def test_pow_gamma_and_phong():
    x = RNG.uniform(0, 1, 400_000).astype(np.float32)
    g = np.float32(1 / 2.2)
    r = ev("pow", x, np.full_like(x, g))
    ref = x.astype(np.float64) ** np.float64(g)
    assert (np.abs(r - ref) / np.maximum(ref, 1e-30)).max() < 1e-6
    assert r.max() <= 1.0
    for e in (250.0, 300.0):  # Scene.cpp:101-105 Phong exponents: y = pow(s, 1/(e+1)) must stay <= 1
        y = np.float32(1) / np.float32(e + 1)
        r = ev("pow", x, np.full_like(x, y))
        assert r.max() <= 1.0
        assert ulp_err(r, x.astype(np.float64) ** np.float64(y)).max() <= 2.0
    assert ev("pow", [0.0, 1.0, 0.5], [g, g, 0.0]).tolist() == [0.0, 1.0, 1.0]


def test_nan_policy():
    for op in ("sin", "cos", "atan", "log", "exp"):
        assert np.isnan(ev(op, [np.nan]))[0], op
    assert np.isnan(ev("sin", [np.inf, 1e9])).all()  # outside the reduction range -> NaN, never garbage
    assert np.isnan(ev("pow", [-1.0, np.nan], [0.5, 0.5])).all()


def test_tracer_constants():
    # s = -2 * tan(fov / 2) with fov = pi/2 (CudaTracer.cu:334): within 1 ulp of 1
    t = ev("tan", [np.float32(math.pi) / np.float32(2) * np.float32(0.5)])[0]
    assert abs(float(t) - 1.0) <= 1.2e-7
    assert ev("sqrt", [2.0])[0] == np.float32(math.sqrt(2.0))


def test_tone_map_threshold_table_describes_the_literal_function():
    """csrc/ptquant.h: T[k] is the smallest float whose 8-bit sample is >= k. Checked here on the host: the table is
    strictly increasing, each threshold and its predecessor float sit on the two sides of a step, and resolving random
    radiances through the table (searchsorted) reproduces the literal clamp / pow / scale function. The device form
    (hardware guess + two compares) is proven against the literal one for all 2^32 patterns in tests/test_gpu_math.py."""
    import ctypes as C
    L = ptss.host_lib()
    T = np.zeros(257, np.float32)
    assert L.ptss_probe_quant_table(T.ctypes.data_as(_f32p)) == 0
    assert T[0] == -np.inf and np.isnan(T[256]) and np.all(np.diff(T[1:256]) > 0) and 0 < T[1] and T[255] < 1

    def literal(x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.zeros(x.size, np.uint32)
        assert L.ptss_probe_quantize(x.ctypes.data_as(_f32p), out.ctypes.data_as(C.POINTER(C.c_uint)), x.size) == 0
        return out

    at = T[1:256]
    below = np.nextafter(at, np.float32(-1), dtype=np.float32)
    assert np.array_equal(literal(at), np.arange(1, 256)) and np.array_equal(literal(below), np.arange(0, 255))
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(200000, np.float32), rng.random(50000, np.float32) ** 8, np.float32([0, 1, -1, 2, np.inf, -np.inf, np.nan, 1e-30, 0.5])])
    want = literal(x)
    via_table = np.where(np.isnan(x), 0, np.searchsorted(T[1:256], x, side="right")).astype(np.uint32)
    assert np.array_equal(via_table, want)
    assert want[-3] == 0 and want[200000 + 50000 + 1] == 255 and want[200000 + 50000 + 6] == 0  # 1e-30, 1.0, NaN


def test_worst_case_points_and_tan_bounds_are_the_recorded_ones():
    """The patterns in WORST and the two tan bounds come from profiles/math_accuracy/worst_cases.txt (the output of
    tools/math_accuracy.cpp), and every recorded worst case is within the bound its test asserts."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "math_accuracy", "worst_cases.txt")
    rows = {}
    for line in open(path).read().splitlines()[1:]:
        f, domain, count, ulp, pattern = line.split()
        rows[(f, domain)] = (int(count), float(ulp), int(pattern, 16))
    keys = {"sin_2pi": ("sin", "|x|<=2pi"), "sin_wide": ("sin", "|x|<=1e4"), "cos_2pi": ("cos", "|x|<=2pi"), "cos_wide": ("cos", "|x|<=1e4"),
            "tan_2pi": ("tan", "|x|<=2pi"), "tan_wide": ("tan", "|x|<=1e4"), "atan": ("atan", "finite"), "log": ("log", "0<x<inf"),
            "exp": ("exp", "-87.3<=x<=88.7")}
    assert set(rows) == set(keys.values())
    for name, key in keys.items():
        assert rows[key][2] in WORST[name].view(np.uint32).tolist(), name
    asserted = {"sin": 2.0, "cos": 2.0, "atan": 3.0, "log": 1.5, "exp": 1.5}
    for (f, domain), (count, ulp, _) in rows.items():
        if f == "tan":
            assert math.ceil(ulp * 4) / 4 == {"|x|<=2pi": 3.75, "|x|<=1e4": 4.0}[domain]
        else:
            assert ulp <= asserted[f], (f, domain)
    assert rows[("atan", "finite")][0] == 2 ** 32 - 2 ** 24 and rows[("log", "0<x<inf")][0] == 0x7f800000 - 1   # every finite pattern


# ---- the vector layer's host probe against a float64 model of each formula -------------------------------------------------------------
VECTOR_OPS = ["dot", "cross", "div_scalar", "madd_scalar", "madd_vector", "rotate", "quat_mul", "normalize_vec3", "normalize_quat", "length"]


def ev_vector(op, cases):
    cases = np.ascontiguousarray(cases, np.float32)
    out = np.full((len(cases), 4), np.nan, np.float32)
    assert ptss.host_lib().ptss_probe_vector(op, cases.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p), len(cases)) == 0
    return out


def test_vector_probe_refusals():
    L = ptss.host_lib()
    a, o = np.zeros(12, np.float32), np.zeros(4, np.float32)
    pa, po = a.ctypes.data_as(_f32p), o.ctypes.data_as(_f32p)
    assert L.ptss_probe_vector(0, pa, po, 1) == 0
    assert L.ptss_probe_vector(0, None, po, 1) == -1 and L.ptss_probe_vector(0, pa, None, 1) == -1
    assert L.ptss_probe_vector(-1, pa, po, 1) == -1 and L.ptss_probe_vector(len(VECTOR_OPS), pa, po, 1) == -1
    assert L.ptss_probe_vector(0, pa, po, 0) == 0


@pytest.mark.parametrize("name", VECTOR_OPS)
def test_vector_probe_against_a_float64_model(name):
    """The rule of tests/test_reference_functions.py for floats (reference_common.distance_ulp): the distance in float32 ulps of the
    result's largest component, with a floor at the magnitude of the terms the result is a sum of. The bound per operation counts
    the roundings of the formula in ptmath.h: a rounding is at most half an ulp of a value no larger than the floor, and half an ulp
    is allowed on top for a value that rounds up into the next binade (the unit is taken from the exact result).
      dot: product, fma, fma = 3 roundings -> 2.   cross: product, fma per component = 2 -> 1.5.   vec3 / float, both madd: 1 -> 1.
      quat_mul: 4 products, 3 sums per component = 7 -> 4.
      length: |v|^2 carries 3 roundings without cancellation, relative 3u (u = 2^-24); the root halves that and rounds: 2.5u; a relative
      error of k u is at most k ulp -> 3.   normalize(vec3): the reciprocal and the product round once more each: 4.5u -> 5.
      normalize(quat): four terms, 4u -> 3u -> 4u -> 5u -> 5.5.
      rotate, v + 2w (u x v) + 2 (u x (u x v)) with the floor F = |v| (1 + 2 |w| |u| + 2 |u|^2): u x v carries 1 ulp of |u| |v|; times
      2w (exact) and rounded: 2 |w| + 0.5; u x (u x v) inherits sqrt(2) |u| times that ulp and adds 1 of its own, doubled: 2 (1.42 + 1); the
      two sums round once each: 1. Together 2 + 0.5 + 4.84 + 1 = 8.34 ulp of values no larger than F -> 9."""
    from reference_common import distance_ulp
    op = VECTOR_OPS.index(name)
    rng = np.random.default_rng(1000 + op)
    n = 10_000
    c = (rng.uniform(-4, 4, (n, 12)) * 10 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    if name in ("rotate", "quat_mul"):   # rotations: quaternions near unit length (x, y, z, w), as the tracer's are
        for q in (slice(0, 4),) + ((slice(4, 8),) if name == "quat_mul" else ()):
            v = rng.normal(size=(n, 4))
            c[:, q] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    d = c.astype(np.float64)
    a, b, p = d[:, 0:3], d[:, 3:6], d[:, 0:4]
    norm = lambda v: np.sqrt((v * v).sum(axis=1))
    used, floor = 3, 0.0
    if name == "dot":
        model, floor, bound, used = (a * b).sum(axis=1)[:, None], np.abs(a * b).sum(axis=1), 2.0, 1
    elif name == "cross":
        model, floor, bound = np.cross(a, b), (np.abs(a[:, [1, 2, 0]] * b[:, [2, 0, 1]]) + np.abs(a[:, [2, 0, 1]] * b[:, [1, 2, 0]])).max(axis=1), 1.5
    elif name == "div_scalar":
        model, bound = a / d[:, 3:4], 1.0
    elif name == "madd_scalar":
        model, floor, bound = a * d[:, 3:4] + d[:, 4:7], (np.abs(a * d[:, 3:4]) + np.abs(d[:, 4:7])).max(axis=1), 1.0
    elif name == "madd_vector":
        model, floor, bound = a * b + d[:, 6:9], (np.abs(a * b) + np.abs(d[:, 6:9])).max(axis=1), 1.0
    elif name == "rotate":
        u, w, v = d[:, 0:3], d[:, 3:4], d[:, 4:7]
        uv = np.cross(u, v)
        model, floor, bound = v + 2 * w * uv + 2 * np.cross(u, uv), norm(v) * (1 + 2 * np.abs(w[:, 0]) * norm(u) + 2 * norm(u) ** 2), 9.0
    elif name == "quat_mul":
        q = d[:, 4:8]
        px, py, pz, pw = p.T
        qx, qy, qz, qw = q.T
        terms = np.array([[pw * qx, px * qw, py * qz, -pz * qy], [pw * qy, py * qw, pz * qx, -px * qz], [pw * qz, pz * qw, px * qy, -py * qx],
                          [pw * qw, -px * qx, -py * qy, -pz * qz]])   # x, y, z, w
        model, floor, bound, used = terms.sum(axis=1).T, np.abs(terms).sum(axis=1).max(axis=0), 4.0, 4
    elif name == "normalize_vec3":
        model, bound = a / norm(a)[:, None], 5.0
    elif name == "normalize_quat":
        model, bound, used = p / norm(p)[:, None], 5.5, 4
    else:
        model, bound, used = norm(a)[:, None], 3.0, 1
    got = ev_vector(op, c)
    assert np.all(got[:, used:] == 0) and not np.signbit(got[:, used:]).any()      # results the operation does not have: +0
    dist = distance_ulp(got[:, :used], model, model, floor if np.isscalar(floor) else floor[:, None], True)
    print(f"{name}: largest distance {dist.max():.3f} ulp (bound {bound})")
    assert not np.isnan(dist).any() and dist.max() <= bound
