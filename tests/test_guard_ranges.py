"""The range guards the shading code no longer pays per operation rest on membership arguments; each is run here as
a check, in float32, without a GPU: the uniforms' extremes and their sums against the reciprocal's and the root's fast ranges; the
light-sample window's ends against the three operations it stands for, at the ends and one and two ulps either side, with its
one-compare integer form; the bound on an offset's components that makes their upper tests unnecessary; +0 and -0 through the
unguarded Markstein sequence; and the create-time classifier of the scene constants."""
import ctypes as C

import numpy as np
import pytest

import ptss
from guard_scene_common import GUARD_EXPONENT, GUARD_POWERS, GUARD_REFRACTION, GLASS, PHONG, host_guard_flags, room

f32 = np.float32
_f32p = C.POINTER(C.c_float)
NUMERATOR, DIVISOR, RCP_OPERAND, LIGHT_WINDOW = 0, 1, 2, 3


def probe(op, x):
    x = np.ascontiguousarray(x, f32)
    out = np.zeros(x.size, np.uint32)
    assert ptss.host_lib().ptss_probe_guard(op, x.ctypes.data_as(_f32p), out.ctypes.data_as(C.POINTER(C.c_uint)), x.size) == 0
    return out.astype(bool)


@pytest.fixture(scope="module")
def k():
    out = np.zeros(9, f32)
    assert ptss.host_lib().ptss_probe_guard_constants(out.ctypes.data_as(_f32p)) == 0
    names = ("sqrt_lo", "sqrt_hi", "rcp_lo", "rcp_hi", "div_lo", "div_hi", "d2_lo", "d2_hi", "four_pi")
    return dict(zip(names, out))


def ulps(x, n):
    """x moved by n units in the last place (positive finite x)."""
    return (np.asarray(x, f32).view(np.uint32).astype(np.int64) + n).astype(np.uint32).view(f32)


def fma(a, b, c):
    """fma of float32 operands: the product is exact in float64; the one float64 rounding of the sum cannot lift a value over a
    bound that is stated with slack (it is used for bounds only)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def test_the_ranges_are_the_documented_powers_of_two(k):
    assert (k["sqrt_lo"], k["sqrt_hi"]) == (f32(2.0 ** -95), f32(2.0 ** 96))
    assert (k["rcp_lo"], k["rcp_hi"]) == (f32(2.0 ** -125), f32(2.0 ** 126))
    assert (k["div_lo"], k["div_hi"]) == (f32(2.0 ** -60), f32(2.0 ** 60))
    assert k["four_pi"] == f32(4) * f32(3.14159265358979323846)


def uniform(x):
    """ptrng::uniform's mapping of a 32-bit draw: two roundings, no fma (csrc/xorwow.h)."""
    return f32(f32(np.uint32(x)) * f32(2.3283064365386963e-10)) + f32(1.1641532182693481e-10)


def test_uniform_extremes_and_sums_stay_inside_the_fast_ranges(k):
    lo, hi = uniform(0), uniform(2 ** 32 - 1)
    assert lo == f32(2.0 ** -33) and hi == f32(1.0)
    draws = np.concatenate([[0, 1, 2, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], np.random.default_rng(5).integers(0, 2 ** 32, 4096)])
    u = np.array([uniform(int(d)) for d in draws], f32)
    assert u.min() == lo and u.max() == hi                  # the mapping is monotone: the extremes of k are the extremes of u
    assert np.all((u >= k["sqrt_lo"]) & (u < k["sqrt_hi"]))   # sqrt(u2), Lambert sampler
    sums = [f32(f32(a + b) + c) for a in (lo, hi) for b in (lo, hi) for c in (lo, hi)]
    sums += list((u[:-2] + u[1:-1]) + u[2:])
    sums = np.array(sums, f32)
    assert sums.min() >= f32(2.0 ** -32) and sums.max() == f32(3.0)
    assert probe(RCP_OPERAND, sums).all()                    # rcp(u1 + u2 + u3), getAreaLightPoint


def per_operation_guards(x, k):
    """The three guards the window replaces, for distance2 = x: sqrt's range, the divisor sqrt(x) of w_i, the divisor 4 pi x of L_i."""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        root = np.sqrt(x)
        four = (k["four_pi"] * x).astype(f32)
    return (x >= k["sqrt_lo"]) & (x < k["sqrt_hi"]) & probe(DIVISOR, root) & probe(DIVISOR, four)


def test_window_ends_are_the_first_floats_whose_product_reaches_the_division_range(k):
    lo, hi = k["d2_lo"], k["d2_hi"]
    assert f32(k["four_pi"] * lo) >= k["div_lo"] > f32(k["four_pi"] * ulps(lo, -1))
    assert f32(k["four_pi"] * hi) >= k["div_hi"] > f32(k["four_pi"] * ulps(hi, -1))
    assert lo.view(np.uint32) == 0x1fa2f983 and hi.view(np.uint32) - lo.view(np.uint32) == 0x3c000000   # the integer form's constants
    # the other two intervals contain it: sqrt's range, and [2^-120, 2^120) for the divisor sqrt(distance2)
    assert k["sqrt_lo"] < lo and hi < k["sqrt_hi"]
    assert np.sqrt(f32(2.0 ** -120)) == k["div_lo"] and np.sqrt(f32(2.0 ** 120)) == k["div_hi"]
    assert np.sqrt(ulps(f32(2.0 ** -120), -1)) < k["div_lo"] and np.sqrt(ulps(f32(2.0 ** 120), -1)) < k["div_hi"]


def test_window_equals_the_three_guards_at_its_ends_and_everywhere_else(k):
    lo, hi = k["d2_lo"], k["d2_hi"]
    near = np.concatenate([ulps(e, np.arange(-2, 3)) for e in (lo, hi, k["sqrt_lo"], k["sqrt_hi"], f32(2.0 ** -120), f32(2.0 ** 120))])
    want_near = (near >= lo) & (near < hi)
    assert list(want_near[:10]) == [False, False, True, True, True, True, True, False, False, False]
    rng = np.random.default_rng(11)
    exps = np.arange(0, 256, dtype=np.uint32)[:, None] << 23        # every exponent, denormals and inf / NaN included
    mant = np.concatenate([[0, 1, 0x7fffff, 0x7ffffe, 0x400000], rng.integers(0, 1 << 23, 59)]).astype(np.uint32)[None, :]
    pos = (exps | mant).ravel()
    every = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(f32)
    x = np.concatenate([near, -near, every])
    got = probe(LIGHT_WINDOW, x)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got, (x >= lo) & (x < hi))              # the one-compare integer form is the float interval
    guards = per_operation_guards(x, k)
    assert np.array_equal(got, guards)   # inside: every replaced guard holds. Outside: one of them fails (4 pi distance2's), so
    #                                      the guarded path such a wave takes is never a path the window could have spared it


def distance2(o):
    return fma(o[..., 2], o[..., 2], fma(o[..., 1], o[..., 1], (o[..., 0].astype(np.float64) * o[..., 0]).astype(f32)))


def test_offset_components_are_bounded_by_the_window(k):
    rng = np.random.default_rng(17)
    random = (rng.standard_normal((20000, 3)) * np.exp2(rng.uniform(-70, 40, (20000, 1)))).astype(f32)
    edge = np.sqrt(np.float64(k["d2_hi"]))
    dominant = np.array([[s * edge * m, t, -t] for s in (1, -1) for m in (1 - 2.0 ** -20, 1 - 2.0 ** -24, 1, 1 + 2.0 ** -23, 1 + 2.0 ** -20)
                         for t in (0.0, 1e-45, 1e-39, 2.0 ** -60, 1.0)], np.float64).astype(f32)
    huge = np.array([[2.0 ** 60, 1, 1], [1, -2.0 ** 60, 1], [1e30, 0, 0], [np.inf, 1, 1], [1, np.nan, 1], [2.0 ** 59, 2.0 ** 59, 2.0 ** 59]], f32)
    o = np.concatenate([random, np.roll(dominant, 1, axis=1), dominant, huge])
    with np.errstate(all="ignore"):
        d2 = distance2(o)
        inside = probe(LIGHT_WINDOW, d2)
        biggest = np.max(np.abs(o), axis=1)
        # distance2 >= c^2 (1 - 2^-24)^3 for every component c whose square does not underflow
        c2 = biggest.astype(np.float64) ** 2
        assert np.all(d2[inside].astype(np.float64) >= c2[inside] * (1 - 2.0 ** -24) ** 3)
        assert np.all(biggest[inside] < 2.0 ** 28.5 * (1 + 2.0 ** -22))      # ... so far below 2^60: no upper test of a numerator
        assert not inside[-len(huge):].any()                                  # components at or above 2^60 (inf, NaN) fail the window
    assert inside[:20000].any() and (~inside[:20000]).any()
    # the lower tests: one minimum of the magnitudes against 2^-60 is the three tests
    least = np.min(np.abs(o[:-2]), axis=1)
    assert np.array_equal(least >= k["div_lo"], np.all(np.abs(o[:-2]) >= k["div_lo"], axis=1))


def markstein(a, b):
    """ptm::div's fast sequence with r = RN(1 / b)."""
    r = f32(1) / f32(b)
    q0 = f32(a) * r
    rem = fma(-f32(b), q0, f32(a))
    return fma(rem, r, q0)


def test_plus_zero_numerator_keeps_the_fast_path_and_minus_zero_does_not():
    for b in (f32(2.0 ** -60), f32(1.0), f32(12.566371), ulps(f32(2.0 ** 60), -1)):
        assert markstein(f32(0.0), b).view(np.uint32) == 0                          # +0 / b = +0, as IEEE
        assert (f32(-0.0) / b).view(np.uint32) == 0x80000000                        # IEEE: -0
        assert markstein(f32(-0.0), b).view(np.uint32) == 0                         # the sequence: +0 — so -0 stays guarded
        assert markstein(f32(3.0), b) == f32(3.0) / b and markstein(f32(-3.0), b) == f32(-3.0) / b
    # (the callers' divisors are positive: distance and 4 pi distance2 inside the window)


def test_numerator_and_operand_classifiers(k):
    lo, hi = k["div_lo"], k["div_hi"]
    x = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, ulps(lo, -1), lo, -lo, 1.0, -7.5, ulps(hi, -1), hi, -hi, np.inf, -np.inf, np.nan], f32)
    want = [1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    assert list(probe(NUMERATOR, x).astype(int)) == want
    assert list(probe(DIVISOR, x).astype(int)) == [0] + want[1:]                    # a divisor of +0 is not in range
    r = np.array([0.0, 1e-45, ulps(k["rcp_lo"], -1), k["rcp_lo"], -1.0, ulps(k["rcp_hi"], -1), k["rcp_hi"], np.inf, np.nan], f32)
    assert list(probe(RCP_OPERAND, r).astype(int)) == [0, 0, 0, 1, 1, 1, 0, 0, 0]


POWER_CASES = [((60, 60, 60), True), ((20, 0.0, 20), True), ((20, -0.0, 20), False), ((1e-45, 1, 1), False), ((1, 1, 2.0 ** -60), True),
               ((1, 1, 2.0 ** -61), False), ((2.0 ** 60, 1, 1), False), ((2.0 ** 59, 1, 1), True), ((2.0 ** 61, 1, 1), False),
               ((-5, 1, 1), True), ((np.inf, 1, 1), False), ((1, np.nan, 1), False)]


@pytest.mark.parametrize("power,fast", POWER_CASES)
def test_scene_classifier_light_powers(power, fast):
    for scene in (room(area_powers=(power,)), room(area_powers=((1, 1, 1),), point=[((0, 3, -3), power)]),
                  room(area_powers=((60, 60, 60), power))):
        flags = host_guard_flags(scene)
        assert bool(flags & GUARD_POWERS) == fast
        assert flags & GUARD_REFRACTION and flags & GUARD_EXPONENT              # the other verdicts do not depend on the lights


def test_scene_classifier_material_constants():
    assert host_guard_flags(room()) == GUARD_POWERS | GUARD_REFRACTION | GUARD_EXPONENT
    for n, fast in ((1.0, True), (1.5, True), (2.0 ** -60, True), (1e-30, False), (0.0, False), (1e30, False), (2.0 ** 60, False),
                    (-1.5, True), (np.inf, False), (np.nan, False)):
        flags = host_guard_flags(room(ior={GLASS: n}))
        assert bool(flags & GUARD_REFRACTION) == fast, n
        assert flags & GUARD_POWERS and flags & GUARD_EXPONENT
    for e, fast in ((0.0, True), (1.0, True), (1e30, True), (np.inf, True), (-1.0, False), (3e38, False), (-np.inf, False), (np.nan, False),
                    (8e37, True), (9e37, False)):
        flags = host_guard_flags(room(exponent={PHONG: e}))
        assert bool(flags & GUARD_EXPONENT) == fast, e
        assert flags & GUARD_POWERS and flags & GUARD_REFRACTION
