"""Scenes that put every precondition of the once-proven range guards on both sides, HIP path against the oracle,
bit for bit: light powers with +0, -0, denormal, 2^61 and negative components; light samples closer than 2^-30 to the surface and
farther than 2^30 from it (whole rooms scaled so that distance2 straddles an end of the light-sample window, and a light 1e14 away);
refraction indices 1, near 0 and huge; Phong exponents 0, 1e30, inf and -1. Each scene's ptss_guard_flags must be what the
preconditions say, and a scene whose flag is off must still render exactly — through the guarded code, the only code that is exact
for it. Frames are 96 x 64 at S = 2, 4 to 8 bounces, two ticks."""
import numpy as np
import pytest

import oracle
import ptss
from guard_scene_common import (BALLS, FLOOR, GLASS, GUARD_EXPONENT, GUARD_POWERS, GUARD_REFRACTION, LAMP, PHONG, WALL, build,
                                host_guard_flags, room)

pytestmark = pytest.mark.gpu
W, H, S = 96, 64, 2
ALL = GUARD_POWERS | GUARD_REFRACTION | GUARD_EXPONENT


def check(scene, bounces, flags, ticks=2, nan_ok=False):
    r = ptss.Renderer(scene, W, H, max_iterations=bounces, float_accumulator=True, samples_per_pass=S)
    o = oracle.Oracle(scene.desc, W, H, max_iterations=bounces, samples_per_pass=S)
    try:
        assert r.guard_flags() == flags == host_guard_flags(scene)
        for _ in range(ticks):
            r.generate_frame()
            o.generate_frame()
            assert np.array_equal(r.live_counts(), o.live_counts())
        assert np.array_equal(r.accumulator(), o.accumulator())
        assert np.array_equal(r.pixels(), o.pixels())
        f, g = r.float_accumulator(), o.float_sum()
        assert np.array_equal(f, g, equal_nan=True) if nan_ok else np.array_equal(f, g)
        assert r.total_ray_bounces() == o.total_ray_bounces()
        for p in (0, W * H // 3, W * H - 1):
            assert np.array_equal(r.rng_state(p), o.rng_state(p, 0))
        return r.live_counts()
    finally:
        r.close()


def scaled(k):
    """The room with every coordinate and radius multiplied by k (the camera sits at the origin: the view is the same)."""
    s = lambda p: tuple(np.float32(c) * np.float32(k) for c in p)
    tris = [(s(a), s(b), s(c), m) for a, b, c, m in LAMP + FLOOR + WALL]
    return build(spheres=[(s(c), np.float32(r) * np.float32(k), m) for c, r, m in BALLS], triangles=tris, area=[((60, 60, 60), 0)],
                 point=[(s((0.5, 2.5, -3.5)), (40, 40, 40))])


def test_mixed_preset_zero_power_component_keeps_the_flag():
    scene = ptss.Scene("mixed")   # its second area light has power (p / 3, +0, p / 3)
    assert any(0.0 in (a.power.x, a.power.y, a.power.z) for a in scene.desc.areaLights[:scene.desc.numAreaLights])
    counts = check(scene, 8, ALL)
    assert counts[1] > 0


@pytest.mark.parametrize("power,fast", [((20, 0.0, 20), True), ((20, -0.0, 20), False), ((1e-42, 30, 30), False), ((2.0 ** 61, 1, 1), False),
                                        ((-25, 30, -0.5), True)])
def test_light_power_components_on_both_sides(power, fast):
    flags = ALL if fast else ALL & ~GUARD_POWERS
    check(room(area_powers=((60, 60, 60), power)), 5, flags)
    check(room(area_powers=((30, 30, 30),), point=[((0.5, 2.5, -3.5), power)]), 4, flags)


@pytest.mark.parametrize("k", [2.0 ** -34, 2.0 ** -40, 2.0 ** 26, 2.0 ** 31])
def test_light_samples_astride_and_beyond_the_window_ends(k):
    """Room distances are 2 .. 9 units: at 2^-34 and 2^26 distance2 lies on both sides of the window's lower (2^-63.65) and upper
    (2^56.35) end within one frame; at 2^-40 and 2^31 every sample is outside."""
    check(scaled(k), 4, ALL)


def test_a_light_1e14_away():
    far = [((3e13, 1e14, -2e13), (2.0 ** 59, 2.0 ** 59, 2.0 ** 59))]
    check(room(point=far), 5, ALL)
    check(room(point=far + [((0.5, 2.5, -3.5), (40, 40, 40))]), 5, ALL)


@pytest.mark.parametrize("n,fast", [(1.0, True), (1.5, True), (1e-30, False), (1e30, False)])
def test_refraction_indices(n, fast):
    check(room(ior={GLASS: n}), 8, ALL if fast else ALL & ~GUARD_REFRACTION, nan_ok=True)


@pytest.mark.parametrize("e,fast", [(0.0, True), (1e30, True), (np.inf, True), (-1.0, False)])
def test_phong_exponents(e, fast):
    check(room(exponent={PHONG: e}), 6, ALL if fast else ALL & ~GUARD_EXPONENT, nan_ok=True)


def test_set_scene_switches_the_flags_with_the_scene():
    on, off = room(), room(area_powers=((60, 60, 60), (1e-42, -0.0, 2.0 ** 61)), ior={GLASS: 1e30}, exponent={PHONG: -1.0})
    r = ptss.Renderer(on, W, H, max_iterations=5, samples_per_pass=S)
    try:
        assert r.guard_flags() == ALL
        r.generate_frame()
        for scene, flags, seed in ((off, 0, 0xC0FFEE), (on, ALL, 0xBEEF), (off, 0, 0xF00D)):
            r.set_scene(scene)
            assert r.guard_flags() == flags
            r.reseed(seed)
            o = oracle.Oracle(scene.desc, W, H, max_iterations=5, seed=seed, samples_per_pass=S)
            for _ in range(2):
                r.generate_frame()
                o.generate_frame()
                assert np.array_equal(r.live_counts(), o.live_counts())
            assert np.array_equal(r.accumulator(), o.accumulator())
            assert np.array_equal(r.pixels(), o.pixels())
    finally:
        r.close()
