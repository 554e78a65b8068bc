"""The film of a path query without a GPU (ptss_generate_rays / ptss_accumulate_paths / ptss_ray_features): the record
layouts against the header, the exported symbols, the host build of csrc/ptcamera.h (the specification of the device's rays) against
ptss_camera_ray, against an independent float64 model and against geometry, the host accumulation against the oracle's tone map, and
the condition under which the frame identity of tests/test_gpu_film.py holds."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
import ptss
import ptss_types
from film_common import (FRAMES, LENS, adversarial_radiance, advance, films, frames_of, oracle_state_after, results_of, seeded_states, turned_camera,
                         words)
from path_query_common import CASES, H, W, satisfies_identity_condition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
U = 2.0 ** -24   # the unit roundoff of float32


def test_dtypes_equal_the_header(tmp_path):
    """sizeof / offsetof as a C compiler sees include/ptss_types.h, against the ctypes and numpy mirrors."""
    fields = ("structSize", "kind", "camera", "width", "height", "lensRadius", "focusDistance", "jitter")
    entry = ("r", "g", "b", "samples")
    body = "".join('printf("%%zu\\n", offsetof(ptss_film_camera, %s));' % f for f in fields)
    body += "".join('printf("%%zu\\n", offsetof(ptss_film_entry, %s));' % f for f in entry)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "ptss_types.h"\nint main(void) { printf("%zu\\n%zu\\n", sizeof(ptss_film_camera), '
                   'sizeof(ptss_film_entry)); ' + body + ' printf("%d %d %d\\n", PTSS_FILM_PINHOLE, PTSS_FILM_THIN_LENS, PTSS_FILM_EQUIRECT); return 0; }\n')
    exe = tmp_path / "layout"
    cc = shutil.which("gcc") or shutil.which("cc")
    subprocess.run([cc, "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)   # (C11: the header's _Static_asserts take part)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F, E = ptss_types.FilmCamera, ptss_types.FilmEntry
    assert got[:2] == [C.sizeof(F), C.sizeof(E)] == [68, 16]
    assert got[2:10] == [getattr(F, f).offset for f in fields] == [0, 4, 8, 48, 52, 56, 60, 64]
    assert got[10:14] == [getattr(E, f).offset for f in entry] == [ptss_types.FILM_DTYPE.fields[f][1] for f in entry] == [0, 4, 8, 12]
    assert got[14:] == [ptss.FILM_PINHOLE, ptss.FILM_THIN_LENS, ptss.FILM_EQUIRECT] == [0, 1, 2]
    assert ptss_types.FILM_DTYPE.itemsize == 16
    assert "#define PTSS_VERSION 300" in open(os.path.join(INC, "ptss.h")).read()   # no existing struct changed


def test_libraries_export_the_symbols():
    L = ptss.device_lib()   # loads without a GPU
    for name in ("ptss_generate_rays", "ptss_accumulate_paths", "ptss_ray_features", "ptss_film_launches", "ptss_film_rejected"):
        assert hasattr(L, name), name
    for name in ("ptss_probe_film_rays", "ptss_probe_accumulate"):
        assert hasattr(ptss.host_lib(), name), name
    assert L.ptss_version() == 300
    film = ptss.film_camera("pinhole", 4, 4)
    # refused before anything touches a device
    assert L.ptss_generate_rays(None, C.byref(film), 0, None, 0, None, None, None) == -1
    assert L.ptss_accumulate_paths(None, None, None, 0, 0, None, 16, None, None, None) == -1
    assert L.ptss_ray_features(None, None, None, 0, None) == -1
    assert L.ptss_film_launches(None, (C.c_ulonglong * 3)()) == -1
    assert L.ptss_film_rejected(None, C.byref(C.c_ulonglong())) == -1


# ---- the pinhole is ptss_camera_ray --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(64, 48), (5, 3), (3, 64), (1, 1)])
def test_pinhole_is_camera_ray_bit_for_bit(width, height):
    cam, seed = turned_camera(), 0xFEED
    n = width * height
    s0 = seeded_states(seed, n)
    film = ptss.film_camera("pinhole", width, height, cam)
    rays, after, rejected = ptss.probe_film_rays(film, s0)
    assert rejected == 0
    q = ptss.RayQuery()
    buf = (C.c_float * 8).from_buffer(q)
    for p in range(n):
        state2, uni = oracle_state_after(seed, p, 2)   # the stream's two draws, and the state behind them, on the oracle
        assert ptss.host_lib().ptss_camera_ray(C.byref(cam), width, height, p % width, p // width, C.c_float(uni[0]), C.c_float(uni[1]), C.byref(q)) == 0
        assert np.array_equal(words(rays)[p], np.array(buf, dtype=np.float32).view(np.uint32)), p
        assert np.array_equal(words(after)[p], state2), p
    assert (rays["tmax"] == np.inf).all() and (rays["pad"] == 0).all()
    # jitter = 0: the pixel centre, no draw
    rays0, after0, _ = ptss.probe_film_rays(ptss.film_camera("pinhole", width, height, cam, jitter=0), s0)
    assert np.array_equal(words(after0), s0)
    for p in (0, n // 2, n - 1):
        assert ptss.host_lib().ptss_camera_ray(C.byref(cam), width, height, p % width, p // width, C.c_float(0.5), C.c_float(0.5), C.byref(q)) == 0
        assert np.array_equal(words(rays0)[p], np.array(buf, dtype=np.float32).view(np.uint32)), p


def test_draw_counts_and_pixel_addressing():
    cam, seed, n = turned_camera(), 5, 40
    s0 = seeded_states(seed, n)
    for film in films(7, 9, cam):
        want = {ptss.FILM_PINHOLE: 2, ptss.FILM_THIN_LENS: 4, ptss.FILM_EQUIRECT: 2}[film.kind] if film.jitter else 0
        assert ptss.film_draws(film) == want
        rays, after, _ = ptss.probe_film_rays(film, s0, first_pixel=11)
        for i in (0, 17, n - 1):
            assert np.array_equal(words(after)[i], advance(s0[i], want)[0]), (film.kind, film.jitter, i)
            assert np.array_equal(words(after)[i], oracle_state_after(seed, i, want)[0]), (film.kind, film.jitter, i)
        # an index names the same pixels; entries beyond the film write nothing and are counted
        index = np.arange(11, 11 + n, dtype=np.uint32)
        index[[3, 29]] = (63, 2 ** 32 - 1)   # 7 * 9 = 63 pixels: both leave the film
        marked = np.full((n, 8), 7.5, dtype=np.float32)
        rays_i, after_i, rejected = ptss.probe_film_rays(film, s0, index=index, rays=marked)
        keep = np.ones(n, bool)
        keep[[3, 29]] = False
        assert rejected == 2
        assert np.array_equal(words(rays_i)[keep], words(rays)[keep]) and np.array_equal(words(after_i)[keep], words(after)[keep])
        assert np.array_equal(words(rays_i)[~keep], words(marked)[~keep]) and np.array_equal(words(after_i)[~keep], s0[~keep])
    # refusals of the probe: the device call's, alignment aside
    bad = [dict(kind=3), dict(jitter=2), dict(width=0), dict(height=-1), dict(structSize=64)]
    lens = [dict(lensRadius=-0.1), dict(focusDistance=0.0), dict(lensRadius=float("inf")), dict(focusDistance=float("nan"))]
    for kind, changes in (("pinhole", bad), ("thinlens", bad + lens)):
        for change in changes:
            film = ptss.film_camera(kind, 7, 9, cam, **LENS)
            for k, v in change.items():
                setattr(film, k, v)
            with pytest.raises(ptss.PtssError):
                ptss.probe_film_rays(film, s0)
    with pytest.raises(ptss.PtssError):
        ptss.probe_film_rays(ptss.film_camera("pinhole", 7, 9, cam), s0, first_pixel=63 - n + 1)   # firstPixel + n leaves the film
    film = ptss.film_camera("pinhole", 7, 9, cam, lens_radius=-1.0, focus_distance=-1.0)   # the lens is the thin lens' alone
    ptss.probe_film_rays(film, s0)


# ---- thin lens and equirect against an independent float64 model -----------------------------------------------------------------------
def rotate64(q, v):
    """glm quat * vec3 in float64, q = (x, y, z, w) as stored."""
    u = np.array(q[:3], dtype=np.float64)
    uv = np.cross(u, v)
    uuv = np.cross(u, uv)
    return v + 2.0 * q[3] * uv + 2.0 * uuv


def camera_numbers(cam):
    q = [float(cam.rotation.x), float(cam.rotation.y), float(cam.rotation.z), float(cam.rotation.w)]
    pos = np.array([cam.position.x, cam.position.y, cam.position.z], dtype=np.float64)
    return q, pos


def sincos_abs_error(lo, hi):
    """The largest absolute error of ptm::sincos on [lo, hi] against libm, sampled densely (ptss_probe_math ops 0 and 1)."""
    x = np.concatenate([np.linspace(lo, hi, 200_001), np.random.default_rng(3).uniform(lo, hi, 200_000)]).astype(np.float32)
    out = []
    for op, ref in ((0, np.sin), (1, np.cos)):
        got = np.empty_like(x)
        f32p = C.POINTER(C.c_float)
        assert ptss.host_lib().ptss_probe_math(op, x.ctypes.data_as(f32p), None, got.ctypes.data_as(f32p), x.size) == 0
        out.append(np.abs(got.astype(np.float64) - ref(x.astype(np.float64))).max())
    return max(out)


# tests/test_ptmath.py pins |ptm::sincos - libm| < 2e-7 on [-60, 60]; the models below use arguments in [-pi, 2 pi]. Measured here on
# that range (400,000 arguments) the error is 9.0e-8; the derivations use the pinned 2e-7 (= 3.36 u). ptm::sqrt is the correctly rounded root on the
# host (relative error <= u / 2, taken as u), and every + - * / fma is correctly rounded (relative error <= u).
A = 2e-7
ROTATE_U = 22.0   # rounding error of ptv::rotate per component, in units of u |v|, for a unit quaternion: uv = cross(u, v) 2 u; uuv = cross(u, uv)
#                   2 * 2 u + 2 u = 6 u; uv * (2 w) 2 * 2 u + 2 u = 6 u; uuv * 2 12 u; (v + uv) rounds at |.| <= 3: 3 u; + uuv: u. 6 + 12 + 3 + 1.
NORMALIZE_U = 4.5  # normalize: dot 3 u relative, halved by the root 1.5 u, sqrt u, rcp u, the product u


def test_sincos_error_on_the_range_the_models_use():
    assert sincos_abs_error(-math.pi, 2 * math.pi) < A


def equirect_bound():
    """|direction - model|_2 for PTSS_FILM_EQUIRECT, first order in u, from the rounded operations of csrc/ptcamera.h:
      X = x + jx (u), invW (u), X invW (u): a in (0, 1], |da| <= 3 u;  b = a - 0.5: |db| <= 3.5 u, |b| <= 0.5
      lon = b * float(2 pi): the constant u, the product u: |dlon| <= 2 pi (3.5 + 1) u = 28.3 u;  |dlat| <= pi 4.5 u = 14.2 u
      sl, cl: A + |dlon|;  se, ce: A + |dlat|      (|sin'|, |cos'| <= 1)
      c.x = sl ce, c.z = -(cl ce): |d| <= (A + |dlon|) + (A + |dlat|) + u;  c.y = se: A + |dlat|
      rotate: an isometry on the incoming error, plus ROTATE_U u per component (|c| = 1)
      normalize: removes the radial part, adds NORMALIZE_U u."""
    dlon, dlat = 2 * math.pi * 4.5 * U, math.pi * 4.5 * U
    ex = (A + dlon) + (A + dlat) + U
    ey = A + dlat
    return 1.01 * (math.sqrt(2 * ex * ex + ey * ey) + ROTATE_U * math.sqrt(3) * U + NORMALIZE_U * U)   # 1.01: the second-order terms


def thin_lens_bounds(film):
    """(|direction - model|_2, |origin - model|_2) for PTSS_FILM_THIN_LENS, first order in u, with F = focusDistance, R = lensRadius,
    s = -2 tan(fov / 2), k = aspect:
      b as above: |db| <= 3.5 u, |b| <= 0.5;  s: tan = sin / cos of fov / 2, relative error e_s = A / |sin| + A / |cos| + u
      start.x = (b s) zNear; t = F / |zNear| (u); f.x = start.x t: |df.x| <= F |s| (3.5 u + 0.5 (e_s + u) + 0.5 * 3 u) = F |s| (5.5 u + 0.5 e_s)
      f.y has the factor k = H / W (u) and one more product (u): |df.y| <= F |s| k (6.5 u + 0.5 e_s);  f.z = zNear t: 2 u F
      lens: r = R sqrt(u1): 2 u relative; the angle float(2 pi) u2: 2 pi 2 u; sn, cs: A + 4 pi u; l.x, l.y: R (A + 4 pi u + 3 u)
      v = f - l: one rounding per component, u (|f| + R);  rotate: ROTATE_U u |v| per component;  |v| >= F (1 - 2 u)
      normalize: the tangential part of the error over |v|, plus NORMALIZE_U u.
      origin = position + rotate(l): the error of l, ROTATE_U u R per component, and the sum's rounding u |origin| per component."""
    F, R = film.focusDistance, film.lensRadius
    fov = float(film.camera.fieldOfView)
    s = 2 * math.tan(fov / 2)
    k = film.height / film.width
    e_s = A / abs(math.sin(fov / 2)) + A / abs(math.cos(fov / 2)) + U
    dl = R * (A + 4 * math.pi * U + 3 * U)
    fx, fy = 0.5 * s * F, 0.5 * s * k * F
    ex = F * s * (5.5 * U + 0.5 * e_s) + dl + U * (fx + R)
    ey = F * s * k * (6.5 * U + 0.5 * e_s) + dl + U * (fy + R)
    ez = 3 * U * F
    vmax = math.sqrt(fx * fx + fy * fy + F * F) + R
    direction = 1.01 * ((math.sqrt(ex * ex + ey * ey + ez * ez) + ROTATE_U * math.sqrt(3) * U * vmax) / (F * (1 - 2 * U)) + NORMALIZE_U * U)
    pos = max(abs(film.camera.position.x), abs(film.camera.position.y), abs(film.camera.position.z)) + R
    origin = 1.01 * (math.sqrt(2) * dl + ROTATE_U * math.sqrt(3) * U * R + math.sqrt(3) * U * pos)
    return direction, origin


def model(film, p, uni):
    """The eye ray of film pixel p in float64, from the formulas of include/ptss.h: (origin, direction, focus point or None)."""
    q, pos = camera_numbers(film.camera)
    jx, jy = (float(uni[0]), float(uni[1])) if film.jitter else (0.5, 0.5)
    X, Y = p % film.width + jx, p // film.width + jy
    if film.kind == ptss.FILM_EQUIRECT:
        lon, lat = (X / film.width - 0.5) * 2 * math.pi, (Y / film.height - 0.5) * math.pi
        d = rotate64(q, np.array([math.sin(lon) * math.cos(lat), math.sin(lat), -math.cos(lon) * math.cos(lat)]))
        return pos, d / np.linalg.norm(d), None
    s = -2 * math.tan(float(film.camera.fieldOfView) / 2)
    z = float(film.camera.zNear)
    start = np.array([(X / film.width - 0.5) * s, (Y / film.height - 0.5) * s * (film.height / film.width), 1.0]) * z
    f = start * (film.focusDistance / abs(start[2]))
    lens = np.zeros(3)
    if film.jitter:
        r, a = film.lensRadius * math.sqrt(float(uni[2])), 2 * math.pi * float(uni[3])
        lens = np.array([r * math.cos(a), r * math.sin(a), 0.0])
    d = rotate64(q, f - lens)
    return pos + rotate64(q, lens), d / np.linalg.norm(d), pos + rotate64(q, f)


@pytest.mark.parametrize("width,height", [(64, 48), (5, 3), (3, 64)])
@pytest.mark.parametrize("jitter", [1, 0])
def test_thin_lens_and_equirect_against_the_float64_model(width, height, jitter):
    cam, seed = turned_camera(), 0xBEEF
    n = width * height
    s0 = seeded_states(seed, n)
    for kind in ("thinlens", "equirect"):
        film = ptss.film_camera(kind, width, height, cam, jitter=jitter, **LENS)
        rays, _, _ = ptss.probe_film_rays(film, s0)
        if kind == "equirect":
            bound_d, bound_o = equirect_bound(), 0.0
        else:
            bound_d, bound_o = thin_lens_bounds(film)
        assert bound_d < 1e-4   # not vacuous: a few 1e-6, 8e-5 on the 3 x 64 film, whose aspect of 21 scales the y terms
        worst_d = worst_o = 0.0
        for p in range(n):
            o, d, _ = model(film, p, advance(s0[p], 4)[1])
            worst_d = max(worst_d, float(np.linalg.norm(rays["direction"][p].astype(np.float64) - d)))
            worst_o = max(worst_o, float(np.linalg.norm(rays["origin"][p].astype(np.float64) - o)))
        print(f"{kind} {width}x{height} jitter {jitter}: direction error {worst_d:.3g} (bound {bound_d:.3g}), origin error {worst_o:.3g} (bound {bound_o:.3g})")
        assert worst_d <= bound_d and worst_o <= bound_o, (kind, worst_d, bound_d, worst_o, bound_o)
        assert (rays["tmax"] == np.inf).all() and (rays["pad"] == 0).all()


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def test_equirect_centre_and_senses_are_the_pinholes():
    cam = turned_camera()
    s0 = seeded_states(1, 15)
    # 5 x 3, jitter 0: pixel (2, 1) has x + 0.5 = width / 2 and y + 0.5 = height / 2
    eq, _, _ = ptss.probe_film_rays(ptss.film_camera("equirect", 5, 3, cam, jitter=0), s0)
    ph, _, _ = ptss.probe_film_rays(ptss.film_camera("pinhole", 5, 3, cam, jitter=0), s0)
    centre = 1 * 5 + 2
    assert np.linalg.norm(eq["direction"][centre].astype(np.float64) - ph["direction"][centre]) <= equirect_bound() + (ROTATE_U * math.sqrt(3) + NORMALIZE_U) * U
    q, pos = camera_numbers(cam)
    assert np.linalg.norm(eq["direction"][centre] - rotate64(q, np.array([0.0, 0.0, -1.0]))) <= equirect_bound()
    for step in (1, 5):   # one pixel to the right, one pixel up: the same side as the pinhole's
        move_eq = eq["direction"][centre + step].astype(np.float64) - eq["direction"][centre]
        move_ph = ph["direction"][centre + step].astype(np.float64) - ph["direction"][centre]
        assert np.dot(move_eq, move_ph) > 0.1 * np.linalg.norm(move_eq) * np.linalg.norm(move_ph), step
    assert np.dot(eq["direction"][centre + 1] - eq["direction"][centre], rotate64(q, np.array([1.0, 0.0, 0.0]))) > 0
    assert np.dot(eq["direction"][centre + 5] - eq["direction"][centre], rotate64(q, np.array([0.0, 1.0, 0.0]))) > 0
    assert np.array_equal(words(eq["origin"]), words(ph["origin"]))
    # the whole sphere is covered: the bottom row looks down, the top row up, the left and right edges backwards
    big, _, _ = ptss.probe_film_rays(ptss.film_camera("equirect", 64, 48, cam, jitter=0), seeded_states(1, 64 * 48))
    local = np.array([rotate64([-q[0], -q[1], -q[2], q[3]], d.astype(np.float64)) for d in big["direction"]]).reshape(48, 64, 3)
    assert (local[0, :, 1] < -0.99).all() and (local[-1, :, 1] > 0.99).all()
    assert (local[24, 0, 2] > 0.99) and (local[24, 63, 2] > 0.99) and local[24, 32, 2] < -0.99
    assert local[24, 16, 0] < -0.99 and local[24, 48, 0] > 0.99


def test_thin_lens_rays_meet_in_the_focus_point():
    cam, seed, width, height = turned_camera(), 77, 16, 12
    film = ptss.film_camera("thinlens", width, height, cam, **LENS)
    bound_d, bound_o = thin_lens_bounds(film)
    q, pos = camera_numbers(cam)
    axis = rotate64(q, np.array([0.0, 0.0, 1.0]))
    far = 0
    for first in (0, 1000, 2000):   # three samples of every pixel: different lens points, different sample positions
        s0 = seeded_states(seed, width * height, first)
        rays, _, _ = ptss.probe_film_rays(film, s0)
        for p in range(width * height):
            _, _, focus = model(film, p, advance(s0[p], 4)[1])
            o, d = rays["origin"][p].astype(np.float64), rays["direction"][p].astype(np.float64)
            miss = np.linalg.norm(np.cross(focus - o, d))   # the distance of the focus point from the ray's line
            reach = np.linalg.norm(focus - o)
            assert miss <= reach * bound_d + bound_o, (p, miss)
            off = o - pos
            assert np.linalg.norm(off) <= film.lensRadius + bound_o, p          # on the lens
            assert abs(np.dot(off, axis)) <= bound_o, p                          # in the lens plane
            far = max(far, np.linalg.norm(off))
    assert far > 0.9 * film.lensRadius   # the lens is used out to its rim


# ---- accumulation ----------------------------------------------------------------------------------------------------------------------
def test_probe_accumulate_against_the_oracle_tone_map():
    rad = adversarial_radiance()
    n, P = len(rad), 97
    res = results_of(rad)
    q = np.array([[oracle.probe_quantize(float(v)) for v in row] for row in rad], dtype=np.uint32)
    assert q[np.isnan(rad)].max() == 0 and (q[rad == np.inf] == 255).all() and (q[rad < 0] == 0).all() and set(np.unique(q)) == set(range(256))
    g = np.random.default_rng(2)
    maps = {"all on one pixel": np.full(n, 5, np.uint32), "many to few": g.integers(0, 7, n).astype(np.uint32),
            "with entries beyond the film": np.where(np.arange(n) % 10 == 3, P + np.arange(n), g.integers(0, P, n)).astype(np.uint32)}
    start = np.zeros(P, dtype=ptss.FILM_DTYPE)
    start["r"], start["g"], start["b"], start["samples"] = 1000, 2000, 3000, 40   # a film that has been in use (pixel 5 and the rest alike)
    for what, index in maps.items():
        film, pixels, history, rejected = ptss.probe_accumulate(res, start, index=index, pixels=np.full((P, 4), 9, np.uint8),
                                                                history=np.full((P, 4), -2.0, np.float32))
        inside = index < P
        assert rejected == int((~inside).sum()), what
        want = words(start).astype(np.uint64)
        for i in np.nonzero(inside)[0]:
            want[index[i], :3] += q[i]
            want[index[i], 3] += 1
        assert np.array_equal(words(film), want.astype(np.uint32)), what
        touched = np.zeros(P, bool)
        touched[index[inside]] = True
        inv = (np.float32(1) / want[:, 3].astype(np.float32)).astype(np.float32)
        value = (want[:, :3].astype(np.float32) * inv[:, None]).astype(np.float32)
        byte = (value + np.float32(0.5)).astype(np.float32).astype(np.uint8)
        assert np.array_equal(pixels[touched, :3], byte[touched]) and (pixels[touched, 3] == 255).all(), what
        assert (pixels[~touched] == 9).all() and (words(history)[~touched] == words(np.full((1, 4), -2.0, np.float32))).all(), what
        assert np.array_equal(words(history)[touched, :3], words(value)[touched]) and np.array_equal(history["weight"][touched], want[touched, 3].astype(np.float32))
    # the identity map, at an offset, with either output absent
    film, pixels, history, rejected = ptss.probe_accumulate(res[:50], start, first_pixel=40, pixels=None, history=True)
    assert rejected == 0 and pixels is None
    assert np.array_equal(words(film)[40:90, :3], words(start)[40:90, :3] + q[:50]) and (film["samples"][40:90] == 41).all()
    assert np.array_equal(words(film)[:40], words(start)[:40]) and np.array_equal(words(film)[90:], words(start)[90:])
    assert (history["weight"][40:90] == 41).all() and (history["weight"][:40] == 0).all()
    with pytest.raises(ptss.PtssError):
        ptss.probe_accumulate(res[:50], start, first_pixel=P - 49)


# ---- the identity's condition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,iterations", CASES)
def test_case_keeps_the_loop_guard_silent_in_every_frame_used(name, iterations):
    f = frames_of(name, iterations)
    assert len(f.live_counts) == FRAMES
    for k, counts in enumerate(f.live_counts):
        assert satisfies_identity_condition(counts, iterations), (name, iterations, k, counts.tolist())
        assert counts[0] == W * H
    assert (f.accum[1] >= f.accum[0]).all() and (f.states[1] != f.states[0]).any(axis=1).all()   # the sums grow, every stream went on


def test_the_tightest_case_is_cornell_at_eight_iterations():
    tightest = min((int(min(c.min() for c in frames_of(name, it).live_counts)), name, it) for name, it in CASES)
    assert tightest == (142, "cornell", 8), tightest
