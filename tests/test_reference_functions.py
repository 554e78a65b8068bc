"""The oracle (oracle/oracle.cpp) and the host mirror's camera, function by function, against THE REFERENCE'S OWN CODE compiled
for the CPU (oracle/_ref/libref_probe.so, oracle/build.py build_ref). Until this file, nothing but known-answer tests and goldens
made from the oracle itself stood between a misread line of the reference and a green suite.

Two classes of assertion, both stated in tests/reference_common.py: decisions are EQUAL (a case may be left out only where a
float64 model puts the deciding quantity within 4 float32 ulp of its threshold; at most 0.5 % per function); floats pass within
3 * e_ref + 1 ulp, e_ref being what the compiled reference itself is away from a float64 model of its formula (at most 64 ulp).

Skips only where neither the reference nor its library exists; FAILS where the reference is there and the library is not."""
import ctypes as C

import numpy as np
import pytest

import oracle
import ptss
import refprobe
from reference_common import (BUMP, GAMMA, INVERSE_PI_F, PI_F, check_floats, check_left_out, closest_hit_model, dot, draws_used, f64,
                              line_of_sight_model, lobe_sample_model, near, norm, quat_rotate, require_reference, rotate_v2v_model,
                              scene_arrays, scene_rays, surface_points, snell_fresnel_model, sphere_model, triangle_model, uniforms, unit_vectors)

N = 4000   # "a few thousand cases each"


@pytest.fixture(scope="module")
def ref():
    return require_reference()


@pytest.fixture(scope="module")
def orc():
    p = refprobe.Probes("oracle")
    yield p
    p.close()


@pytest.fixture(scope="module")
def scenes(ref):
    """The reference's two scenes, built by the reference: name -> (tables, float64 arrays, SceneDesc)."""
    out = {}
    for kind, name in ((1, "cornell"), (0, "default")):
        t = ref.build_scene(kind)
        out[name] = (t, scene_arrays(t), refprobe.desc_of_tables(t))
    return out


def test_the_stand_in_rng_is_the_oracles_rng(ref):
    """oracle/ref_shim/curand_kernel.h against oracle.probe_rng (itself held against rocRAND's tables): seed scramble, subsequence
    jump, raw draws, uniforms."""
    for seed, seq in [(0, 0), (0x5EED, 0), (0x5EED, 1), (1, 7), (123456789, 262143), (0xFFFFFFFF, 65536), (2 ** 40 + 5, 3)]:
        a, b = ref.rng(seed, seq, 64), oracle.probe_rng(seed, seq, 64)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (seed, seq)


# ---- Primitives.h ----------------------------------------------------------------------------------------------------------
def _sphere_cases(rng, n):
    """Random spheres and unit rays, most aimed into the sphere (a third of random rays would hit nothing), origins inside and
    outside; then the edge cases of tests/test_sphere_forms.py and tests/test_sphere_behind.py."""
    c = rng.uniform(-3, 3, (n, 3))
    r = rng.uniform(0.2, 2.5, (n, 1))
    o = rng.uniform(-6, 6, (n, 3))
    inside = rng.random(n) < 0.25
    o[inside] = (c + unit_vectors(rng, n) * r * rng.uniform(0, 0.95, (n, 1)))[inside]
    # aimed at a point within 0.9 radii of the centre (a hit whose discriminant keeps its digits) or beyond 1.1 (a miss)
    aim = c + unit_vectors(rng, n) * r * np.where(rng.random((n, 1)) < 0.75, rng.uniform(0, 0.9, (n, 1)), rng.uniform(1.1, 1.6, (n, 1)))
    d = aim - o
    d /= norm(d)[:, None]
    flip = rng.random(n) < 0.15   # spheres behind the origin
    d[flip] = -d[flip]
    sph = np.concatenate([c, r], axis=1).astype(np.float32)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    edge_s, edge_r = [], []

    def add(center, radius, origin, direction):
        edge_s.append([*center, radius])
        edge_r.append([*origin, *direction])
    add((0, 0, -5), 1, (0, 0, 0), (0, 0, -1))        # head on
    add((0, 0, -5), 1, (0, 0, -5), (0, 0, -1))       # from the centre
    add((0, 0, -5), 1, (0, 0, -5), (1, 0, 0))
    add((0, 0, 5), 1, (0, 0, 0), (0, 0, -1))         # wholly behind
    add((0, 0, -5), 1, (0, 0, -4), (0, 0, -1))       # origin on the surface, going in: t0 = 0
    add((0, 0, -5), 1, (0, 0, -4), (0, 0, 1))        # origin on the surface, going out: t1 = 0
    add((0, 0, -5), 1, (0, 0, -6), (0, 0, -1))       # on the far surface, leaving
    add((0, 0, -5), 1, (1, 0, 0), (0, 0, -1))        # tangent: discriminant exactly 0
    add((0, 0, -5), 1, (1.5, 0, 0), (0, 0, -1))      # passes beside
    add((0, 0, -5), 0.5, (0, 0, 0), (0, 0, -2))      # direction not normalised (the formula assumes a = 1)
    add((1e3, 0, 0), 1, (0, 0, 0), (1, 0, 0))        # far away
    add((0, 0, -5), 1e-3, (0, 0, 0), (0, 0, -1))     # tiny
    add((0, 0, 0), 100, (1, 2, 3), (0, 1, 0))        # huge, origin inside
    sph = np.concatenate([sph, np.array(edge_s, np.float32)])
    rays = np.concatenate([rays, np.array(edge_r, np.float32)])
    return sph, rays, len(edge_s)


@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("finite", [False, True])
def test_sphere_intersect_ray(ref, orc, update, finite):
    """Sphere::intersectRay / getSurfaceElement, Primitives.h:98-175, with and without updateSurfel, `distance` infinite or finite."""
    rng = np.random.default_rng(11)
    sph, rays, edges = _sphere_cases(rng, N)
    c, r, o, d = f64(sph[:, :3]), f64(sph[:, 3]), f64(rays[:, :3]), f64(rays[:, 3:])
    tmax = np.full(len(sph), np.inf, np.float32)
    if finite:   # a limit on either side of the hit distance, and exactly on it for the edge cases
        _, t_inf, _, _, _ = sphere_model(c, r, o, d, f64(tmax))
        tmax = np.where(np.isfinite(t_inf), t_inf * rng.uniform(0.5, 1.5, len(sph)), 3.0).astype(np.float32)
        tmax[-edges:] = np.where(np.isfinite(t_inf[-edges:]) & (t_inf[-edges:] > 0), t_inf[-edges:], 1.0).astype(np.float32)
    hit_m, t, point, normal, nr = sphere_model(c, r, o, d, f64(tmax))
    name = f"Sphere::intersectRay update={int(update)} finite={int(finite)}"
    keep = check_left_out(name, nr)
    hr, outr = ref.sphere(sph, rays, tmax, update)
    ho, outo = orc.sphere(sph, rays, tmax, update)
    assert np.array_equal(hr[keep], hit_m[keep]), "the compiled reference and its float64 model decide differently away from every threshold"
    assert np.array_equal(hr[keep], ho[keep]), np.flatnonzero(keep & (hr != ho))[:10]
    assert hr.sum() > N // 3 and (~hr).sum() > N // 10
    # floats: the cases whose discriminant b^2 - 4c keeps at least 2^-6 of its larger term (the random cases are aimed that way; a
    # grazing ray, a pin-head sphere seen from afar, an origin on the surface are decisions to get right, not distances to compare).
    # The distance is a difference of terms the size of |origin - centre| + radius, the point one of terms the size of the origin
    # and the distance: those are the floors.
    v = o - c
    b2, c4 = (2 * dot(d, v)) ** 2, 4 * (dot(v, v) - r * r)
    k = keep & hr & (b2 - c4 >= 2.0 ** -6 * np.maximum(b2, 4 * np.maximum(dot(v, v), r * r)))
    assert k.sum() > N // 5
    span = norm(v) + r
    check_floats(name + " distance", outr[:, 0], outo[:, 0], t, floor=span, vector=False, keep=k)
    # a miss leaves `distance` alone: bit for bit
    assert np.array_equal(outr[keep & ~hr, 0].view(np.uint32), outo[keep & ~hr, 0].view(np.uint32))
    if update:
        check_floats(name + " point", outr[:, 1:4], outo[:, 1:4], point, floor=span + norm(o), keep=k)
        # the normal divides (point - centre) by its length, the radius: the point's error over the radius
        check_floats(name + " normal", outr[:, 4:7], outo[:, 4:7], normal, floor=np.maximum(1.0, (span + norm(o)) / r), keep=k)
        assert np.array_equal(outr[k, 7], outo[k, 7])
    # where nothing is written, nothing is written on either side (the surfel went in zeroed)
    untouched = ~hr if update else np.ones(len(hr), bool)
    assert not outr[untouched, 1:].any() and not outo[untouched, 1:].any()


def _triangle_cases(rng, n):
    v0 = rng.uniform(-4, 4, (n, 3))
    v1 = v0 + rng.uniform(-3, 3, (n, 3))
    v2 = v0 + rng.uniform(-3, 3, (n, 3))
    normals = [unit_vectors(rng, n) for _ in range(3)]
    w = rng.uniform(-0.3, 1.0, (n, 2))   # target in the triangle's plane, inside for w1, w2 >= 0, w1 + w2 <= 1
    target = v0 + (v1 - v0) * w[:, :1] + (v2 - v0) * w[:, 1:]
    o = rng.uniform(-6, 6, (n, 3))
    d = target - o
    d /= norm(d)[:, None]
    flip = rng.random(n) < 0.1
    d[flip] = -d[flip]   # triangle behind the ray
    tri = np.concatenate([v0, v1, v2] + normals, axis=1).astype(np.float32)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    et, er = [], []

    def add(a, b, c, origin, direction, nrm=((0, 0, 1),) * 3):
        et.append([*a, *b, *c, *nrm[0], *nrm[1], *nrm[2]])
        er.append([*origin, *direction])
    A, B, Cc = (-1, -1, -3), (1, -1, -3), (0, 1, -3)
    add(A, B, Cc, (0, 0, 0), (0, 0, -1))             # through the inside
    add(A, B, Cc, (0, -1, 0), (0, 0, -1))            # onto an edge: weight[2] = 0
    add(A, B, Cc, (-1, -1, 0), (0, 0, -1))           # onto a vertex
    add(A, B, Cc, (0, 1, 0), (0, 0, -1))             # onto the apex
    add(A, B, Cc, (0, 0, 0), (0, 0, 1))              # behind
    add(A, B, Cc, (0, 0, -3), (0, 0, -1))            # origin in the plane: dist = 0 is a miss
    add(A, B, Cc, (0, 0, 0), (1, 0, 0))              # parallel: det = 0
    add(A, B, Cc, (0, 0, -6), (0, 0, 1))             # from the back side
    add(A, B, Cc, (5, 5, 0), (0, 0, -1))             # far outside
    add(A, A, Cc, (0, 0, 0), (0, 0, -1))             # degenerate: two equal vertices
    add((-1e-3, -1e-3, -3), (1e-3, -1e-3, -3), (0, 1e-3, -3), (0, 0, 0), (0, 0, -1))   # tiny: |det| against the epsilon
    add((-1e-4, -1e-4, -3), (1e-4, -1e-4, -3), (0, 1e-4, -3), (0, 0, 0), (0, 0, -1))   # tinier: below the epsilon
    add(A, B, Cc, (0, 0, 0), (0, 0, -1), ((1, 0, 0), (0, 1, 0), (0, 0, 1)))            # interpolated normals
    tri = np.concatenate([tri, np.array(et, np.float32)])
    rays = np.concatenate([rays, np.array(er, np.float32)])
    return tri, rays, len(et)


@pytest.mark.parametrize("update", [True, False])
@pytest.mark.parametrize("finite", [False, True])
def test_triangle_intersect_ray(ref, orc, update, finite):
    """Triangle::intersectRay, Primitives.h:25-83, with and without updateSurfel, `distance` infinite or finite."""
    rng = np.random.default_rng(12)
    tri, rays, edges = _triangle_cases(rng, N)
    parts = [f64(tri[:, 3 * k:3 * k + 3]) for k in range(6)]
    o, d = f64(rays[:, :3]), f64(rays[:, 3:])
    tmax = np.full(len(tri), np.inf, np.float32)
    if finite:
        _, t_inf, _, _, _ = triangle_model(*parts, o, d, f64(tmax))
        ok = np.isfinite(t_inf) & (t_inf > 0)
        tmax = np.where(ok, t_inf * rng.uniform(0.5, 1.5, len(tri)), 3.0).astype(np.float32)
        tmax[-edges:] = np.where(ok[-edges:], t_inf[-edges:], 1.0).astype(np.float32)
    hit_m, t, point, normal, nr = triangle_model(*parts, o, d, f64(tmax))
    name = f"Triangle::intersectRay update={int(update)} finite={int(finite)}"
    keep = check_left_out(name, nr)
    hr, outr = ref.triangle(tri, rays, tmax, update)
    ho, outo = orc.triangle(tri, rays, tmax, update)
    assert np.array_equal(hr[keep], hit_m[keep]), "the compiled reference and its float64 model decide differently away from every threshold"
    assert np.array_equal(hr[keep], ho[keep]), np.flatnonzero(keep & (hr != ho))[:10]
    assert hr.sum() > N // 10 and (~hr).sum() > N // 5
    # floats: the cases whose determinant keeps at least 2^-3 of |e1| |e2| |d| (neither a sliver nor a grazing ray: those are
    # decisions to get right, not distances to compare). The distance is a quotient of triple products of vectors the size of
    # |origin - vertex0| and the edges: their sum is the floor; the weights are quotients of the same kind.
    v0, v1, v2 = parts[:3]
    e1, e2, s = v1 - v0, v2 - v0, o - v0
    det = dot(e1, np.cross(d, e2))
    k = keep & hr & (np.abs(det) >= 2.0 ** -3 * norm(e1) * norm(e2) * norm(d))
    assert k.sum() > N // 20
    span = norm(s) + norm(e1) + norm(e2)
    check_floats(name + " distance", outr[:, 0], outo[:, 0], t, floor=span, vector=False, keep=k)
    assert np.array_equal(outr[keep & ~hr, 0].view(np.uint32), outo[keep & ~hr, 0].view(np.uint32))
    if update:
        check_floats(name + " point", outr[:, 1:4], outo[:, 1:4], point, floor=span + norm(o), keep=k)
        check_floats(name + " normal", outr[:, 4:7], outo[:, 4:7], normal, floor=np.maximum(1.0, span / np.minimum(norm(e1), norm(e2))), keep=k)
        assert np.array_equal(outr[k, 7], outo[k, 7])
    untouched = ~hr if update else np.ones(len(hr), bool)
    assert not outr[untouched, 1:].any() and not outo[untouched, 1:].any()


# ---- the scene loops ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "default"])
def test_closest_hit_loops(ref, orc, scenes, name):
    """The intersection loops of pathTraceKernel, CudaTracer.cu:121-141: which primitive wins, and its surfel."""
    tables, sc, desc = scenes[name]
    ref.use_scene(desc)
    orc.use_scene(desc)
    rng = np.random.default_rng(21)
    rays = scene_rays(rng, name, N)
    tmax = np.where(rng.random(N) < 0.25, rng.uniform(0.5, 12, N), np.inf).astype(np.float32)
    kind_m, prim_m, t, point, normal, nr = closest_hit_model(sc, f64(rays[:, :3]), f64(rays[:, 3:]), f64(tmax))
    label = f"pathTraceKernel loops [{name}]"
    keep = check_left_out(label, nr)
    kr, pr, outr = ref.closest_hit(rays, tmax)
    ko, po, outo = orc.closest_hit(rays, tmax)
    assert np.array_equal(kr[keep], kind_m[keep]) and np.array_equal(pr[keep], prim_m[keep]), "reference against its float64 model"
    assert np.array_equal(kr[keep], ko[keep]) and np.array_equal(pr[keep], po[keep])
    assert np.array_equal(outr[keep, 7], outo[keep, 7])   # materialIdx
    assert (kr == 2).sum() > N // 4 and (kr == 0).sum() > 0 and (kr == 1).sum() > N // 50
    # floats, with the floors and the conditioning of the two primitive tests: a sphere hit counts where its discriminant keeps 2^-6
    # of its larger term, and its normal is the point's error over the radius
    o, d = f64(rays[:, :3]), f64(rays[:, 3:])
    sph = kr == 1
    c, r = sc["c"][np.where(sph, pr, 0)], sc["r"][np.where(sph, pr, 0)]
    v = o - c
    b2, c4 = (2 * dot(d, v)) ** 2, 4 * (dot(v, v) - r * r)
    k = keep & (kr > 0) & (~sph | (b2 - c4 >= 2.0 ** -6 * np.maximum(b2, 4 * np.maximum(dot(v, v), r * r))))
    span = norm(o) + np.where(np.isfinite(t), t, 0.0) + 1.0
    check_floats(label + " distance", outr[:, 0], outo[:, 0], t, floor=span, vector=False, keep=k)
    check_floats(label + " point", outr[:, 1:4], outo[:, 1:4], point, floor=span, keep=k)
    check_floats(label + " normal", outr[:, 4:7], outo[:, 4:7], normal, floor=np.where(sph, np.maximum(1.0, span / r), 1.0), keep=k)


@pytest.mark.parametrize("name", ["cornell", "default"])
def test_line_of_sight(ref, orc, scenes, name):
    """lineOfSight, CudaTracer.cu:420-455, between surface points and points on the lights / anywhere in the box."""
    tables, sc, desc = scenes[name]
    ref.use_scene(desc)
    orc.use_scene(desc)
    rng = np.random.default_rng(22)
    p0, nrm = surface_points(rng, ref, name, N, tables)
    lights = tables["areaLights"]["triangleIdx"]
    tri = tables["triangles"][rng.choice(lights, N) + rng.integers(0, 2, N)]
    w = rng.dirichlet((1, 1, 1), N)
    on_light = f64(tri["vertex0"]) * w[:, :1] + f64(tri["vertex1"]) * w[:, 1:2] + f64(tri["vertex2"]) * w[:, 2:]
    half = 4.0 if name == "cornell" else 5.0
    anywhere = np.stack([rng.uniform(-0.9 * half, 0.9 * half, N), rng.uniform(-0.9 * half, 0.9 * half, N), rng.uniform(-1.9 * half, -0.1, N)], axis=1)
    p1 = np.where((rng.random(N) < 0.6)[:, None], on_light, anywhere).astype(np.float32)
    vis_m, w_i, d2, nr = line_of_sight_model(sc, f64(nrm), f64(p0), f64(p1))
    label = f"lineOfSight [{name}]"
    keep = check_left_out(label, nr)
    vr, outr = ref.line_of_sight(nrm, p0, p1)
    vo, outo = orc.line_of_sight(nrm, p0, p1)
    assert np.array_equal(vr[keep], vis_m[keep]), "reference against its float64 model"
    assert np.array_equal(vr[keep], vo[keep])
    assert vr.sum() > N // 10 and (~vr).sum() > N // 10
    check_floats(label + " w_i", outr[:, :3], outo[:, :3], w_i, floor=1.0)
    check_floats(label + " distance2", outr[:, 3], outo[:, 3], d2, floor=1.0, vector=False)


# ---- Snell, Fresnel, the rays ------------------------------------------------------------------------------------------------
def test_snell_and_fresnel(ref, orc):
    """computeSinT2AndRefractiveIndexes with computeFresnelForReflectance, CudaTracer.cu:457-494, on both sides of total internal
    reflection: from outside (cosI > 0) there is none; from inside (cosI <= 0) it sets in below cos = sqrt(1 - 1/n^2)."""
    rng = np.random.default_rng(31)
    refr = rng.uniform(1.05, 6.0, N)
    cos_i = rng.uniform(-1, 1, N)
    crit = -np.sqrt(1 - 1 / refr ** 2)
    k = N // 4
    cos_i[:k] = crit[:k] * rng.uniform(0.9, 1.1, k)            # around the critical angle, from inside
    extra_n = np.array([1.55, 1.55, 1.55, 1.55, 1.7, 5.8, 2.5, 1.0, 1.0, 1.55, 1.55], dtype=np.float32)
    extra_c = np.array([1.0, -1.0, 0.0, -0.0, 1e-6, -1e-6, 0.5, 0.5, -0.5, 1e-20, -1e-20], dtype=np.float32)
    refr = np.concatenate([refr.astype(np.float32), extra_n])
    cos_i = np.clip(np.concatenate([cos_i.astype(np.float32), extra_c]), -1, 1)
    c, s2, n1, n2, n, f, nr = snell_fresnel_model(f64(refr), f64(cos_i))
    keep = check_left_out("Snell + Fresnel", nr)
    r, o = ref.fresnel(refr, cos_i), orc.fresnel(refr, cos_i)
    tir_r, tir_o, tir_m = r[:, 1] > 1, o[:, 1] > 1, s2 > 1
    assert np.array_equal(tir_r[keep], tir_m[keep]) and np.array_equal(tir_r[keep], tir_o[keep])
    assert tir_r.sum() > N // 20 and (~tir_r).sum() > N // 2
    for col in (0, 2, 3):   # cosI made positive, n1, n2: copies of the inputs
        assert np.array_equal(r[:, col].view(np.uint32), o[:, col].view(np.uint32))
    assert np.array_equal(r[keep & tir_r, 5], o[keep & tir_r, 5]) and (r[keep & tir_r, 5] == 1.0).all()
    check_floats("Snell n", r[:, 4], o[:, 4], n, floor=1.0, vector=False)
    check_floats("Snell sinT2", r[:, 1], o[:, 1], s2, floor=1.0, vector=False)
    # the reflectance is a sum of squares of ratios whose numerators cancel near normal incidence and near Brewster's angle: floor 1
    check_floats("Fresnel reflectance", r[:, 5], o[:, 5], f, floor=1.0, vector=False, keep=keep & ~tir_r)


def test_refl_ray_both_overloads(ref, orc):
    """reflRay(ray, surfel, cosI), CudaTracer.cu:496-503, and reflRay(ray, point, normal), :505-514 (which takes |d . n|)."""
    rng = np.random.default_rng(32)
    d, nrm = unit_vectors(rng, N), unit_vectors(rng, N)
    p = rng.uniform(-5, 5, (N, 3)).astype(np.float32)
    d[:3], nrm[:3] = [(0, 0, -1), (0, 0, -1), (1, 0, 0)], [(0, 0, 1), (0, 0, -1), (0, 1, 0)]   # head on, from behind, grazing
    cos_i = (-dot(f64(d), f64(nrm))).astype(np.float32)   # what pathTraceKernel passes, CudaTracer.cu:150
    D, Nn, P, Cc = f64(d), f64(nrm), f64(p), f64(cos_i)
    r, o = ref.refl_surfel(d, p, nrm, cos_i), orc.refl_surfel(d, p, nrm, cos_i)
    check_floats("reflRay(surfel, cosI) origin", r[:, :3], o[:, :3], P + Nn * BUMP, floor=1.0)
    check_floats("reflRay(surfel, cosI) direction", r[:, 3:], o[:, 3:], D - (2 * -Cc)[:, None] * Nn, floor=1.0)
    r, o = ref.refl_normal(d, p, nrm), orc.refl_normal(d, p, nrm)
    check_floats("reflRay(point, normal) origin", r[:, :3], o[:, :3], P + Nn * BUMP, floor=1.0)
    check_floats("reflRay(point, normal) direction", r[:, 3:], o[:, 3:], D - (2 * -np.abs(dot(D, Nn)))[:, None] * Nn, floor=1.0)
    # the sign that a misreading would flip: the reflected ray leaves on the normal's side
    assert (dot(f64(o[:, 3:]), Nn) >= -1e-6).all()


def test_refr_ray(ref, orc):
    """refrRay, CudaTracer.cu:516-531, fed as computeIndirectRadianceAndScatter feeds it; total internal reflection clears `active`
    and leaves NaN behind on both sides."""
    rng = np.random.default_rng(33)
    d, nrm = unit_vectors(rng, N), unit_vectors(rng, N)
    p = rng.uniform(-5, 5, (N, 3)).astype(np.float32)
    refr = rng.uniform(1.1, 3.0, N).astype(np.float32)
    cos_in = (-dot(f64(d), f64(nrm))).astype(np.float32)
    sn = ref.fresnel(refr, cos_in)
    cos_i, sin_t2, n = sn[:, 0].copy(), sn[:, 1].copy(), sn[:, 4].copy()
    ar, r = ref.refr(d, p, nrm, cos_i, sin_t2, n)
    ao, o = orc.refr(d, p, nrm, cos_i, sin_t2, n)
    tir = sin_t2 > 1
    assert np.array_equal(ar, ~tir) and np.array_equal(ao, ~tir) and tir.sum() > N // 20   # the comparison reads the same float: no threshold case
    assert np.isnan(r[tir]).all() and np.isnan(o[tir]).all()
    D, Nn, P = f64(d), f64(nrm), f64(p)
    with np.errstate(invalid="ignore"):
        cos_t = np.sqrt(1.0 - f64(sin_t2))
        w = f64(n)[:, None] * D + (f64(n) * f64(cos_i) - cos_t)[:, None] * Nn
        w = w * (1.0 / np.sqrt(dot(w, w)))[:, None]
    # cosT = sqrt(1 - sinT2) loses its digits as sinT2 approaches 1: keep the cases where 1 - sinT2 still has 2^-6 of them
    k = ~tir & (1.0 - f64(sin_t2) > 2.0 ** -6)
    assert k.sum() > N // 2
    check_floats("refrRay direction", r[:, 3:], o[:, 3:], w, floor=1.0, keep=k)
    check_floats("refrRay origin", r[:, :3], o[:, :3], P + w * BUMP, floor=1.0, keep=k)


def test_rotate_vector_to_vector(ref, orc):
    """rotateVectorToVector, CudaTracer.cu:579-585; exactly opposite vectors give a zero quaternion, which normalize turns into the
    identity (a decision)."""
    rng = np.random.default_rng(34)
    s, t = unit_vectors(rng, N), unit_vectors(rng, N)
    s[: N // 2] = (0, 1, 0)   # the only source the reference uses
    t[:4] = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, -1)]
    s[N // 2: N // 2 + 2], t[N // 2: N // 2 + 2] = [(1, 0, 0), (0, 0, 1)], [(-1, 0, 0), (0, 0, -1)]
    q = rotate_v2v_model(f64(s), f64(t))
    r, o = ref.rotate_v2v(s, t), orc.rotate_v2v(s, t)
    opposite = (1.0 + dot(f64(s), f64(t)) == 0) & (norm(np.cross(f64(s), f64(t))) == 0)
    assert opposite.sum() == 3
    ident = np.array([0, 0, 0, 1], np.float32)
    assert (r[opposite] == ident).all() and (o[opposite] == ident).all()
    # near-opposite vectors leave a quaternion of cancelled digits: keep 1 + s.t >= 2^-6
    k = ~opposite & (1.0 + dot(f64(s), f64(t)) >= 2.0 ** -6)
    assert k.sum() > 0.95 * N
    check_floats("rotateVectorToVector", r, o, q, floor=1.0, keep=k)


# ---- the lobes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,label", [(0, "randomDirectionLambert"), (1, "randomDirectionPhong"), (2, "randomDirectionBeckmann")])
def test_lobe_samplers(ref, orc, kind, label):
    """randomDirection{Lambert, Phong, Beckmann}, CudaTracer.cu:533-577: direction, and the RNG state afterwards (two draws, in the
    reference's order — Beckmann draws its polar angle first, the other two their azimuth)."""
    rng = np.random.default_rng(40 + kind)
    seed = 0xC0FFEE + kind
    axis = unit_vectors(rng, N)
    axis[:3] = [(0, 1, 0), (1, 0, 0), (0, 0, -1)]
    # away from the axis -y, where rotateVectorToVector cancels (see test_rotate_vector_to_vector)
    axis[axis[:, 1] < -0.98] *= -1
    param = {0: np.zeros(N), 1: rng.choice([0.0, 1.0, 10.0, 250.0, 300.0, 5000.0], N), 2: rng.choice([0.1, 0.3, 0.5, 1.0], N)}[kind].astype(np.float32)
    u = uniforms(seed, range(N), 2)
    model = lobe_sample_model(kind, f64(axis), f64(param), u[:, 0], u[:, 1])
    r, sr = ref.sampler(kind, axis, param, seed)
    o, so = orc.sampler(kind, axis, param, seed)
    assert np.array_equal(sr, so), "RNG state after the call"
    assert (draws_used(seed, range(64), sr[:64]) == 2).all()
    # sqrt(1 - y * y) loses its digits as y approaches 1 (a Phong lobe of exponent 5000 lives there): keep 1 - y^2 >= 2^-6
    if kind == 2:
        k = np.ones(N, bool)
    else:
        y = np.sqrt(u[:, 1]) if kind == 0 else np.power(u[:, 1], 1.0 / (f64(param) + 1.0))
        k = 1 - y * y >= 2.0 ** -6
    assert k.sum() > N // 5
    check_floats(label, r, o, model, floor=1.0, keep=k)
    # the rest still has to agree, to what the cancellation leaves: 2^-6 of 24 bits
    assert np.abs(f64(r) - f64(o)).max() <= 2.0 ** -17


def test_get_area_light_point(ref, orc, scenes):
    """getAreaLightPoint, CudaTracer.cu:392-418: four draws, three weights, and the fourth draw picks the triangle (> .5: the
    light's first)."""
    rng = np.random.default_rng(45)
    for name, seed in (("cornell", 77), ("default", 78)):
        tables, sc, desc = scenes[name]
        ref.use_scene(desc)
        orc.use_scene(desc)
        lights = rng.integers(0, len(tables["areaLights"]), N).astype(np.int32)
        r, sr = ref.area_light_point(lights, seed)
        o, so = orc.area_light_point(lights, seed)
        assert np.array_equal(sr, so), "RNG state after the call"
        assert (draws_used(seed, range(64), sr[:64]) == 4).all()
        u = uniforms(seed, range(N), 4)
        first = tables["areaLights"]["triangleIdx"][lights]
        tri = tables["triangles"][np.where(u[:, 3] > 0.5, first, first + 1)]   # decided on a float the two sides share: no threshold case
        inv = 1.0 / (u[:, 0] + u[:, 1] + u[:, 2])
        model = (f64(tri["vertex0"]) * (u[:, 0] * inv)[:, None] + f64(tri["vertex1"]) * (u[:, 1] * inv)[:, None]
                 + f64(tri["vertex2"]) * (u[:, 2] * inv)[:, None])
        check_floats(f"getAreaLightPoint [{name}]", r, o, model, floor=1.0)


def _shade_model(tables, sc, point, nrm, mat_idx, u):
    mats = tables["materials"][mat_idx]
    rad = np.zeros((len(point), 3))
    nr = np.zeros(len(point), bool)
    for li, light in enumerate(tables["areaLights"]):
        uu = u[:, 4 * li: 4 * li + 4]
        first = int(light["triangleIdx"])
        tri = tables["triangles"][np.where(uu[:, 3] > 0.5, first, first + 1)]
        inv = 1.0 / (uu[:, 0] + uu[:, 1] + uu[:, 2])
        lp = (f64(tri["vertex0"]) * (uu[:, 0] * inv)[:, None] + f64(tri["vertex1"]) * (uu[:, 1] * inv)[:, None]
              + f64(tri["vertex2"]) * (uu[:, 2] * inv)[:, None])
        # the light point the reference hands on is a float32
        lp = f64(lp.astype(np.float32))
        vis, w_i, d2, near_l = line_of_sight_model(sc, nrm, point, lp)
        nr |= near_l
        l_i = f64(light["power"])[None, :] / (4 * PI_F * d2)[:, None]
        cos_i = np.maximum(0.0, dot(nrm, w_i))
        term = cos_i[:, None] * l_i * f64(mats["diffuseColor"]) * f64(mats["diffAvg"])[:, None] * INVERSE_PI_F
        rad += np.where(vis[:, None], term, 0.0)
    return rad, nr


@pytest.mark.parametrize("name", ["cornell", "default"])
def test_shade(ref, orc, scenes, name):
    """shade, CudaTracer.cu:345-390: every area light costs four draws whether or not it is visible."""
    tables, sc, desc = scenes[name]
    ref.use_scene(desc)
    orc.use_scene(desc)
    rng = np.random.default_rng(46)
    seed = 4242
    p, nrm = surface_points(rng, ref, name, N, tables)
    diffuse = np.flatnonzero(tables["materials"]["diffAvg"] > 0)
    mat = rng.choice(diffuse, N).astype(np.int32)
    r, sr = ref.shade(p, nrm, mat, seed)
    o, so = orc.shade(p, nrm, mat, seed)
    lights = len(tables["areaLights"])
    assert np.array_equal(sr, so), "RNG state after the call"
    assert (draws_used(seed, range(64), sr[:64]) == 4 * lights).all()
    model, nr = _shade_model(tables, sc, f64(p), f64(nrm), mat, uniforms(seed, range(N), 4 * lights))
    keep = check_left_out(f"shade [{name}]", nr)
    lit = model.max(axis=1) > 0
    assert np.array_equal((f64(r).max(axis=1) > 0)[keep], lit[keep]) and np.array_equal((f64(o).max(axis=1) > 0)[keep], lit[keep])
    assert lit.sum() > N // 4
    # radiance off a surface a unit from the light is of order 1: that is the floor; the light point (a float32 both sides round on
    # their own before the visibility test) moves the result by its own ulp over the distance
    check_floats(f"shade [{name}]", r, o, model, floor=1.0, keep=keep)


def test_compute_eye_ray(ref, orc):
    """computeEyeRay, CudaTracer.cu:321-343, at 512 x 512 (DIM is fixed), for the default camera and moved ones."""
    rng = np.random.default_rng(47)
    seed = 0x5EED
    x = rng.integers(0, 512, N).astype(np.int32)
    y = rng.integers(0, 512, N).astype(np.int32)
    x[:4], y[:4] = [0, 511, 0, 511], [0, 0, 511, 511]
    for keys in ("", "wdqf", "ttgh" * 3 + "s"):
        cam = ptss.default_camera()
        for key in keys:
            ptss.move_camera(cam, key)
        r, sr = ref.eye_ray(x, y, cam, seed)
        o, so = orc.eye_ray(x, y, cam, seed)
        assert np.array_equal(sr, so), "RNG state after the call"
        seqs = (y.astype(np.int64) * 512 + x)
        assert (draws_used(seed, seqs[:32], sr[:32]) == 2).all()
        assert np.array_equal(r[:, :3].view(np.uint32), o[:, :3].view(np.uint32))   # the origin is the camera's position, copied
        u = uniforms(seed, seqs, 2)
        s = -2 * np.tan(float(cam.fieldOfView) * 0.5)
        inv = float(np.float32(1.0) / np.float32(512))
        z_near = float(cam.zNear)
        start = np.stack([((x + u[:, 0]) * inv - 0.5) * s, ((y + u[:, 1]) * inv - 0.5) * s, np.ones(N)], axis=1) * z_near
        q = np.array([cam.rotation.x, cam.rotation.y, cam.rotation.z, cam.rotation.w], dtype=np.float64)
        v = quat_rotate(np.broadcast_to(q, (N, 4)), start)
        model = v * (1.0 / np.sqrt(dot(v, v)))[:, None]
        check_floats(f"computeEyeRay keys={keys[:4] or '-'}", r[:, 3:], o[:, 3:], model, floor=1.0)


# ---- scattering ----------------------------------------------------------------------------------------------------------------
def _scatter_materials(rng, n):
    """Every class of material the reference's scenes hold (Scene.cpp:101-105, 128-140, 198-210, 239-245, 309-317), with colours
    that tell the returned lobe apart."""
    m = np.zeros(n, dtype=refprobe.MATERIAL_DTYPE)
    cls = rng.integers(0, 7, n)
    m["diffuseColor"], m["specularColor"] = (0.25, 0.5, 0.75), (0.375, 0.625, 0.875)
    m["indexOfRefraction"] = 1.0
    table = {   # diffAvg, specAvg, refrAvg, exponent, ior, flags, roughness
        0: (0.7, 0.0, 0.0, 0.0, 1.0, 0, 0.0),            # Lambert wall
        1: (0.35, 0.6, 0.0, 250.0, 2.5, 0, 0.0),         # red Phong sphere
        2: (0.0, 0.9, 0.9, 300.0, 1.55, 0, 0.0),         # Phong glass
        3: (0.0, 0.7, 0.7, np.inf, 1.55, 0, 0.0),        # mirror-lobe glass
        4: (0.1, 0.6, 0.0, np.inf, 1.7, 3, 0.3),         # Cook-Torrance
        5: (0.0, 0.9, 0.0, np.inf, 5.8, 1, 0.0),         # PURE_REFLECTION mirror: flags & 3 != 0 sends it down the Cook-Torrance branch
        6: (0.0, 0.8, 0.0, np.inf, 5.8, 0, 0.0),         # Fresnel mirror
    }
    for c, row in table.items():
        k = cls == c
        for field, v in zip(("diffAvg", "specAvg", "refrAvg", "specularExponent", "indexOfRefraction", "flags", "roughness"), row):
            m[field][k] = v
    m["roughness"][cls == 4] = rng.choice([0.1, 0.3, 0.5], (cls == 4).sum())
    return m, cls


LOBES = ("diffuse", "cook-torrance", "phong", "mirror", "refraction", "absorbed")


def _scatter_model(d, p, nrm, m, cos_in, u):
    """computeIndirectRadianceAndScatter, CudaTracer.cu:208-318, one case in float64: lobe, active, draws, origin, direction, colour,
    near (a lobe decision on its threshold)."""
    r = u[0]
    nr = False
    diff_avg, spec_avg, refr_avg = float(m["diffAvg"]), float(m["specAvg"]), float(m["refrAvg"])
    if diff_avg > 0:
        r -= diff_avg
        nr |= bool(near(r, 0.0, 1.0))
        if r < 0:
            dirn = lobe_sample_model(0, nrm[None], np.zeros(1), u[1:2], u[2:3])[0]
            return "diffuse", True, 3, p + BUMP * nrm, dirn, f64(m["diffuseColor"]), nr
    c, s2, n1, n2, n, f, near_tir = (float(a) for a in snell_fresnel_model(np.float64(m["indexOfRefraction"]), np.float64(cos_in)))
    flags = int(m["flags"])
    uses_fresnel = False
    if spec_avg > 0:
        if flags & 1:
            r -= spec_avg
        else:
            r -= spec_avg * f
            uses_fresnel = True
        nr |= bool(near(r, 0.0, 1.0))
        if r < 0:
            if flags & 3:
                h = lobe_sample_model(2, nrm[None], np.float64(m["roughness"])[None], u[1:2], u[2:3])[0]
                cos_h = abs(float(dot(d, h)))
                out = d - 2 * -cos_h * h
                half = out - d
                half = half * (1.0 / np.sqrt(dot(half, half)))
                nh, nl, vh, nv = abs(dot(nrm, half)), abs(dot(nrm, out)), abs(dot(d, half)), abs(c)
                with np.errstate(divide="ignore", invalid="ignore"):
                    geo = min(min(1.0, 2 * nh * nl / vh), 2 * nh * nv / vh)
                return "cook-torrance", True, 3, p + h * BUMP, out, f64(m["specularColor"]) * geo / nv, nr or (uses_fresnel and bool(near_tir))
            out = d - 2 * -c * nrm
            if np.isinf(m["specularExponent"]):
                return "mirror", True, 1, p + nrm * BUMP, out, f64(m["specularColor"]), nr or (uses_fresnel and bool(near_tir))
            dirn = lobe_sample_model(1, out[None], np.float64(m["specularExponent"])[None], u[1:2], u[2:3])[0]
            return "phong", True, 3, p + nrm * BUMP, dirn, f64(m["specularColor"]), nr or (uses_fresnel and bool(near_tir))
    nr |= uses_fresnel and bool(near_tir)
    if refr_avg > 0:
        r -= refr_avg * (1.0 - f)
        nr |= bool(near(r, 0.0, 1.0)) or bool(near_tir)
        if r < 0:
            with np.errstate(invalid="ignore"):
                cos_t = np.sqrt(1.0 - s2)
                w = n * d + (n * c - cos_t) * nrm
                w = w * (1.0 / np.sqrt(dot(w, w)))
            return "refraction", not s2 > 1.0, 1, p + w * BUMP, w, np.ones(3), nr
    return "absorbed", False, 1, None, None, np.zeros(3), nr


def test_compute_indirect_radiance_and_scatter(ref, orc):
    """computeIndirectRadianceAndScatter, CudaTracer.cu:208-318: the lobe taken, whether the ray stays active, the draws used, and
    the ray and colour that come out, for every material class of the reference's scenes, hit from outside and from inside."""
    rng = np.random.default_rng(51)
    seed = 0xABCD
    n_cases = N
    mats, cls = _scatter_materials(rng, n_cases)
    d, nrm = unit_vectors(rng, n_cases), unit_vectors(rng, n_cases)
    nrm[nrm[:, 1] < -0.98] *= -1   # rotateVectorToVector's cancellation (see test_rotate_vector_to_vector)
    p = rng.uniform(-5, 5, (n_cases, 3)).astype(np.float32)
    facing = dot(f64(d), f64(nrm)) < 0
    opaque = np.isin(cls, (0, 1, 4, 5, 6))
    d[opaque & ~facing] *= -1   # opaque things are only ever hit from outside; glass from both sides
    cos_i = (-dot(f64(d), f64(nrm))).astype(np.float32)
    dist = rng.uniform(0.1, 9, n_cases).astype(np.float32)
    ar, r, sr = ref.scatter(d, p, nrm, mats, cos_i, dist, seed)
    ao, o, so = orc.scatter(d, p, nrm, mats, cos_i, dist, seed)
    u = uniforms(seed, range(n_cases), 3)
    D, Nn, P = f64(d), f64(nrm), f64(p)
    lobe, active, draws, nr = [], np.zeros(n_cases, bool), np.zeros(n_cases, int), np.zeros(n_cases, bool)
    m_org, m_dir, m_col = np.full((n_cases, 3), np.nan), np.full((n_cases, 3), np.nan), np.zeros((n_cases, 3))
    for i in range(n_cases):
        lb, active[i], draws[i], org, dirn, col, nr[i] = _scatter_model(D[i], P[i], Nn[i], mats[i], float(cos_i[i]), u[i])
        lobe.append(lb)
        m_col[i] = col
        if org is not None:
            m_org[i], m_dir[i] = org, dirn
    lobe = np.array(lobe)
    keep = check_left_out("computeIndirectRadianceAndScatter", nr)
    for lb in LOBES:
        assert (lobe == lb).sum() > n_cases // 100, f"no cases of the {lb} lobe"
    # (at total internal reflection the reflectance is 1 and the refraction lobe has no weight left: refrRay's own TIR branch cannot
    # be reached from here, test_refr_ray covers it)
    assert active[lobe == "refraction"].all()
    # decisions: RNG state (= draws), active; the lobe shows in which of the two states and which colour came back
    assert np.array_equal(sr[keep], so[keep]), "RNG state after the call"
    assert np.array_equal(draws_used(seed, np.flatnonzero(keep)[:400], sr[keep][:400]), draws[keep][:400])
    assert np.array_equal(ar[keep], active[keep]) and np.array_equal(ao[keep], active[keep])
    fixed = keep & np.isin(lobe, ("diffuse", "phong", "mirror", "refraction", "absorbed"))
    assert np.array_equal(r[fixed, 6:], m_col[fixed].astype(np.float32)) and np.array_equal(o[fixed, 6:], r[fixed, 6:]), "the lobe's colour"
    moved = keep & (lobe != "absorbed") & active
    # the cancellations of the lobes (tests above): Lambert and Phong near their axis; refraction near the critical angle
    y_ok = np.ones(n_cases, bool)
    lam, pho, rfr = lobe == "diffuse", lobe == "phong", lobe == "refraction"
    y_ok[lam] = 1 - u[lam, 2] >= 2.0 ** -6
    y_ok[pho] = 1 - np.power(u[pho, 2], 2.0 / (f64(mats["specularExponent"][pho]) + 1.0)) >= 2.0 ** -6
    sn = ref.fresnel(mats["indexOfRefraction"], cos_i)
    y_ok[rfr] = 1.0 - f64(sn[rfr, 1]) > 2.0 ** -6
    # the rotation onto the outgoing axis cancels near -y for Phong as well
    y_ok[pho] &= (D[pho] - (2 * -f64(sn[pho, 0]))[:, None] * Nn[pho])[:, 1] > -0.98
    k = moved & y_ok
    check_floats("computeIndirect... origin", r[:, :3], o[:, :3], m_org, floor=1.0, keep=k)
    check_floats("computeIndirect... direction", r[:, 3:6], o[:, 3:6], m_dir, floor=1.0, keep=k)
    ct = keep & (lobe == "cook-torrance") & np.isfinite(m_col).all(axis=1)
    # Cook-Torrance's weight divides by |v . h| (twice: the half vector is the difference of two unit vectors 2 |v . h| apart) and by
    # |cosI|, and it is computed from a float32 microfacet normal: keep both divisors above 1/4
    h_ok = np.zeros(n_cases, bool)
    for i in np.flatnonzero(ct):
        half = m_dir[i] - D[i]
        half /= np.sqrt(dot(half, half))
        h_ok[i] = abs(dot(D[i], half)) > 0.25 and abs(float(cos_i[i])) > 0.25
    check_floats("computeIndirect... Cook-Torrance weight", r[:, 6:], o[:, 6:], m_col, floor=1.0, keep=ct & h_ok)


# ---- the tone map ----------------------------------------------------------------------------------------------------------------
def _tonemap_patterns():
    """A stride of 2^24 float patterns, every pattern within 2 of each byte breakpoint, and the specials. NaN is left out: C++
    leaves the conversion of NaN to an integer undefined, so the CPU build of the reference decides nothing about it."""
    pats = [np.arange(0, 2 ** 32, 2 ** 24, dtype=np.uint64)]
    lo = np.zeros(255, np.uint32)                                       # bisect each breakpoint b: the first pattern whose byte is >= b
    hi = np.full(255, np.float32(1.0).view(np.uint32), np.uint32)
    byte = np.arange(1, 256)
    while (hi - lo > 1).any():
        mid = ((lo.astype(np.uint64) + hi) // 2).astype(np.uint32)
        v = f64(mid.view(np.float32))
        q = np.floor(np.clip(255.0 * np.power(np.clip(v, 0, 1), GAMMA) + 0.5, 0, 255))
        up = q >= byte
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    around = (hi.astype(np.int64)[:, None] + np.arange(-8, 9)[None, :]).ravel()   # the float64 bisection may sit a pattern or two off
    pats.append(around[around >= 0].astype(np.uint64))
    specials = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-45, -1e-45, 1.1754944e-38, 1e-39, 0.5, 2.0, 3.4e38, -3.4e38,
                         np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))], dtype=np.float32)
    pats.append(specials.view(np.uint32).astype(np.uint64))
    p = np.unique(np.concatenate(pats)).astype(np.uint32)
    v = p.view(np.float32)
    return v[~np.isnan(v)]


def test_tone_map_bytes(ref, orc):
    """The tone map of writeToPixelsKernel, CudaTracer.cu:72-85, run through the kernel itself: clamp, gamma 1/2.2, * 255 + .5,
    clamp, truncate. Bytes are decisions; a pattern is left out only where float64 puts 255 * v^(1/2.2) + .5 within 4 ulp of an
    integer."""
    v = _tonemap_patterns()
    x = 255.0 * np.power(np.clip(f64(v), 0, 1), GAMMA) + 0.5
    nr = near(x, np.round(x), 256.0) & (x > 0.5) & (x < 255.5)
    # every pattern within 2 of a breakpoint is a threshold case by construction: the share is asserted on the strided sweep, the
    # breakpoints are compared without leave
    r, o = ref.tonemap(v), orc.tonemap(v)
    assert r.max() == 255 and r.min() == 0
    model = np.floor(np.clip(x, 0, 255)).astype(np.uint32)
    far = ~nr
    assert np.array_equal(r[far], model[far]), "reference against its float64 model"
    assert np.array_equal(r[far], o[far])
    on = np.flatnonzero(nr)
    print(f"[reference] tone map: {len(v)} patterns, {len(on)} on a breakpoint; of those the oracle differs at {(r[on] != o[on]).sum()}")
    # on the breakpoints themselves the two may differ by the last place of pow: never by more than one byte, and only there
    assert (np.abs(r[on].astype(int) - o[on].astype(int)) <= 1).all()
    sweep = np.arange(0, 2 ** 32, 2 ** 24, dtype=np.uint64).astype(np.uint32).view(np.float32)
    sweep = sweep[~np.isnan(sweep)]
    xs = 255.0 * np.power(np.clip(f64(sweep), 0, 1), GAMMA) + 0.5
    check_left_out("tone map (strided sweep)", near(xs, np.round(xs), 256.0) & (xs > 0.5) & (xs < 255.5))


# ---- the camera keys -----------------------------------------------------------------------------------------------------------
REFERENCE_KEYS = "wasdqefhgt"     # the keys moveCamera handles, CudaTracer.cu:826-867
ISSUE_KEYS = "wasdqezxcv"         # the ten the issue lists: z, x, c, v move nothing on either side


def _camera_model(cam, key):
    q = np.array([cam.rotation.x, cam.rotation.y, cam.rotation.z, cam.rotation.w], dtype=np.float64)
    pos = np.array([cam.position.x, cam.position.y, cam.position.z], dtype=np.float64)
    step, turn = float(np.float32(0.2)), float(np.float32(10.0) * np.float32(PI_F) / np.float32(180.0))
    moves = {"w": (0, 0, -step), "a": (-step, 0, 0), "s": (0, 0, step), "d": (step, 0, 0), "q": (0, step, 0), "e": (0, -step, 0)}
    turns = {"f": (0, turn, 0), "h": (0, -turn, 0), "g": (-turn, 0, 0), "t": (turn, 0, 0)}
    if key in moves:
        return q, pos + quat_rotate(q, np.array(moves[key]))
    if key in turns:
        e = np.array(turns[key]) * 0.5
        c, s = np.cos(e), np.sin(e)
        r = np.array([s[0] * c[1] * c[2] - c[0] * s[1] * s[2], c[0] * s[1] * c[2] + s[0] * c[1] * s[2],
                      c[0] * c[1] * s[2] - s[0] * s[1] * c[2], c[0] * c[1] * c[2] + s[0] * s[1] * s[2]])
        px, py, pz, pw = q
        rx, ry, rz, rw = r
        out = np.array([pw * rx + px * rw + py * rz - pz * ry, pw * ry + py * rw + pz * rx - px * rz,
                        pw * rz + pz * rw + px * ry - py * rx, pw * rw - px * rx - py * ry - pz * rz])
        return out / np.sqrt(dot(out, out)), pos
    return q, pos


def test_move_camera_every_key(ref):
    """moveCamera, CudaTracer.cu:822-870, against the host mirror (ptss_camera_move) for every key the reference handles and every
    key of the issue's list, from the default camera and from cameras already moved."""
    rng = np.random.default_rng(61)
    d0, h0 = ref.default_camera(), ptss.default_camera()
    assert bytes(d0) == bytes(h0), "Camera() defaults, RenderStructs.h:51-52"
    keys = sorted(set(REFERENCE_KEYS + ISSUE_KEYS + " 0\x1b"))
    starts = [""] + ["".join(rng.choice(list(REFERENCE_KEYS), 12)) for _ in range(40)]
    got_r, got_h, model = [], [], []
    for prefix in starts:
        cam = ptss.default_camera()
        for k in prefix:
            ptss.move_camera(cam, k)
        for key in keys:
            moved_r, after_r = ref.move_camera(cam, key)
            after_h = ptss.default_camera()
            C.memmove(C.byref(after_h), C.byref(cam), C.sizeof(cam))
            moved_h = ptss.move_camera(after_h, key)
            assert moved_r == moved_h == (key in REFERENCE_KEYS), key
            if not moved_r:
                assert bytes(after_r) == bytes(cam) and bytes(after_h) == bytes(cam)
            for name in ("zNear", "zFar", "fieldOfView"):
                assert getattr(after_r, name) == getattr(after_h, name)
            q, pos = _camera_model(cam, key)
            got_r.append(np.concatenate([refprobe.cam10(after_r)[:4], refprobe.cam10(after_r)[4:7]]))
            got_h.append(np.concatenate([refprobe.cam10(after_h)[:4], refprobe.cam10(after_h)[4:7]]))
            model.append(np.concatenate([q, pos]))
    got_r, got_h, model = np.array(got_r), np.array(got_h), np.array(model)
    check_floats("moveCamera rotation (host mirror)", got_r[:, :4], got_h[:, :4], model[:, :4], floor=1.0)
    check_floats("moveCamera position (host mirror)", got_r[:, 4:], got_h[:, 4:], model[:, 4:], floor=1.0)
