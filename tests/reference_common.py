"""Shared by tests/test_reference_*.py and tests/golden/make_reference_golden.py: where the reference's CPU build is, float64
numpy models of the reference's formulas, and the tolerance rule.

THE RULE (one for every float the reference computes). Reference and oracle are two float32 roundings of the same real value.
For each function a float64 model of the reference's formula gives that value; e_ref is the largest distance of the compiled
reference from the model over the test's inputs, in ulp of the output (for a vector: of its largest component; never less than the
ulp of the function's stated floor, which keeps results that cancel to almost nothing from being measured in their own tiny
ulp). The oracle passes when its distance from the reference is at most 3 * e_ref + 1 of the same ulp: it may be as far from the
truth as twice the reference, plus the final rounding. e_ref itself must stay at or below 64, so that a wrong model fails the
test instead of loosening it.

DECISIONS (hit or miss, which primitive, which lobe, the RNG state afterwards, bytes, integers) must be equal. A case may be left
out only where the float64 model puts the deciding quantity within 4 float32 ulp of its threshold — ulp taken at the scale of
the quantity's operands, the product of the operand magnitudes for a dot or cross product — and at most 0.5 % of a function's
cases may be left out."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "cuda-path-tracer-ss_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import refprobe  # noqa: E402

E_REF_CAP = 64.0          # ulp
MAX_LEFT_OUT = 0.005      # share of a function's cases
NEAR_ULPS = 4.0
PI_F = float(np.float32(3.14159265358979323846))      # RenderStructs.h:10
INVERSE_PI_F = float(np.float32(0.31830988618))       # CudaTracer.h:4
BUMP = float(np.float32(1e-4))                        # CudaTracer.h:6
TRI_EPS = float(np.float32(1e-7))                     # Primitives.h:31
GAMMA = float(np.float32(1) / np.float32(2.2))        # CudaTracer.h:7

MEASURED = {}   # function -> (e_ref, oracle's distance), both in ulp: printed by the tests, copied into DESIGN.md §4


def require_reference():
    """Probes("ref"), or skip where there is neither a reference nor its library; FAIL where the reference is there and the
    library is not (a build that failed must not pass as a skip)."""
    state = refprobe.availability()
    if state == "absent":
        pytest.skip("no reference directory and no oracle/_ref/libref_probe.so on this machine")
    assert state == "built", ("the reference is at %s but oracle/_ref/libref_probe.so is missing: oracle/build.py build_ref() failed "
                              "(see the build log)" % refprobe.reference_dir())
    return refprobe.Probes("ref")


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def ulp_at(mag):
    """float32 ulp at magnitude `mag` (float64 array)."""
    m = np.minimum(np.abs(np.asarray(mag, dtype=np.float64)), 3.0e38).astype(np.float32)
    return np.spacing(m).astype(np.float64)


def unit_of(truth, floor, vector):
    t = np.abs(np.asarray(truth, dtype=np.float64))
    if vector:
        t = t.max(axis=-1, keepdims=True)
    return ulp_at(np.maximum(np.nan_to_num(t, nan=0.0, posinf=3.0e38), floor))


def distance_ulp(a, b, truth, floor, vector):
    """|a - b| in the unit of the rule; NaN against NaN and equal infinities count as 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / unit_of(truth, floor, vector)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    return np.where(same, 0.0, d)


def check_floats(name, ref, orc, model, floor, vector=True, keep=None):
    """Applies THE RULE to one output; returns (e_ref, oracle's distance). keep: boolean mask of the cases that count."""
    ref, orc, model = np.asarray(ref), np.asarray(orc), np.asarray(model, dtype=np.float64)
    floor_text = f"{floor:g}" if np.isscalar(floor) else "per case"
    if not np.isscalar(floor):   # one floor per case: the magnitude of what the output is a difference of
        floor = np.asarray(floor, dtype=np.float64)
        if keep is not None:
            floor = floor[keep]
        if vector:
            floor = floor[:, None]
    if keep is not None:
        ref, orc, model = ref[keep], orc[keep], model[keep]
    assert len(ref), name
    e = distance_ulp(ref, model, model, floor, vector)
    assert not np.isnan(e).any(), f"{name}: the reference and the model disagree about NaN"
    e_ref = float(e.max())
    d = distance_ulp(orc, ref, model, floor, vector)
    assert not np.isnan(d).any(), f"{name}: the oracle and the reference disagree about NaN"
    dist = float(d.max())
    prev = MEASURED.get(name, (0.0, 0.0))
    MEASURED[name] = (max(prev[0], e_ref), max(prev[1], dist))
    print(f"[reference] {name:<34s} cases {len(ref):6d}  e_ref {e_ref:8.3f} ulp  oracle-reference {dist:8.3f} ulp  (floor {floor_text})")
    assert e_ref <= E_REF_CAP, f"{name}: the compiled reference is {e_ref:.1f} ulp from the float64 model (cap {E_REF_CAP}): wrong model or ill-conditioned inputs"
    assert dist <= 3.0 * e_ref + 1.0, f"{name}: the oracle is {dist:.2f} ulp from the reference, allowed 3 * {e_ref:.2f} + 1"
    return e_ref, dist


def check_left_out(name, near):
    share = float(np.mean(near)) if len(near) else 0.0
    print(f"[reference] {name:<34s} cases {len(near):6d}  left out as within {NEAR_ULPS:g} ulp of a threshold: {int(np.sum(near))} ({100 * share:.3f} %)")
    assert share <= MAX_LEFT_OUT, f"{name}: {100 * share:.2f} % of the cases sit on a threshold; choose other input ranges"
    return ~np.asarray(near, dtype=bool)


def near(q, threshold, scale):
    """The float64 quantity q is within NEAR_ULPS float32 ulp (at `scale`) of `threshold`."""
    return np.abs(np.asarray(q) - threshold) <= NEAR_ULPS * ulp_at(np.maximum(np.abs(scale), np.abs(threshold)))


def norm(v):
    return np.sqrt((v * v).sum(axis=-1))


def dot(a, b):
    return (a * b).sum(axis=-1)


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / norm(v)[:, None]).astype(np.float32)


# ---- float64 models (inputs: float32 values, widened) ------------------------------------------------------------------
def sphere_model(c, r, o, d, tmax):
    """Sphere::intersectRay, Primitives.h:107-175. Arrays broadcast; returns hit, t, point, normal, near."""
    v = o - c
    vd, vv = norm(v) * norm(d), dot(v, v)
    b = 2 * dot(d, v)
    cc = vv - r * r
    disc = b * b - 4 * cc
    nr = near(disc, 0.0, np.maximum(4 * vd * vd, 4 * np.maximum(vv, r * r)))
    with np.errstate(invalid="ignore"):
        s = np.sqrt(np.maximum(disc, 0.0))
    t0, t1 = (-b + s) * 0.5, (-b - s) * 0.5
    tscale = np.maximum(np.abs(b), s)
    nr = nr | near(t0, 0.0, tscale) | near(t1, 0.0, tscale)
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    t = np.where(lo < 0, hi, lo)
    hit = (disc >= 0) & ~((t0 < 0) & (t1 < 0))
    with np.errstate(invalid="ignore"):
        nr = nr | (hit & np.isfinite(tmax) & near(t, tmax, np.maximum(tscale, np.abs(np.where(np.isfinite(tmax), tmax, 0.0)))))
        hit = hit & ~(t > tmax)
    point = o + d * t[..., None]
    n = point - c
    with np.errstate(invalid="ignore", divide="ignore"):
        normal = n * (1.0 / np.sqrt(dot(n, n)))[..., None]
    return hit, t, point, normal, nr


def triangle_model(v0, v1, v2, n0, n1, n2, o, d, tmax):
    """Triangle::intersectRay, Primitives.h:25-83. Returns hit, dist, point, normal, near."""
    e1, e2 = v1 - v0, v2 - v0
    q = np.cross(d, e2)
    det = dot(e1, q)
    s = o - v0
    r = np.cross(s, e1)
    le1, le2, ld, ls = norm(e1), norm(e2), norm(d), norm(s)
    nr = near(np.abs(det), TRI_EPS, le1 * ld * le2)
    ok = np.abs(det) > TRI_EPS
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        num = dot(e2, r)
        dist = num * inv
        nr = nr | near(num, 0.0, le2 * ls * le1)
        fin = np.isfinite(tmax)
        nr = nr | (fin & near(dist, np.where(fin, tmax, 0.0), np.maximum(np.abs(np.where(fin, tmax, 0.0)), le2 * ls * le1 * np.abs(inv))))
        ok = ok & ~((dist <= 0) | (dist > tmax))
        a1, a2 = dot(s, q), dot(d, r)
        w1, w2 = a1 * inv, a2 * inv
        w0 = 1.0 - (w1 + w2)
        nr = nr | near(a1, 0.0, ls * ld * le2) | near(a2, 0.0, ld * ls * le1)
        nr = nr | near(w0, 0.0, np.maximum(1.0, (ls * ld * le2 + ld * ls * le1) * np.abs(inv)))
        ok = ok & ~((w0 < 0) | (w1 < 0) | (w2 < 0))
    normal = n0 * w0[..., None] + n1 * w1[..., None] + n2 * w2[..., None]
    point = o + d * dist[..., None]
    return ok, dist, point, normal, nr


def scene_arrays(tables):
    s, t = tables["spheres"], tables["triangles"]
    return dict(c=f64(s["position"]), r=f64(s["radius"]), v0=f64(t["vertex0"]), v1=f64(t["vertex1"]), v2=f64(t["vertex2"]),
                n0=f64(t["normal0"]), n1=f64(t["normal1"]), n2=f64(t["normal2"]), smat=s["materialIdx"], tmat=t["materialIdx"])


def closest_hit_model(sc, o, d, tmax):
    """The loops of pathTraceKernel (CudaTracer.cu:121-141) in float64: kind, prim, t, point, normal, near. A primitive replaces
    the current hit when its t is not greater than the current distance, so of equal distances the LAST wins."""
    n = len(o)
    ns, nt = len(sc["r"]), len(sc["v0"])
    O, D = o[:, None, :], d[:, None, :]
    inf = np.full((n, 1), np.inf)
    ts = np.full((n, 0), np.inf)
    nr = np.zeros(n, bool)
    cols = []
    if ns:
        hit, t, p, nm, nrs = sphere_model(sc["c"][None], sc["r"][None], O, D, inf)
        cols.append((np.where(hit, t, np.inf), p, nm, nrs))
    if nt:
        hit, t, p, nm, nrt = triangle_model(sc["v0"][None], sc["v1"][None], sc["v2"][None], sc["n0"][None], sc["n1"][None], sc["n2"][None],
                                            O, D, inf)
        cols.append((np.where(hit, t, np.inf), p, nm, nrt))
    T = np.concatenate([c[0] for c in cols], axis=1)
    P = np.concatenate([c[1] for c in cols], axis=1)
    N = np.concatenate([c[2] for c in cols], axis=1)
    NR = np.concatenate([c[3] for c in cols], axis=1)
    T = np.where(T > tmax[:, None], np.inf, T)
    with np.errstate(invalid="ignore"):
        NR = NR | (np.isfinite(tmax)[:, None] & near(T, np.where(np.isfinite(tmax), tmax, 0.0)[:, None], np.abs(np.where(np.isfinite(T), T, 0.0))))
    # the winner: the smallest t, the last index among equals
    rev = T[:, ::-1]
    k = T.shape[1] - 1 - np.argmin(rev, axis=1)
    rows = np.arange(n)
    best = T[rows, k]
    hit = np.isfinite(best)
    # near: a primitive that decides on a threshold and could beat (or be) the winner, or a runner-up within 4 ulp of the winner
    could = NR & ~(np.where(np.isfinite(T), T, -np.inf) > (best[:, None] + 4 * ulp_at(np.where(hit, best, 0.0))[:, None]))
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(T) & (np.abs(T - best[:, None]) <= NEAR_ULPS * ulp_at(np.where(hit, best, 0.0))[:, None])
    tie[rows, k] = False
    nr = could.any(axis=1) | tie.any(axis=1)
    kind = np.where(~hit, 0, np.where(k < ns, 1, 2))
    prim = np.where(~hit, -1, np.where(k < ns, k, k - ns))
    return kind, prim, best, P[rows, k], N[rows, k], nr


def line_of_sight_model(sc, normal, p0, p1):
    """lineOfSight, CudaTracer.cu:420-455: visible, w_i, distance2, near."""
    off = p1 - p0
    d2 = dot(off, off)
    dist = np.sqrt(d2)
    w = off / dist[:, None]
    o = p0 + BUMP * normal
    tmax = dist - 2 * BUMP
    n = len(p0)
    blocked, nr = np.zeros(n, bool), np.zeros(n, bool)
    O, D, TM = o[:, None, :], w[:, None, :], tmax[:, None]
    if len(sc["r"]):
        hit, _, _, _, nrs = sphere_model(sc["c"][None], sc["r"][None], O, D, TM)
        blocked |= hit.any(axis=1)
        nr |= nrs.any(axis=1)
    if len(sc["v0"]):
        hit, _, _, _, nrt = triangle_model(sc["v0"][None], sc["v1"][None], sc["v2"][None], sc["n0"][None], sc["n1"][None], sc["n2"][None], O, D, TM)
        blocked |= hit.any(axis=1)
        nr |= nrt.any(axis=1)
    return ~blocked, w, d2, nr


def quat_rotate(q, v):
    """glm quat * vec3 with q = (x, y, z, w) rows."""
    u = q[..., :3]
    uv = np.cross(u, v)
    uuv = np.cross(u, uv)
    return v + 2 * q[..., 3:4] * uv + 2 * uuv


def rotate_v2v_model(src, tgt):
    """rotateVectorToVector, CudaTracer.cu:579-585, as (x, y, z, w); identity where the length is not positive."""
    axis = np.cross(src, tgt)
    q = np.concatenate([axis, (1.0 + dot(src, tgt))[..., None]], axis=-1)
    ln = np.sqrt(dot(q, q))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = q / ln[..., None]
    ident = np.zeros_like(q)
    ident[..., 3] = 1.0
    return np.where((ln <= 0)[..., None], ident, out)


Y_AXIS = np.array([0.0, 1.0, 0.0])


def lobe_sample_model(kind, axis, param, u1, u2):
    """randomDirection{Lambert, Phong, Beckmann}, CudaTracer.cu:533-577; u1, u2: the two uniforms in draw order."""
    if kind == 2:
        with np.errstate(divide="ignore"):
            theta = np.arctan(-param * param * np.log(1.0 - u1))
        phi = u2 * 2 * PI_F
        sample = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=-1)
    else:
        theta = u1 * 2 * PI_F
        y = np.sqrt(u2) if kind == 0 else np.power(u2, 1.0 / (param + 1.0))
        r = np.sqrt(1 - y * y)
        sample = np.stack([r * np.cos(theta), y, r * np.sin(theta)], axis=-1)
    return quat_rotate(rotate_v2v_model(np.broadcast_to(Y_AXIS, axis.shape), axis), sample)


def snell_fresnel_model(refr, cos_i):
    """computeSinT2AndRefractiveIndexes + computeFresnelForReflectance, CudaTracer.cu:457-494: cosI', sinT2, n1, n2, n, F, near."""
    outside = cos_i > 0
    c = np.where(outside, cos_i, -cos_i)
    n1 = np.where(outside, 1.0, refr)
    n2 = np.where(outside, refr, 1.0)
    n = n1 / n2
    sin_t2 = n * n * (1.0 - c * c)
    nr = near(sin_t2, 1.0, np.maximum(1.0, n * n))
    with np.errstate(invalid="ignore", divide="ignore"):
        cos_t = np.sqrt(1.0 - sin_t2)
        rs = (n1 * c - n2 * cos_t) / (n1 * c + n2 * cos_t)
        rp = (n2 * c - n1 * cos_t) / (n2 * c + n1 * cos_t)
        f = np.where(sin_t2 > 1.0, 1.0, (rs * rs + rp * rp) * 0.5)
    return c, sin_t2, n1, n2, n, f, nr


def uniforms(seed, sequences, count):
    """The first `count` uniforms of curand_init(seed, s, 0) for every s, from the oracle's generator (held against rocRAND's
    tables by tests/test_xorwow.py and against the reference build's stand-in by test_reference_functions.py)."""
    import oracle
    return np.stack([oracle.probe_rng(seed, int(s), count)[2] for s in sequences]).astype(np.float64)


def draws_used(seed, sequences, states, max_draws=64):
    """How many draws separate curand_init(seed, s, 0) from each given state (asserts that it is reachable)."""
    import oracle
    out = np.zeros(len(sequences), np.int64)
    for k, s in enumerate(sequences):
        st, _, _ = oracle.probe_rng(seed, int(s), 1)
        v = [int(x) for x in st[:5]]
        d = int(st[5])
        target = [int(x) for x in states[k]]
        n = 0
        while v + [d] != target:
            assert n < max_draws, "state not reachable from the stream's start"
            t = v[0] ^ (v[0] >> 2)
            v = v[1:] + [((v[4] ^ (v[4] << 4)) ^ (t ^ (t << 1))) & 0xFFFFFFFF]
            d = (d + 362437) & 0xFFFFFFFF
            n += 1
        out[k] = n
    return out


# ---- inputs on the reference's two scenes ---------------------------------------------------------------------------------
def scene_rays(rng, name, n):
    """Rays from inside the box of either scene in every direction, and from the camera through the frame."""
    half = 4.0 if name == "cornell" else 5.0
    o = rng.uniform(-0.9 * half, 0.9 * half, (n, 3))
    o[:, 2] = rng.uniform(-1.9 * half, -0.1, n)
    d = unit_vectors(rng, n).astype(np.float64)
    eye = rng.random(n) < 0.3
    # the default scene's front wall lies in the camera's own plane z = 0 (Scene.cpp:353-357): from the camera itself every ray
    # decides its distance to that wall on the threshold 0, so the eye of this test stands a quarter unit inside
    o[eye] = 0.0 if name == "cornell" else (0.0, 0.0, -0.25)
    d[eye] = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), -np.ones(n)], axis=1)[eye]
    d /= norm(d)[:, None]
    return np.concatenate([o, d], axis=1).astype(np.float32)


def surface_points(rng, ref, name, n, tables):
    """Points on the scene's surfaces with their normals: where rays land. Not on the lights: the segment from a point of a light
    to another point of it lies in the light's plane (and in the planes of floor and ceiling), det = 0 by construction."""
    rays = scene_rays(rng, name, 3 * n)
    kind, _, out = ref.closest_hit(rays)
    emits = tables["materials"]["emmitance"].max(axis=1) > 0
    ok = (kind > 0) & np.isfinite(out).all(axis=1)
    ok &= ~emits[np.clip(out[:, 7].astype(int), 0, len(emits) - 1)]
    # ... and a tenth of a unit clear of every light's plane (the lights hang 0.01 off floor and ceiling, Scene.cpp:290, 361-367):
    # from the strip of wall beside a light the segment to it runs almost inside that plane, a determinant on its threshold
    for first in tables["areaLights"]["triangleIdx"]:
        tri = tables["triangles"][first]
        ok &= np.abs(dot(f64(out[:, 1:4]) - f64(tri["vertex0"]), f64(tri["normal0"]))) >= 0.1
    assert ok.sum() >= n
    return out[ok][:n, 1:4], out[ok][:n, 4:7]




def los_rays(normal, p0, p1):
    """The ray and limit lineOfSight builds from its arguments (CudaTracer.cu:423-432), in float32 with the reference's operations in
    the reference's order: offset, dot (x, y, z left to right, no fma), sqrt, offset / distance, point0 + eps * normal,
    distance - 2 * eps. Returns (rays (n, 6), tmax (n,)) float32."""
    f = np.float32
    n, a, b = np.asarray(normal, f), np.asarray(p0, f), np.asarray(p1, f)
    off = b - a
    d2 = (off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2]
    dist = np.sqrt(d2)
    w = off / dist[:, None]
    o = a + f(1e-4) * n
    return np.concatenate([o, w], axis=1).astype(f), (dist - f(2) * f(1e-4)).astype(f)


def query_cases(rng, ref, name, tables, n):
    """n segments (normal, point0, point1) on one of the reference's scenes for the recorded queries: from surface points to points
    on the lights and anywhere in the box, and from the eye into the frame (normal 0: the ray starts at the eye itself)."""
    p0, nrm = surface_points(rng, ref, name, n, tables)
    lights = tables["areaLights"]["triangleIdx"]
    tri = tables["triangles"][rng.choice(lights, n) + rng.integers(0, 2, n)]
    w = rng.dirichlet((1, 1, 1), n)
    on_light = f64(tri["vertex0"]) * w[:, :1] + f64(tri["vertex1"]) * w[:, 1:2] + f64(tri["vertex2"]) * w[:, 2:]
    half = 4.0 if name == "cornell" else 5.0
    anywhere = np.stack([rng.uniform(-0.9 * half, 0.9 * half, n), rng.uniform(-0.9 * half, 0.9 * half, n), rng.uniform(-1.9 * half, -0.1, n)], axis=1)
    p1 = np.where((rng.random(n) < 0.5)[:, None], on_light, anywhere)
    eye = rng.random(n) < 0.25
    p0, nrm = p0.copy(), nrm.copy()
    p0[eye] = 0.0 if name == "cornell" else (0.0, 0.0, -0.25)   # see scene_rays
    nrm[eye] = 0.0
    far = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), -np.ones(n)], axis=1) * 30.0   # beyond the back wall
    p1[eye] = (f64(p0) + far)[eye]
    return nrm.astype(np.float32), p0.astype(np.float32), p1.astype(np.float32)


def hit_floors(rays, dist, kind, prim, tables):
    """The per-case floors of the closest-hit floats, as test_closest_hit_loops states them; and which cases count (sphere hits whose
    discriminant keeps 2^-6 of its larger term)."""
    sc = scene_arrays(tables)
    o, d = f64(rays[:, :3]), f64(rays[:, 3:])
    sph = kind == 1
    ok = np.ones(len(rays), bool)
    span = norm(o) + np.where(np.isfinite(dist), f64(dist), 0.0) + 1.0
    nfloor = np.ones(len(rays))
    if len(sc["r"]):
        c, r = sc["c"][np.where(sph, prim, 0)], sc["r"][np.where(sph, prim, 0)]
        v = o - c
        b2, c4 = (2 * dot(d, v)) ** 2, 4 * (dot(v, v) - r * r)
        ok = ~sph | (b2 - c4 >= 2.0 ** -6 * np.maximum(b2, 4 * np.maximum(dot(v, v), r * r)))
        nfloor = np.where(sph, np.maximum(1.0, span / r), 1.0)
    return span, nfloor, ok
