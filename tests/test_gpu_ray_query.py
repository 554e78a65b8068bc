"""Batched ray queries (ptss_intersect / ptss_occluded) against the oracle's own primitive tests, applied in the reference's order.

The expected closest hit of a ray is intersectScene's loop (CudaTracer.cu:120-141) run on the CPU with the oracle's
Sphere::intersectRay and Triangle::intersectRay (oracle_probe_sphere / oracle_probe_triangle, the functions behind
oracle.probe_sphere / oracle.probe_triangle, called on the scene's own records): spheres 0..S-1 then triangles 0..T-1 with a
running distance that starts at tmax, keeping the last accepted primitive. Occlusion: some primitive accepts with limit tmax.
Every field is compared by its bits (NaN against NaN: x86 and gfx950 make different default NaNs). The rays mix camera rays,
random rays inside and outside the scene, rays leaving primitives, exact ties, tmax at and around hit distances, and
non-unit, zero, huge, infinite and NaN inputs, shuffled into the same waves as ordinary rays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import ptss
from meshgen import icosphere_obj, translate_scale, write
from test_gpu_kernel_coverage import SCENES as COVERAGE_SCENES, compare
from test_gpu_fuzz_scenes import random_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
INF = np.float32(np.inf)
NAN = np.float32(np.nan)


# ---- the oracle loops ---------------------------------------------------------------------------------------------------
def oracle_closest(desc, ray):
    """(kind, primitive, materialIdx, distance, point[3], normal[3]) of intersectScene with `distance` = tmax."""
    L = oracle.lib()
    r6 = (C.c_float * 6)(*[float(v) for v in ray[0:3]], *[float(v) for v in ray[4:7]])
    out = (C.c_float * 8)()
    dist = float(ray[3])
    res = (0, -1, -1, np.float32(ray[3]), np.zeros(3, np.float32), np.zeros(3, np.float32))
    for k in range(desc.numSpheres):
        if L.oracle_probe_sphere(C.byref(desc.spheres[k]), r6, dist, out):
            v = np.array(out[:], np.float32)
            dist = float(v[0])
            res = (1, k, desc.spheres[k].materialIdx, v[0], v[1:4], v[4:7])
    for k in range(desc.numTriangles):
        if L.oracle_probe_triangle(C.byref(desc.triangles[k]), r6, dist, out):
            v = np.array(out[:], np.float32)
            dist = float(v[0])
            res = (2, k, desc.triangles[k].materialIdx, v[0], v[1:4], v[4:7])
    return res


def oracle_occluded(desc, ray):
    L = oracle.lib()
    r6 = (C.c_float * 6)(*[float(v) for v in ray[0:3]], *[float(v) for v in ray[4:7]])
    out = (C.c_float * 8)()
    tmax = float(ray[3])
    return int(any(L.oracle_probe_sphere(C.byref(desc.spheres[k]), r6, tmax, out) for k in range(desc.numSpheres)) or
               any(L.oracle_probe_triangle(C.byref(desc.triangles[k]), r6, tmax, out) for k in range(desc.numTriangles)))


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(both_nan | (a.view(np.uint32) == b.view(np.uint32))))


def check_hits(desc, rays, hits, occ, axis_normals=False):
    assert hits.shape == (len(rays),) and occ.shape == (len(rays),)
    for i, ray in enumerate(rays):
        kind, prim, mat, dist, point, normal = oracle_closest(desc, ray)
        h = hits[i]
        what = (i, ray.tolist(), (kind, prim, mat, float(dist)), (int(h["kind"]), int(h["primitive"]), int(h["materialIdx"]), float(h["distance"])))
        assert (h["kind"], h["primitive"], h["materialIdx"]) == (kind, prim, mat), what
        assert same_bits(h["distance"], dist), what
        assert same_bits(h["point"], point) and same_bits(h["normal"], normal), what
        if kind != 2:
            assert h["w1"] == 0 and h["w2"] == 0 and not np.signbit(h["w1"]) and not np.signbit(h["w2"]), what
        elif axis_normals and np.isfinite(normal).all():   # normals (1,0,0), (0,1,0), (0,0,1): the normal is (w0, w1, w2)
            # (for finite weights: an infinite weight makes 0 * inf = NaN in the other components)
            assert same_bits(h["w1"], normal[1]) and same_bits(h["w2"], normal[2]), what
        if kind == 0:
            assert not h["point"].any() and not h["normal"].any(), what
        assert occ[i] == oracle_occluded(desc, ray), what


# ---- rays ---------------------------------------------------------------------------------------------------------------
def scene_box(desc):
    pts = [np.array([s.position.x, s.position.y, s.position.z]) for s in (desc.spheres[k] for k in range(desc.numSpheres))]
    for k in range(desc.numTriangles):
        t = desc.triangles[k]
        pts += [np.array([v.x, v.y, v.z]) for v in (t.vertex0, t.vertex1, t.vertex2)]
    pts = np.array(pts) if pts else np.zeros((1, 3))
    return pts.min(0), pts.max(0)


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def surface_points(desc, rng, n):
    out = []
    for _ in range(n):
        if desc.numSpheres and (not desc.numTriangles or rng.random() < 0.5):
            s = desc.spheres[int(rng.integers(desc.numSpheres))]
            out.append(np.array([s.position.x, s.position.y, s.position.z]) + s.radius * unit(rng, 1)[0])
        else:
            t = desc.triangles[int(rng.integers(desc.numTriangles))]
            a, b = rng.random(2)
            if a + b > 1:
                a, b = 1 - a, 1 - b
            v = [np.array([p.x, p.y, p.z]) for p in (t.vertex0, t.vertex1, t.vertex2)]
            out.append(v[0] + a * (v[1] - v[0]) + b * (v[2] - v[0]))
    return np.array(out, np.float32)


def adversarial(rng, lo, hi):
    """Non-unit, zero, huge (|d|^2 >= 2^30), infinite and NaN directions and origins, far origins, and odd tmax values."""
    c = ((lo + hi) / 2).astype(np.float32)
    rows = []
    for d, o, t in [((0, 0, -7.5), c, INF), ((0, 0, -1e-3), c, INF), ((0, 0, 0), c, INF), ((4e4, 1e3, -3e4), c, INF),
                    ((0, 0, -1), c + np.float32(1e20), INF), ((0, 0, -1), (1e30, 0, 0), INF), ((NAN, 0, -1), c, INF),
                    ((0, INF, -1), c, INF), ((0, 0, -1), (NAN, 0, 0), INF), ((0, 0, -1), (0, -INF, 0), INF),
                    ((0.3, -0.2, -1), c, NAN), ((0.3, -0.2, -1), c, 0.0), ((0.3, -0.2, -1), c, -0.0), ((0.3, -0.2, -1), c, -2.0),
                    ((1e-30, 1e-30, -1e-30), c, INF), ((3e19, -2e19, 1e19), c, INF), ((-INF, INF, 0), c, INF),
                    ((0.1, 0.2, -0.97), (c[0], c[1], hi[2] + 3), 1e-3)]:
        rows.append(ptss.make_rays([o], [d], t)[0])
    for _ in range(24):   # random unit-ish rays with one broken component
        o = rng.uniform(lo - 2, hi + 2).astype(np.float32)
        d = unit(rng, 1)[0]
        j = int(rng.integers(3))
        if rng.random() < 0.5:
            d[j] = rng.choice([NAN, INF, -INF, np.float32(3e5), np.float32(0)])
        else:
            o[j] = rng.choice([NAN, INF, np.float32(-1e25)])
        rows.append(ptss.make_rays([o], [d], rng.choice([INF, np.float32(5.0), NAN]))[0])
    return np.array(rows, np.float32)


def query_rays(desc, seed, n_random=96, cam_size=(12, 8)):
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(desc)
    lo, hi = lo.astype(np.float32), hi.astype(np.float32)
    parts = [ptss.camera_rays(ptss.default_camera(), *cam_size)]
    inside = rng.uniform(lo, hi, size=(n_random, 3)).astype(np.float32)
    outside = (rng.uniform(lo, hi, size=(n_random // 2, 3)) + rng.choice([-1, 1], size=(n_random // 2, 3)) * (hi - lo + 1) * 2).astype(np.float32)
    parts += [ptss.make_rays(inside, unit(rng, n_random)), ptss.make_rays(outside, -outside / np.linalg.norm(outside, axis=1, keepdims=True))]
    if desc.numSpheres + desc.numTriangles:
        parts.append(ptss.make_rays(surface_points(desc, rng, n_random // 2), unit(rng, n_random // 2)))
    parts.append(adversarial(rng, lo, hi))
    rays = np.concatenate(parts)
    return rays[rng.permutation(len(rays))]


def with_tmax_at_hits(desc, rays, hits, count=24):
    """Copies of rays that hit something with tmax = the hit distance (accepted: `dist > distance` is false), one ulp below it,
    half of it (between the origin and the hit), 0 and -1."""
    idx = [i for i in range(len(rays)) if hits[i]["kind"] != 0 and np.isfinite(hits[i]["distance"])][:count]
    out = []
    for i in idx:
        d = np.float32(hits[i]["distance"])
        for t in (d, np.nextafter(d, np.float32(0)), d * np.float32(0.5), np.float32(0), np.float32(-1)):
            r = rays[i].copy()
            r[3] = t
            out.append(r)
    return np.array(out, np.float32).reshape(-1, 8)


# ---- scenes -------------------------------------------------------------------------------------------------------------
def duplicate_spheres(holder, pairs):
    for src, dst in pairs:
        C.memmove(C.byref(holder.desc.spheres[dst]), C.byref(holder.desc.spheres[src]), C.sizeof(ptss.Sphere))
    return holder


def icosphere_scene(tmp_path):
    s = ptss.Scene("cornell")
    s.add_obj(write(tmp_path, "ico.obj", icosphere_obj(5)), transform=translate_scale(0.0, -2.0, -5.0, 1.5), material=2)
    return s


def axis_normal_scene():
    """Triangles whose vertex normals are the unit axes (the oracle's normal is then the weights), duplicated for exact ties."""
    s = COVERAGE_SCENES["bounded"]()
    for k in range(s.desc.numTriangles):
        t = s.desc.triangles[k]
        t.normal0.x, t.normal0.y, t.normal0.z = 1, 0, 0
        t.normal1.x, t.normal1.y, t.normal1.z = 0, 1, 0
        t.normal2.x, t.normal2.y, t.normal2.z = 0, 0, 1
    return s


SCENE_MAKERS = {
    "default": lambda tmp: ptss.Scene("default"),
    "lambert": lambda tmp: ptss.Scene("lambert"),
    "cornell": lambda tmp: ptss.Scene("cornell"),
    "mixed": lambda tmp: ptss.Scene("mixed"),
    "in_place_484": lambda tmp: COVERAGE_SCENES["plain_padded"](),
    "spheres_1000_dup": lambda tmp: duplicate_spheres(random_scene(7410, ns=1000, nt=6)[0], [(3, 700), (10, 11), (500, 999)]),
    "mesh": lambda tmp: ptss.Scene("mesh"),
    "icosphere_20k": icosphere_scene,
    "axis_normals": lambda tmp: axis_normal_scene(),
}
# scenes whose oracle loop is long: fewer rays
SMALL = {"spheres_1000_dup": 40, "icosphere_20k": 12}


def frame_lds(r):
    r.generate_frame()
    lds = {k[3] for k in r.launched_kernels() if k[0] == "bounce"}
    assert len(lds) == 1
    return lds.pop()


@pytest.mark.parametrize("every_sphere_loop", [False, True])
@pytest.mark.parametrize("name", list(SCENE_MAKERS))
def test_queries_match_the_reference_loop(name, every_sphere_loop, tmp_path):
    scene = SCENE_MAKERS[name](tmp_path)
    desc = scene.desc
    r = ptss.Renderer(scene, 24, 16, max_iterations=2, every_sphere_loop=every_sphere_loop)
    lds = frame_lds(r)
    if name == "in_place_484":
        assert not lds
    if name in ("mesh", "icosphere_20k"):   # cfg.everySphereLoop also walks every triangle (no mesh image)
        assert (r.triangle_leaves() > 0) != every_sphere_loop
    n = SMALL.get(name)
    rays = query_rays(desc, seed=len(name) * 7 + every_sphere_loop, n_random=96 if n is None else n, cam_size=(12, 8) if n is None else (4, 3))
    if n is not None:
        rays = rays[:n * 3]
    hits = r.intersect(rays)
    occ = r.occluded(rays)
    assert r.launched_kernels() - ptss.all_kernels() - ptss.mesh_kernels() == {("query", "closest", lds), ("query", "any", lds)}
    check_hits(desc, rays, hits, occ, axis_normals=(name == "axis_normals"))
    more = with_tmax_at_hits(desc, rays, hits, 24 if n is None else 3)
    if len(more):
        check_hits(desc, more, r.intersect(more), r.occluded(more), axis_normals=(name == "axis_normals"))
    r.close()


def test_exact_ties_on_duplicate_primitives_end_on_the_highest_index():
    s = duplicate_spheres(random_scene(7411, ns=60, nt=0)[0], [(5, 40), (5, 41)])
    sp = s.desc.spheres[5]
    c = np.array([sp.position.x, sp.position.y, sp.position.z], np.float32)
    o = c + np.float32(20)
    rays = ptss.make_rays(np.repeat(o[None], 8, 0), np.repeat((c - o)[None] / np.linalg.norm(c - o), 8, 0))
    for every in (False, True):
        r = ptss.Renderer(s, 16, 16, max_iterations=1, every_sphere_loop=every)
        hits = r.intersect(rays)
        check_hits(s.desc, rays, hits, r.occluded(rays))
        r.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(n):
    scene = ptss.Scene("mixed")
    r = ptss.Renderer(scene, 16, 16, max_iterations=1)
    rays = query_rays(scene.desc, seed=n)[:n]
    hits, occ = r.intersect(rays), r.occluded(rays)
    assert hits.shape == (n,) and occ.shape == (n,)
    check_hits(scene.desc, rays, hits, occ)
    r.close()


@pytest.mark.parametrize("name", ["mixed", "spheres_1000_dup", "mesh"])
def test_a_million_rays_equal_the_every_sphere_loop_context(name, tmp_path):
    scene = SCENE_MAKERS[name](tmp_path)
    rng = np.random.default_rng(11)
    lo, hi = scene_box(scene.desc)
    n = 1 << 20
    rays = ptss.make_rays(rng.uniform(lo - 1, hi + 1, size=(n, 3)), unit(rng, n))
    a = ptss.Renderer(scene, 16, 16, max_iterations=1)
    b = ptss.Renderer(scene, 16, 16, max_iterations=1, every_sphere_loop=True)
    ha, hb = a.intersect(rays), b.intersect(rays)
    assert ha.tobytes() == hb.tobytes()
    assert np.array_equal(a.occluded(rays), b.occluded(rays))
    # a sample of them against the oracle loop
    pick = rng.choice(n, 48, replace=False)
    check_hits(scene.desc, rays[pick], ha[pick], a.occluded(rays[pick]))
    a.close()
    b.close()


def test_torch_tensors_on_the_current_stream_equal_the_numpy_path():
    torch = pytest.importorskip("torch")
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, 16, 16, max_iterations=1)
    rays = query_rays(scene.desc, seed=3)
    want_h, want_o = r.intersect(rays), r.occluded(rays)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(rays).to("cuda", non_blocking=False)
        th, to = r.intersect(t), r.occluded(t)
        got_h = th.cpu().numpy()
        got_o = to.cpu().numpy()
    assert th.shape == (len(rays), 12) and th.dtype == torch.float32
    assert got_h.tobytes() == want_h.tobytes()   # the same device: the same bits, NaN payloads included
    assert np.array_equal(got_o.astype(np.uint32), want_o)
    r.close()


@pytest.mark.parametrize("name,lanes", [("cornell", 0), ("mixed", 2), ("mesh", 2)])
def test_frames_are_untouched_by_queries(name, lanes):
    """Queries between frames and on a second stream while frames run, camera moves, two free-running frame lanes: the frames
    still equal the oracle's, and no guard wait expired."""
    torch = pytest.importorskip("torch")
    scene = ptss.Scene(name)
    w, h, bounces = 40, 24, 4
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, frame_lanes=lanes, lanes_free_run=lanes > 1)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces)
    rays = query_rays(scene.desc, seed=9)
    want = r.intersect(rays)
    side = torch.cuda.Stream()
    t = torch.from_numpy(rays).cuda()
    torch.cuda.synchronize()
    cam = ptss.default_camera()
    for tick, key in enumerate(["", "", "w", "", "f", ""]):
        if key:
            ptss.move_camera(cam, key)
            r.set_camera(cam)
            o.set_camera(cam)
        with torch.cuda.stream(side):
            side_hits = r.intersect(t)
        r.generate_frame()
        o.generate_frame()
        assert np.array_equal(r.live_counts(), o.live_counts()), (name, tick)
        assert r.intersect(rays).tobytes() == want.tobytes()
        side.synchronize()
        assert side_hits.cpu().numpy().tobytes() == want.tobytes()
    compare(r, o, (name, "frames with queries"), w, h, 1)
    r.close()
    o.close()


@pytest.mark.parametrize("preset", ["cornell", "mesh"])
def test_main_pick_prints_the_reference_loops_primitive(preset):
    w, h = 64, 48
    picks = [(32, 24), (5, 40), (60, 3), (20, 30)]
    args = [MAIN, "--preset", preset, "--size", f"{w}x{h}", "--ticks", "1", "--quiet"]
    for x, y in picks:
        args += ["--pick", f"{x},{y}"]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("pick ")]
    assert len(lines) == len(picks)
    scene = ptss.Scene(preset)
    cam = ptss.default_camera()
    for (x, y), line in zip(picks, lines):
        kind, prim, mat, dist, _, _ = oracle_closest(scene.desc, ptss.camera_ray(cam, w, h, x, y))
        f = line.split()
        assert f[1] == f"{x},{y}:" and f[2] == ("miss", "sphere", "triangle")[kind], line
        assert int(f[3]) == prim and int(f[5]) == mat, line
        assert np.float32(float(f[7])) == dist, line
