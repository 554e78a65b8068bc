"""tools/query_bench.py [reps=5] [out.json] — rays/s of the batched ray queries (ptss_intersect / ptss_occluded).

2^22 rays of two kinds per scene: "camera" = the eye rays of a 1920 x 1080 frame, two jittered rays per pixel (coherent), and
"surface" = rays leaving random points on random primitives in random unit directions (incoherent). Scenes: the "mixed" (c3),
"stress" (c5, 1,024 spheres) and "mesh" presets and the "cornell" preset with a level-5 icosphere (20,480 triangles). The same
rays run on a context of the scene's own image and on one with cfg.everySphereLoop = 1 (every primitive, caller's order). Each
figure: HIP events around one call on the current stream, one warm-up, `reps` timed calls, median [min, max] in Mrays/s, to
stdout and out.json. (Camera rays are built here with numpy in the same arithmetic order as ptss_camera_ray; they feed a
measurement only.)"""
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402
from meshgen import icosphere_obj, translate_scale  # noqa: E402

N = 1 << 22
W, H = 1920, 1080
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_path = sys.argv[2] if len(sys.argv) > 2 else None
torch.cuda.init()


def camera_rays(cam, w, h, jitters):
    """ptss_camera_ray's operations, vectorised (float32 throughout)."""
    f = np.float32
    s = f(-2) * f(np.tan(f(cam.fieldOfView) * f(0.5)))
    aspect, inv_w, inv_h = f(h) / f(w), f(1) / f(w), f(1) / f(h)
    q = np.array([cam.rotation.x, cam.rotation.y, cam.rotation.z, cam.rotation.w], np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    out = []
    for jx, jy in jitters:
        sx = ((xs.astype(f) + f(jx)) * inv_w - f(0.5)) * s
        sy = ((ys.astype(f) + f(jy)) * inv_h - f(0.5)) * s * aspect
        v = np.stack([sx, sy, np.ones_like(sx)], -1).reshape(-1, 3) * f(cam.zNear)
        u = q[:3]
        t = f(2) * np.cross(u, v)
        d = v + q[3] * t + np.cross(u, t)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(ptss.make_rays(np.broadcast_to([cam.position.x, cam.position.y, cam.position.z], d.shape), d))
    return np.concatenate(out)[:N]


def surface_rays(desc, rng):
    sph = [(np.array([s.position.x, s.position.y, s.position.z]), s.radius) for s in (desc.spheres[k] for k in range(desc.numSpheres))]
    tri = [np.array([[v.x, v.y, v.z] for v in (t.vertex0, t.vertex1, t.vertex2)]) for t in (desc.triangles[k] for k in range(desc.numTriangles))]
    ns, nt = len(sph), len(tri)
    which = rng.integers(0, ns + nt, N)
    pts = np.empty((N, 3))
    d = rng.normal(size=(N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if ns:
        c = np.array([p for p, _ in sph]), np.array([r for _, r in sph])
        m = which < ns
        u = rng.normal(size=(m.sum(), 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        pts[m] = c[0][which[m]] + c[1][which[m], None] * u
    if nt:
        T = np.array(tri)
        m = which >= ns
        a, b = rng.random(m.sum()), rng.random(m.sum())
        flip = a + b > 1
        a[flip], b[flip] = 1 - a[flip], 1 - b[flip]
        t = T[which[m] - ns]
        pts[m] = t[:, 0] + a[:, None] * (t[:, 1] - t[:, 0]) + b[:, None] * (t[:, 2] - t[:, 0])
    return ptss.make_rays(pts, d)


def icosphere_scene(tmp):
    s = ptss.Scene("cornell")
    path = os.path.join(tmp, "ico.obj")
    with open(path, "w") as f:
        f.write(icosphere_obj(5))
    s.add_obj(path, transform=translate_scale(0.3, -2.2, -5.0, 1.6), material=2)
    return s


def time_call(fn, t):
    fn(t)   # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(t)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    mrays = sorted(N / (m * 1e3) for m in ms)
    return {"median": statistics.median(mrays), "min": mrays[0], "max": mrays[-1]}


def main():
    rng = np.random.default_rng(1)
    results = {}
    with tempfile.TemporaryDirectory() as tmp:
        scenes = {"mixed": ptss.Scene("mixed"), "stress": ptss.Scene("stress"), "mesh": ptss.Scene("mesh"), "icosphere_20k": icosphere_scene(tmp)}
        cam = ptss.default_camera()
        cam_rays = torch.from_numpy(camera_rays(cam, W, H, [(0.25, 0.25), (0.75, 0.75)])).cuda()
        for name, scene in scenes.items():
            kinds = {"camera": cam_rays, "surface": torch.from_numpy(surface_rays(scene.desc, rng)).cuda()}
            for every in (False, True):
                r = ptss.Renderer(scene, 64, 64, max_iterations=1, every_sphere_loop=every)
                image = "every-primitive" if every else "scene image"
                for kind, t in kinds.items():
                    for q, fn in (("closest", r.intersect), ("occluded", r.occluded)):
                        res = time_call(fn, t)
                        results[f"{name}/{image}/{kind}/{q}"] = res
                        print(f"{name:14s} {image:16s} {kind:8s} {q:9s} {res['median']:9.1f} Mrays/s [{res['min']:.1f}, {res['max']:.1f}]",
                              flush=True)
                r.close()
    out = {"rays": N, "reps": reps, "unit": "Mrays/s", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
