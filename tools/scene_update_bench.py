#!/usr/bin/env python3
"""tools/scene_update_bench.py [--out profiles/update/scene_update_bench.json] — what moving a model costs on one MI355X
(DESIGN.md §3.18), at 1920x1080, one sample per tick:

  * per mesh size (5,120 / 81,920 / 1,046,528 triangles — the last just under the mesh image's limit of 2^20 once the box's 14
    are added —, a wavy grid inside the Cornell box): the time of ptss_update_triangles (both kernels; the records already on
    the device), of ptss_set_scene and of ptss_destroy + ptss_create — host clock around the call and a synchronise, median of
    the repeats after a warm-up;
  * for the 5,120-triangle mesh turned by 30 and by 90 degrees: Mrays/s of the frames after a refit against the frames after
    ptss_set_scene of the same pose — the price of the kd order staying the packed pose's.
Prints one JSON document."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ptss  # noqa: E402
from scene_update_common import TableScene, preset_triangles, triangles_of  # noqa: E402

W, H, BOUNCES = 1920, 1080, 8


def wavy_grid(nu, nv, turn=0.0):
    """2 nu nv triangles: a height field over the box's floor, turned by `turn` radians about the vertical through its centre."""
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="xy")
    x, z = -3.0 + 6.0 * i / nu, -1.5 - 5.0 * j / nv
    y = -3.0 + 0.6 * np.sin(2.5 * x) * np.cos(2.0 * z)
    cx, cz = 0.0, -4.0
    c, s = np.cos(turn), np.sin(turn)
    p = np.stack([cx + c * (x - cx) + s * (z - cz), y, cz + c * (z - cz) - s * (x - cx)], axis=-1).astype(np.float32)
    p00, p10, p11, p01 = p[:-1, :-1], p[:-1, 1:], p[1:, 1:], p[1:, :-1]
    a = np.stack([p00, p00], axis=2).reshape(-1, 3)
    b = np.stack([p10, p11], axis=2).reshape(-1, 3)
    d = np.stack([p11, p01], axis=2).reshape(-1, 3)
    return triangles_of(a, b, d, 4)


def scene_of(nu, nv, turn=0.0):
    return TableScene(np.concatenate([preset_triangles(), wavy_grid(nu, nv, turn)]))


def median_ms(fn, repeats, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "repeats": repeats}


def mrays(r, frames=30):
    for _ in range(5):
        r.generate_frame()
    r.synchronize()
    n0, t = r.total_ray_bounces(), time.perf_counter()
    for _ in range(frames):
        r.generate_frame()
    n1 = r.total_ray_bounces()   # synchronises
    return (n1 - n0) / (time.perf_counter() - t) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L, Hip = ptss.device_lib(), None
    result = {"frame": [W, H], "bounces": BOUNCES, "sizes": [], "stale_order": []}
    for nu, nv in ((64, 40), (256, 160), (1024, 511)):   # + the box's 14: 5,134 / 81,934 / 1,046,542 (the mesh image ends at 2^20)
        scene = scene_of(nu, nv)
        moved = scene_of(nu, nv, turn=0.2)
        n = len(scene.triangles)
        holder = {"r": ptss.Renderer(scene, W, H, max_iterations=BOUNCES, sync_each_frame=False)}
        r = holder["r"]
        Hip = ptss._hip_lib()
        dev = C.c_void_p()
        ptss._hip_check(Hip.hipMalloc(C.byref(dev), moved.triangles.nbytes), "hipMalloc")
        ptss._hip_check(Hip.hipMemcpy(dev, moved.triangles.ctypes.data, moved.triangles.nbytes, 1), "hipMemcpy")

        def update():
            ptss._check(L.ptss_update_triangles(r._ctx, dev, 0, n, None))
            r.synchronize()

        def set_scene():
            r.set_scene(moved)
            r.synchronize()

        def recreate():
            holder["r"].close()
            holder["r"] = ptss.Renderer(moved, W, H, max_iterations=BOUNCES, sync_each_frame=False)
            holder["r"].synchronize()

        row = {"triangles": n, "leaves": r.triangle_leaves(), "update_triangles": median_ms(update, 20), "set_scene": median_ms(set_scene, 5, warm=1)}
        Hip.hipFree(dev)
        row["destroy_create"] = median_ms(recreate, 3, warm=1)
        holder["r"].close()
        result["sizes"].append(row)
    base = scene_of(64, 40)
    for degrees in (30, 90):
        pose = scene_of(64, 40, turn=np.radians(degrees))
        r = ptss.Renderer(base, W, H, max_iterations=BOUNCES, sync_each_frame=False)
        r.update_triangles(pose.triangles)
        refit = mrays(r)
        r.set_scene(pose)
        repacked = mrays(r)
        r.update_triangles(pose.triangles)   # (a refit of the packed pose: the order is now the pose's own)
        again = mrays(r)
        r.close()
        result["stale_order"].append({"degrees": degrees, "mrays_after_refit": refit, "mrays_after_set_scene": repacked,
                                      "mrays_after_refit_of_the_packed_pose": again})
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
