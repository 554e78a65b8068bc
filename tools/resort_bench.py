#!/usr/bin/env python3
"""tools/resort_bench.py [--out profiles/resort/resort_bench.json] [--frame 480x270] [--stale-sizes 0,1] — what re-sorting a live
mesh on the device costs and buys on one MI355X. The meshes are tools/scene_update_bench.py's wavy grids inside
the Cornell box (5,134 / 81,934 / 1,046,542 triangles); the pose scatters every leaf: each triangle of the grid takes the place of
a pseudo-random other one.

  (a) per size: the time of ptss_resort_triangles (the sort, the permutation and the refit) against ptss_set_scene of the same pose
      IN THE SAME PROCESS — the only other way to get the order rebuilt — and, for scale, ptss_update_triangles: host clock around
      the call and a synchronise, a warm-up, then median, min and max of the repeats;
  (b) per size of --stale-sizes: Mrays/s over 30 frames of the scattered pose after the refit alone (the order of the packed pose),
      after the re-sort, and after ptss_set_scene — the price of a stale order, which §3.18 left unmeasured;
  (c) at the largest size, once: ptss_read_triangle_positions after the re-sort equals ptss_probe_kd_order of the pose.
Prints one JSON document and a table."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ptss  # noqa: E402
from resort_common import scatter  # noqa: E402
from scene_update_bench import scene_of  # noqa: E402

BOUNCES = 8
GRIDS = ((64, 40), (256, 160), (1024, 511))   # + the box's 14 triangles
BOX = range(14)


def timed(fn, repeats, warm, before=None):
    """before: run ahead of every call, outside the clock."""
    for _ in range(warm):
        if before:
            before()
        fn()
    out = []
    for _ in range(repeats):
        if before:
            before()
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "repeats": repeats, "warm_up": warm}


def mrays(r, frames=30, warm=2):
    for _ in range(warm):
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
    ap.add_argument("--frame", default="480x270")
    ap.add_argument("--sizes", default="0,1,2", help="indices into the three grids for (a)")
    ap.add_argument("--stale-sizes", default="0,1", help="indices into the three grids for (b)")
    args = ap.parse_args()
    W, H = (int(v) for v in args.frame.split("x"))
    sizes = [int(v) for v in args.sizes.split(",") if v != ""]
    stale = [int(v) for v in args.stale_sizes.split(",") if v != ""]
    L, Hip = ptss.device_lib(), ptss._hip_lib()
    result = {"frame": [W, H], "bounces": BOUNCES, "sizes": [], "stale_order": [], "positions_equal_probe": None}
    for k in sorted(set(sizes) | set(stale)):
        scene = scene_of(*GRIDS[k])
        pose = scatter(scene.triangles, keep=BOX)
        moved = scene.with_triangles(pose)
        n = len(pose)
        print(f"{n} triangles ...", file=sys.stderr, flush=True)
        r = ptss.Renderer(scene, W, H, max_iterations=BOUNCES, sync_each_frame=False)
        try:
            if k in stale:
                r.update_triangles(pose)
                refit_only = mrays(r)
                print(f"  refit only: {refit_only:.1f} Mrays/s", file=sys.stderr, flush=True)
                r.resort_triangles()
                resorted = mrays(r)
                r.set_scene(moved)
                repacked = mrays(r)
                result["stale_order"].append({"triangles": n, "frames": 30, "mrays_after_refit_only": refit_only,
                                              "mrays_after_resort": resorted, "mrays_after_set_scene": repacked})
                r.set_scene(scene)
            if k in sizes:
                dev, dev0 = C.c_void_p(), C.c_void_p()
                for d, table in ((dev, pose), (dev0, scene.triangles)):
                    ptss._hip_check(Hip.hipMalloc(C.byref(d), table.nbytes), "hipMalloc")
                    ptss._hip_check(Hip.hipMemcpy(d, table.ctypes.data, table.nbytes, 1), "hipMemcpy")
                turn = [0]

                def update():
                    ptss._check(L.ptss_update_triangles(r._ctx, dev, 0, n, None))
                    r.synchronize()

                def other_pose():   # the two poses in turn: every timed re-sort finds the order of the OTHER pose and moves every row
                    turn[0] ^= 1
                    ptss._check(L.ptss_update_triangles(r._ctx, dev0 if turn[0] else dev, 0, n, None))
                    r.synchronize()

                def resort():
                    ptss._check(L.ptss_resort_triangles(r._ctx, None))
                    r.synchronize()

                def set_scene():
                    r.set_scene(moved)
                    r.synchronize()

                update()
                t = time.perf_counter()
                resort()   # the first call: allocates the scratch and sorts the order of the packed pose into the scattered one's
                first_ms = (time.perf_counter() - t) * 1e3
                if k == max(sizes) and k == len(GRIDS) - 1:
                    result["positions_equal_probe"] = {"triangles": n, "equal": bool(np.array_equal(r.triangle_positions(n), ptss.probe_kd_order(pose)))}
                row = {"triangles": n, "leaves": r.triangle_leaves(), "resort_first_call_ms": first_ms,
                       "update_triangles": timed(update, 20, 2), "resort_triangles": timed(resort, 20, 2, before=other_pose),
                       "set_scene": timed(set_scene, 5, 1)}
                row["set_scene_over_resort"] = row["set_scene"]["median_ms"] / row["resort_triangles"]["median_ms"]
                Hip.hipFree(dev)
                Hip.hipFree(dev0)
                result["sizes"].append(row)
        finally:
            r.close()
    text = json.dumps(result, indent=1)
    print(text)
    lines = [f"frame {W}x{H}, {BOUNCES} bounces; ms: median [min, max] of the repeats after a warm-up, host clock around call + synchronise"]
    for row in result["sizes"]:
        f = lambda d: f"{d['median_ms']:.3f} [{d['min_ms']:.3f}, {d['max_ms']:.3f}] x{d['repeats']}"
        lines.append(f"{row['triangles']:>9,} triangles: resort {f(row['resort_triangles'])} (first call {row['resort_first_call_ms']:.3f}); "
                     f"set_scene {f(row['set_scene'])}; update {f(row['update_triangles'])}; set_scene / resort = {row['set_scene_over_resort']:.1f}")
    for row in result["stale_order"]:
        lines.append(f"{row['triangles']:>9,} triangles, scattered pose, Mrays/s over {row['frames']} frames: refit only {row['mrays_after_refit_only']:.1f}, "
                     f"re-sorted {row['mrays_after_resort']:.1f}, set_scene {row['mrays_after_set_scene']:.1f}")
    if result["positions_equal_probe"]:
        p = result["positions_equal_probe"]
        lines.append(f"{p['triangles']:>9,} triangles: ptss_read_triangle_positions == ptss_probe_kd_order: {p['equal']}")
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")
        open(os.path.splitext(args.out)[0] + ".txt", "w").write("\n".join(lines) + "\n")
    if result["positions_equal_probe"] and not result["positions_equal_probe"]["equal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
