"""tools/mesh_bench.py [passes=6] [reps=5] [out.json] — Mrays/s of the mesh image against the every-triangle loop
(cfg.everySphereLoop = 1) on the "cornell" preset with a procedural icosphere of about 4k (level 4, 5,120 triangles), 16k
(level 5, 20,480) and 64k (three level-5 spheres, 61,440) triangles, at 640 x 360, 8 bounces, one sample per pass. The two
images alternate within one process, `reps` timed runs of `passes` passes each; the median and the spread (min, max) per image
go to stdout and to out.json."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402
from meshgen import icosphere_obj, translate_scale  # noqa: E402

W, H, BOUNCES = 640, 360, 8
passes = int(sys.argv[1]) if len(sys.argv) > 1 else 6
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
torch.cuda.init()

SCENES = {
    "4k": [(4, (0.3, -2.2, -5.0, 1.6), 0)],
    "16k": [(5, (0.3, -2.2, -5.0, 1.6), 0)],
    "64k": [(5, (-2.2, -2.6, -5.5, 1.1), 1), (5, (0.0, -2.6, -5.5, 1.1), 0), (5, (2.2, -2.6, -5.5, 1.1), 4)],
}


def scene_of(models, tmp):
    s = ptss.Scene("cornell")
    for k, (level, place, mat) in enumerate(models):
        path = os.path.join(tmp, f"m{k}.obj")
        with open(path, "w") as f:
            f.write(icosphere_obj(level))
        s.add_obj(path, transform=translate_scale(*place), material=mat)
    return s


def timed(r):
    r0 = r.total_ray_bounces()
    t0 = time.perf_counter()
    for _ in range(passes):
        r.generate_frame()
    r.synchronize()
    return (r.total_ray_bounces() - r0) / (time.perf_counter() - t0) / 1e6


results = {"frame": [W, H], "bounces": BOUNCES, "passes": passes, "reps": reps, "scenes": {}}
with tempfile.TemporaryDirectory() as tmp:
    for name, models in SCENES.items():
        s = scene_of(models, tmp)
        rs = {every: ptss.Renderer(s, W, H, max_iterations=BOUNCES, sync_each_frame=False, every_sphere_loop=every) for every in (False, True)}
        for r in rs.values():
            r.generate_frame()   # warm-up
            r.synchronize()
        runs = {False: [], True: []}
        for _ in range(reps):
            for every in (False, True):   # alternating within the call
                runs[every].append(timed(rs[every]))
        row = {}
        for every, label in ((False, "mesh"), (True, "every_triangle")):
            v = runs[every]
            row[label] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
        row["triangles"] = s.desc.numTriangles
        row["leaves"] = rs[False].triangle_leaves()
        row["speedup"] = row["mesh"]["median"] / row["every_triangle"]["median"]
        results["scenes"][name] = row
        print(f"{name}: {row['triangles']} triangles, {row['leaves']} leaves: mesh {row['mesh']['median']:.1f} Mrays/s "
              f"[{row['mesh']['min']:.1f}, {row['mesh']['max']:.1f}], every triangle {row['every_triangle']['median']:.2f} "
              f"[{row['every_triangle']['min']:.2f}, {row['every_triangle']['max']:.2f}]: x{row['speedup']:.1f}", flush=True)
        for r in rs.values():
            r.close()
if out_path:
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1)
