"""tools/motion_bench.py [runs=5] [calls=50] [out.json] — what the motion rows cost, on one GPU.

1920x1080, the "mesh" and "mixed" presets: four frames at pose A become the history; every triangle vertex is displaced by a smooth
field of 0.05 (ptss_update_triangles where the image takes it: mesh; mixed stores its 16 triangles by edge class, so there only the
"previous pose" handed to the motion call differs) and the camera moves ('w', 'd', 'f'); one frame is rendered. Timed in the same
process, HIP events around `calls` back-to-back calls on the context's stream after a warm-up of the same shape, `runs` times,
milliseconds per call, median [min, max]:
  ptss_render_features  against  ptss_render_features_motion with the whole table as previous pose, and with count = 0;
  ptss_reproject        against  ptss_reproject_motion on the rows of the whole-table call.
The expectation to confirm or refute: the extra cost is the 16 B written per pixel plus the 36 B gathered per pixel on a moved
triangle — far below a second trace. Written to stdout and out.json."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402
from ptss_types import Triangle  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080


def timed(fn):
    for _ in range(3):
        fn()   # warm-up of this shape
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    ms.sort()
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def nudged(t, amount):
    out = t.copy()
    for name in ("vertex0", "vertex1", "vertex2"):
        p = t[name].astype(np.float64)
        field = np.stack([np.sin(2.0 * p[:, 1] + 0.3), 0.5 * np.sin(3.0 * p[:, 0]), 0.3 * np.sin(p[:, 0] + p[:, 2])], axis=1)
        out[name] = (p + amount * field).astype(np.float32)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("motion_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    L = ptss.device_lib()
    H_ = ptss._hip_lib()
    results = {}
    for name, updatable in (("mesh", True), ("mixed", False)):
        scene = ptss.Scene(name)
        T = scene.desc.numTriangles
        pose_a = np.frombuffer(C.string_at(scene.desc.triangles, T * C.sizeof(Triangle)), dtype=ptss.TRIANGLE_DTYPE).copy()
        r = ptss.Renderer(scene, W, H, sync_each_frame=False)
        cam_a = ptss.default_camera()
        for _ in range(4):
            r.generate_frame()
        r.synchronize()
        n = r.local_pixels
        d_fa, d_ha, d_hb = (r._device_buffer(k, n * size) for k, size in (("features_a", 32), ("history_a", 16), ("history_b", 16)))
        d_fb, d_mb = r.features_devptr(), r.motion_devptr()
        d_prev = r._device_buffer("prev_pose", pose_a.nbytes)
        p = ptss.default_reproject_params()
        ptss._check(L.ptss_render_features(r._ctx, d_fa, None))
        ptss._check(L.ptss_reproject(r._ctx, d_fa, None, None, None, C.byref(p), d_ha, None))
        if updatable:
            r.update_triangles(nudged(pose_a, 0.05))
            prev = pose_a
        else:
            prev = nudged(pose_a, 0.05)
        ptss._hip_check(H_.hipMemcpy(d_prev, prev.ctypes.data, prev.nbytes, 1), "hipMemcpy")
        cam_b = ptss.default_camera()
        for k in "wdf":
            ptss.move_camera(cam_b, k)
        r.set_camera(cam_b)
        r.generate_frame()
        r.synchronize()
        res = {"features_ms": timed(lambda: ptss._check(L.ptss_render_features(r._ctx, d_fb, None))),
               "features_motion_static_ms": timed(lambda: ptss._check(L.ptss_render_features_motion(r._ctx, None, 0, 0, d_fb, d_mb, None))),
               "features_motion_ms": timed(lambda: ptss._check(L.ptss_render_features_motion(r._ctx, d_prev, 0, T, d_fb, d_mb, None)))}
        res["reproject_ms"] = timed(lambda: ptss._check(L.ptss_reproject(r._ctx, d_fb, C.byref(cam_a), d_fa, d_ha, C.byref(p), d_hb, None)))
        res["reproject_motion_ms"] = timed(
            lambda: ptss._check(L.ptss_reproject_motion(r._ctx, d_fb, d_mb, C.byref(cam_a), d_fa, d_ha, C.byref(p), d_hb, None)))
        torch.cuda.synchronize()
        motion = np.empty(n, dtype=ptss.MOTION_DTYPE)
        ptss._hip_check(H_.hipMemcpy(motion.ctypes.data, d_mb, motion.nbytes, 2), "hipMemcpy")
        on_triangle = float((motion["surface"] >= 0x40000000).mean())
        res["pixels_on_moved_triangles"] = on_triangle
        res["pixels_with_history"] = float((r.read_history(d_hb)["weight"] > 1).mean())
        res["extra_bytes"] = int(n * 16 + on_triangle * n * 36)
        results[f"{name}/{W}x{H}"] = res
        f, s, m, a, b = (res[k] for k in ("features_ms", "features_motion_static_ms", "features_motion_ms", "reproject_ms", "reproject_motion_ms"))
        print(f"{name}/{W}x{H}: features {f['median']:.3f} ms [{f['min']:.3f}, {f['max']:.3f}]  with motion rows, count = 0 {s['median']:.3f} ms "
              f"[{s['min']:.3f}, {s['max']:.3f}]  with motion rows, whole table {m['median']:.3f} ms [{m['min']:.3f}, {m['max']:.3f}] "
              f"({100 * on_triangle:.1f} % of the pixels on a moved triangle, {res['extra_bytes'] / 1e6:.1f} MB more)  reproject {a['median']:.3f} ms "
              f"[{a['min']:.3f}, {a['max']:.3f}]  reproject_motion {b['median']:.3f} ms [{b['min']:.3f}, {b['max']:.3f}] "
              f"({100 * res['pixels_with_history']:.1f} % of the pixels with history)", flush=True)
        r.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
