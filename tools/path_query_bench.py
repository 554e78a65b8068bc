"""tools/path_query_bench.py [runs=5] [calls=5] [out.json] — what radiance along caller-supplied rays costs against the frame loop
(ptss_trace_paths) on one GPU.

1920x1080, the "mixed" and "mesh" presets, maxIterations = the context's. The rays are the frame's own eye rays: ptss_camera_ray of
every pixel with the two jitter draws of the pixel's stream (the streams ptss_seed_path_rng makes, drawn here with numpy), the states
those streams two draws later — what a frame of the context traces. Per figure: HIP events around `calls` back-to-back calls on the
context's stream, after a warm-up of the same shape, `runs` times; milliseconds per call, median [min, max]. In one process:
  frame      one S = 1 ptss_generate_frame of the same context (the frame loop: compaction between bounces, shadow segments regrouped
             through the wave queue), the streams carrying on from call to call;
  paths      ptss_trace_paths over those rays in pixel order, the states carrying on from call to call likewise;
  shuffled   the same rays and states in a random order: the cost of an incoherent caller.
No ratio is fixed in advance: the path kernel has no compaction (a wave runs until its longest path ends) and tests one shadow segment
per lane per light. Also reported: the iterations entered per ray (from the results) beside the frame's (from its live counts), and
the mean over waves of the longest path in a wave, which is what a wave pays. Written to stdout and out.json."""
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

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080
SCENES = ["mixed", "mesh"]
SEED = 0x5EED


def draw(states):
    """One draw of every XORWOW stream of an (n, 6) uint32 array, in place (csrc/xorwow.h next + uniform) -> (n,) float32."""
    v = states
    t = v[:, 0] ^ (v[:, 0] >> np.uint32(2))
    v4 = v[:, 4].copy()
    v[:, 0:4] = v[:, 1:5].copy()
    v[:, 4] = (v4 ^ (v4 << np.uint32(4))) ^ (t ^ (t << np.uint32(1)))
    v[:, 5] += np.uint32(362437)
    x = v[:, 4] + v[:, 5]
    return x.astype(np.float32) * np.float32(2.3283064365386963e-10) + np.float32(1.1641532182693481e-10)


def eye_rays(cam, states):
    """ptss_camera_ray of every pixel with the first two draws of its stream: (W * H, 8) float32 in pixel order."""
    s = states.copy()
    jx, jy = draw(s), draw(s)
    out = np.empty((W * H, 8), dtype=np.float32)
    q = ptss.RayQuery()
    buf = (C.c_float * 8).from_buffer(q)
    fn, ref_cam, ref_q = ptss.host_lib().ptss_camera_ray, C.byref(cam), C.byref(q)
    for y in range(H):
        for x in range(W):
            p = y * W + x
            if fn(ref_cam, W, H, x, y, C.c_float(jx[p]), C.c_float(jy[p]), ref_q) != 0:
                raise SystemExit("ptss_camera_ray failed")
            out[p] = buf
    return out


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("path_query_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    n = W * H
    results, rays = {}, None
    for name in SCENES:
        r = ptss.Renderer(ptss.Scene(name), W, H, seed=SEED, sync_each_frame=False)
        iterations = int(r.cfg.maxIterations)
        if rays is None:   # the default camera and the seed are the same for every scene
            rays = eye_rays(ptss.default_camera(), ptss_words(r.seed_path_rng(n, SEED)))
        d_rays = torch.from_numpy(rays).cuda()
        d_rng = r.seed_path_rng(n, SEED, 0, skip=2, device=True)
        perm = torch.randperm(n, device=d_rays.device, generator=torch.Generator(device=d_rays.device).manual_seed(1))
        s_rays, s_rng = d_rays[perm].contiguous(), d_rng[perm].contiguous()

        frame = timed(lambda: r.generate_frame())
        live = r.live_counts()
        paths = timed(lambda: r.trace_paths(d_rays, d_rng, iterations))
        bounces = r.trace_paths(d_rays, d_rng, iterations)[:, 3].contiguous().view(torch.int32).cpu().numpy()
        shuffled = timed(lambda: r.trace_paths(s_rays, s_rng, iterations))
        s_bounces = r.trace_paths(s_rays, s_rng, iterations)[:, 3].contiguous().view(torch.int32).cpu().numpy()
        wave_max = lambda b: float(b[:len(b) // 64 * 64].reshape(-1, 64).max(axis=1).mean())
        in_place, lds = r.path_launches()
        res = {"maxIterations": iterations, "rays": n, "scene_image": "in LDS" if lds else "in place", "frame_ms": frame, "paths_ms": paths,
               "shuffled_ms": shuffled, "paths_over_frame": paths["median"] / frame["median"],
               "shuffled_over_paths": shuffled["median"] / paths["median"], "shuffled_over_frame": shuffled["median"] / frame["median"],
               "frame_iterations_per_ray": float(np.asarray(live, dtype=np.float64).sum() / n), "frame_live_counts": [int(v) for v in live],
               "paths_iterations_per_ray": float(bounces.mean()), "paths_mean_of_wave_max_iterations": wave_max(bounces),
               "shuffled_mean_of_wave_max_iterations": wave_max(s_bounces),
               "paths_Mrays_per_s": n / paths["median"] / 1e3, "frame_Mrays_per_s": n / frame["median"] / 1e3}
        results[f"{name}/{W}x{H}"] = res
        print(f"{name}/{W}x{H}, {iterations} iterations, scene {res['scene_image']}: frame {frame['median']:.3f} ms [{frame['min']:.3f}, "
              f"{frame['max']:.3f}]; paths {paths['median']:.3f} ms [{paths['min']:.3f}, {paths['max']:.3f}] = {res['paths_over_frame']:.2f} x frame; "
              f"shuffled {shuffled['median']:.3f} ms [{shuffled['min']:.3f}, {shuffled['max']:.3f}] = {res['shuffled_over_paths']:.2f} x paths; "
              f"iterations per ray: frame {res['frame_iterations_per_ray']:.2f}, paths {res['paths_iterations_per_ray']:.2f}, longest in a wave "
              f"{res['paths_mean_of_wave_max_iterations']:.2f} (shuffled {res['shuffled_mean_of_wave_max_iterations']:.2f})", flush=True)
        r.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


def ptss_words(states):
    return np.ascontiguousarray(states).view(np.uint32).reshape(len(states), 6).copy()


if __name__ == "__main__":
    main()
