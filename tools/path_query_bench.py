"""tools/path_query_bench.py [runs=5] [calls=5] [out.json] [scenes=mixed,mesh] — what radiance along caller-supplied rays costs against
the frame loop (ptss_trace_paths) and what the refill schedule makes of it (ptss_trace_paths_opt with
PTSS_PATHS_REFILL) on one GPU.

1920x1080, the "mixed" and "mesh" presets, maxIterations = the context's. The rays are the frame's own eye rays — ptss_generate_rays of
a pinhole film of the frame's size over the streams ptss_seed_path_rng makes, which is ptss_camera_ray of every pixel with the two
jitter draws of the pixel's stream, bit for bit (tests/test_gpu_film.py) — and the states those streams two draws later: what a frame
of the context traces. Per figure: HIP events around `calls` back-to-back calls on the context's stream, after a warm-up of the same
shape, `runs` times; milliseconds per call, median [min, max]. In one process:
  frame             one S = 1 ptss_generate_frame of the same context (the frame loop: compaction between bounces, shadow segments
                    regrouped through the wave queue), the streams carrying on from call to call;
  paths             ptss_trace_paths over those rays in pixel order, the states carrying on from call to call likewise;
  refill            the same with PTSS_PATHS_REFILL, maxWorkgroups 0, on states of its own that carry on likewise;
  shuffled, shuffled_refill   the same rays and states in a random order: the cost of an incoherent caller.
The plain and the refill leg of a pair are interleaved: run k of the one, then run k of the other. No ratio is fixed in advance. Also
reported: the iterations entered per ray (from the results) beside the frame's (from its live counts); the mean over waves of the
longest path in a wave, which is what a wave of the plain schedule pays; the lane occupancy = lane iterations / (64 x wave iterations),
of the refill schedule from ptss_path_refill_stats over one call and of the plain schedule from the `bounces` column of the same call
(whose bytes the refill call's are compared with); the dequeues of that call. The chunk size is the library's (PTSS_REFILL_CHUNK of
csrc/ptss_paths.hip): run the tool once per variant library (tools/build_variants.py rc64=PTSS_REFILL_CHUNK=64, PTSS_LIBNAME=...) to
compare chunk sizes; the library's name is recorded. Written to stdout and out.json."""
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
SCENES = sys.argv[4].split(",") if len(sys.argv) > 4 else ["mixed", "mesh"]
W, H = 1920, 1080
SEED = 0x5EED


def one_run(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def timed(*fns):
    """Each of `fns` warmed up, then `runs` runs of each, interleaved run by run -> one summary per function."""
    for fn in fns:
        for _ in range(3):
            fn()   # warm-up of this shape
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            ms[k].append(one_run(fn))
    out = [summary(m) for m in ms]
    return out[0] if len(fns) == 1 else out


def occupancies(r, d_rays, d_rng, iterations):
    """One plain and one refill call on copies of the same states -> (bounces, plain occupancy, refill occupancy, wave iterations of
    the plain schedule, of the refill call, its dequeues). The two calls' bytes must agree."""
    a, b = d_rng.clone(), d_rng.clone()
    plain = r.trace_paths(d_rays, a, iterations)
    before = r.path_refill_stats()
    refill = r.trace_paths(d_rays, b, iterations, schedule="refill")
    after = r.path_refill_stats()
    if not (torch.equal(plain.view(torch.int32), refill.view(torch.int32)) and torch.equal(a, b)):
        raise SystemExit("path_query_bench: the refill call's bytes differ from ptss_trace_paths'")
    bounces = plain[:, 3].contiguous().view(torch.int32).cpu().numpy().astype(np.int64)
    padded = np.concatenate([bounces, np.zeros((-len(bounces)) % 64, dtype=np.int64)]).reshape(-1, 64)
    plain_waves = int(padded.max(axis=1).sum())
    waves, lanes, dequeues = (after[k] - before[k] for k in (2, 3, 4))
    if lanes != int(bounces.sum()):
        raise SystemExit("path_query_bench: the lane iterations are not the sum of the bounces")
    return bounces, float(bounces.sum() / (64.0 * plain_waves)), float(lanes / (64.0 * waves)), plain_waves, int(waves), int(dequeues)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("path_query_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    n = W * H
    results = {}
    for name in SCENES:
        r = ptss.Renderer(ptss.Scene(name), W, H, seed=SEED, sync_each_frame=False)
        iterations = int(r.cfg.maxIterations)
        d_rng = r.seed_path_rng(n, SEED, 0, skip=0, device=True)
        d_rays = r.generate_rays(ptss.film_camera("pinhole", W, H, ptss.default_camera(), jitter=1), d_rng)   # d_rng: two draws later
        perm = torch.randperm(n, device=d_rays.device, generator=torch.Generator(device=d_rays.device).manual_seed(1))
        s_rays, s_rng = d_rays[perm].contiguous(), d_rng[perm].contiguous()
        bounces, occ_plain, occ_refill, waves_plain, waves_refill, dequeues = occupancies(r, d_rays, d_rng, iterations)
        s_bounces, s_occ_plain, s_occ_refill, s_waves_plain, s_waves_refill, s_dequeues = occupancies(r, s_rays, s_rng, iterations)
        r_rng, sr_rng = d_rng.clone(), s_rng.clone()   # the refill legs' own states

        frame = timed(lambda: r.generate_frame())
        live = r.live_counts()
        paths, refill = timed(lambda: r.trace_paths(d_rays, d_rng, iterations), lambda: r.trace_paths(d_rays, r_rng, iterations, schedule="refill"))
        shuffled, s_refill = timed(lambda: r.trace_paths(s_rays, s_rng, iterations),
                                   lambda: r.trace_paths(s_rays, sr_rng, iterations, schedule="refill"))
        wave_max = lambda b: float(b[:len(b) // 64 * 64].reshape(-1, 64).max(axis=1).mean())
        in_place, lds = r.path_launches()
        res = {"maxIterations": iterations, "rays": n, "scene_image": "in LDS" if lds else "in place", "frame_ms": frame, "paths_ms": paths,
               "shuffled_ms": shuffled, "paths_over_frame": paths["median"] / frame["median"],
               "shuffled_over_paths": shuffled["median"] / paths["median"], "shuffled_over_frame": shuffled["median"] / frame["median"],
               "frame_iterations_per_ray": float(np.asarray(live, dtype=np.float64).sum() / n), "frame_live_counts": [int(v) for v in live],
               "paths_iterations_per_ray": float(bounces.mean()), "paths_mean_of_wave_max_iterations": wave_max(bounces),
               "shuffled_mean_of_wave_max_iterations": wave_max(s_bounces),
               "paths_Mrays_per_s": n / paths["median"] / 1e3, "frame_Mrays_per_s": n / frame["median"] / 1e3,
               "refill_ms": refill, "shuffled_refill_ms": s_refill, "refill_over_paths": refill["median"] / paths["median"],
               "refill_over_frame": refill["median"] / frame["median"], "refill_wholly_below_paths": refill["max"] < paths["min"],
               "shuffled_refill_over_shuffled": s_refill["median"] / shuffled["median"],
               "shuffled_refill_over_frame": s_refill["median"] / frame["median"],
               "shuffled_refill_wholly_below_shuffled": s_refill["max"] < shuffled["min"],
               "lane_occupancy": {"paths": occ_plain, "refill": occ_refill, "shuffled": s_occ_plain, "shuffled_refill": s_occ_refill},
               "wave_iterations": {"paths": waves_plain, "refill": waves_refill, "shuffled": s_waves_plain, "shuffled_refill": s_waves_refill},
               "dequeues_per_call": {"refill": dequeues, "shuffled_refill": s_dequeues}, "refill_Mrays_per_s": n / refill["median"] / 1e3}
        results[f"{name}/{W}x{H}"] = res
        print(f"{name}/{W}x{H}, {iterations} iterations, scene {res['scene_image']}: frame {frame['median']:.3f} ms [{frame['min']:.3f}, "
              f"{frame['max']:.3f}]; paths {paths['median']:.3f} ms [{paths['min']:.3f}, {paths['max']:.3f}] = {res['paths_over_frame']:.2f} x frame; "
              f"shuffled {shuffled['median']:.3f} ms [{shuffled['min']:.3f}, {shuffled['max']:.3f}] = {res['shuffled_over_paths']:.2f} x paths; "
              f"iterations per ray: frame {res['frame_iterations_per_ray']:.2f}, paths {res['paths_iterations_per_ray']:.2f}, longest in a wave "
              f"{res['paths_mean_of_wave_max_iterations']:.2f} (shuffled {res['shuffled_mean_of_wave_max_iterations']:.2f})", flush=True)
        print(f"  refill {refill['median']:.3f} ms [{refill['min']:.3f}, {refill['max']:.3f}] = {res['refill_over_paths']:.2f} x paths = "
              f"{res['refill_over_frame']:.2f} x frame (wholly below paths: {res['refill_wholly_below_paths']}); shuffled refill "
              f"{s_refill['median']:.3f} ms [{s_refill['min']:.3f}, {s_refill['max']:.3f}] = {res['shuffled_refill_over_shuffled']:.2f} x shuffled; "
              f"lane occupancy paths {occ_plain:.3f}, refill {occ_refill:.3f}, shuffled {s_occ_plain:.3f}, shuffled refill {s_occ_refill:.3f}; "
              f"wave iterations {waves_plain} -> {waves_refill} ({waves_plain / waves_refill:.2f} x fewer); dequeues per call {dequeues}", flush=True)
        r.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(ptss.DEVICE_LIB), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
