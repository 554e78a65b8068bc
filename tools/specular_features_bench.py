"""tools/specular_features_bench.py [runs=5] [calls=50] [out.json] — time of ptss_render_features_specular on one GPU.

1920x1080, the "mixed", "default" and "mesh" presets. Per figure: HIP events around `calls` back-to-back calls on the context's
stream, after a warm-up of the same shape, `runs` times; milliseconds per call, median [min, max]. Measured in one process:
ptss_render_features (the first-hit kernel) and ptss_render_features_specular at maxSteps 1, 4 and 8, with dev_steps.

No ratio is fixed in advance. The yardstick of a chain kernel is one closest hit per link: the first-hit kernel's time multiplied by
(1 + mean steps per pixel), the mean taken from dev_steps of that very call. Reported per maxSteps: the mean steps, that product, the
measured time and the factor measured / product. A factor above 1 is what the chain costs beyond its closest hits: a wave runs
until its deepest lane has ended, with the finished lanes idle, so it pays max steps over its 64 pixels, not the mean (reported as
`wave_bound`: the first-hit time multiplied by 1 + the mean over waves of the largest step count among a wave's 64 consecutive
pixels — what the kernel would cost if only that mattered); secondary rays are less coherent than eye rays; and on the mesh preset a
wave with a direction outside the unit-length tolerance of the two-level traversal walks the triangles in the literal loop
(csrc/pthit.h meshQueryOk). Written to stdout and out.json."""
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
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080
SCENES = ["mixed", "default", "mesh"]
MAX_STEPS = [1, 4, 8]


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
        raise SystemExit("specular_features_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    L = ptss.device_lib()
    results = {}
    for name in SCENES:
        scene = ptss.Scene(name)
        r = ptss.Renderer(scene, W, H, sync_each_frame=False)
        d_first, d_feat = r.features_devptr(), r.features_specular_devptr()
        d_steps = r._device_buffer("specular_steps", r.local_pixels * 4)
        first = timed(lambda: ptss._check(L.ptss_render_features(r._ctx, d_first, None)))
        res = {"features_ms": first, "specular": {}}
        print(f"{name}/{W}x{H}: first-hit features {first['median']:.3f} ms [{first['min']:.3f}, {first['max']:.3f}]", flush=True)
        for max_steps in MAX_STEPS:
            t = timed(lambda: ptss._check(L.ptss_render_features_specular(r._ctx, max_steps, d_feat, d_steps, None)))
            _, steps = r.features_specular(max_steps, steps=True)
            mean = float(steps.mean())
            per_wave = steps[:len(steps) // 64 * 64].reshape(-1, 64).max(axis=1)   # a wave = 64 consecutive local pixels
            product = first["median"] * (1.0 + mean)
            wave_bound = first["median"] * (1.0 + float(per_wave.mean()))
            res["specular"][str(max_steps)] = {"ms": t, "mean_steps": mean, "pixels_with_steps": float((steps > 0).mean()),
                                               "histogram": np.bincount(steps, minlength=max_steps + 1).tolist(),
                                               "yardstick_ms": product, "factor": t["median"] / product,
                                               "mean_of_wave_max_steps": float(per_wave.mean()), "wave_bound_ms": wave_bound,
                                               "factor_over_wave_bound": t["median"] / wave_bound}
            print(f"    maxSteps {max_steps}: {t['median']:.3f} ms [{t['min']:.3f}, {t['max']:.3f}], mean steps {mean:.3f}, "
                  f"first-hit x (1 + mean) = {product:.3f} ms, factor {t['median'] / product:.2f}; mean of a wave's max steps "
                  f"{per_wave.mean():.3f}, first-hit x (1 + that) = {wave_bound:.3f} ms, factor {t['median'] / wave_bound:.2f}", flush=True)
        inplace, lds = r.specular_feature_launches()
        res["scene_image"] = "in LDS" if lds else "in place"
        results[f"{name}/{W}x{H}"] = res
        r.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
