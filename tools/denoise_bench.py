"""tools/denoise_bench.py [runs=5] [calls=50] [out.json] — time of ptss_render_features and ptss_denoise on one GPU.

1920x1080 and 3840x2160, the "mixed" and "mesh" presets. Per figure: HIP events around `calls` back-to-back calls on the context's
stream, after a warm-up of the same shape, `runs` times; milliseconds per call, median [min, max]. Measured: the feature kernel;
ptss_denoise at 1 .. 5 levels (1, 3 and 5 are the headline figures; the time of level k is the step from k - 1 to k levels, in
which pass k - 1 also turns from the byte-writing into a plane-writing pass); and one pass of ptss_generate_frame at one sample
per pixel of the same context in the same process — the pass the filter cleans up, the yardstick. Per level the algorithmic
bytes (every input and output element once, computed from the shapes below) over that time. Written to stdout and out.json."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
out_path = sys.argv[3] if len(sys.argv) > 3 else None
SIZES = [(1920, 1080), (3840, 2160)]
SCENES = ["mixed", "mesh"]


def pass_bytes(pixels, level, levels):
    """Algorithmic bytes of pass `level` of a `levels`-pass denoise: each pixel's colour (12 B from the accumulator in the first
    pass, else a 16-B plane entry), its feature row and material index (16 + 4 B) read once, its result written once (4 B of
    display in the last pass, else a 16-B plane entry)."""
    read = (12 if level == 0 else 16) + 20
    write = 4 if level == levels - 1 else 16
    return pixels * (read + write)


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
        raise SystemExit("denoise_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    L = ptss.device_lib()
    results = {}
    for w, h in SIZES:
        for name in SCENES:
            scene = ptss.Scene(name)
            r = ptss.Renderer(scene, w, h, sync_each_frame=False)
            key = f"{name}/{w}x{h}"
            pixels_dev = r.pixels_devptr()
            for _ in range(4):
                r.generate_frame()
            r.synchronize()
            d_feat, d_out = r.features_devptr(), r._device_buffer("denoised", r.local_pixels * 4)
            res = {"features_ms": timed(lambda: ptss._check(L.ptss_render_features(r._ctx, d_feat, None)))}
            per_levels = {}
            for levels in range(1, 6):
                p = ptss.default_denoise_params(levels=levels)
                per_levels[levels] = timed(lambda: ptss._check(L.ptss_denoise(r._ctx, d_feat, C.byref(p), d_out, None)))
            res["denoise_ms"] = {str(k): v for k, v in per_levels.items()}
            res["levels"] = []
            for k in range(1, 6):
                step = per_levels[k]["median"] - (per_levels[k - 1]["median"] if k > 1 else 0.0)
                nbytes = pass_bytes(w * h, k - 1, 5)
                res["levels"].append({"level": k - 1, "spacing": 1 << (k - 1), "step_ms": step, "algorithmic_bytes": nbytes,
                                      "GB_per_s": nbytes / (step * 1e6) if step > 0 else None})
            res["pass_ms"] = timed(lambda: r.generate_frame(pixels_dev))
            results[key] = res
            f, d, ps = res["features_ms"], res["denoise_ms"], res["pass_ms"]
            print(f"{key:18s} features {f['median']:.3f} ms [{f['min']:.3f}, {f['max']:.3f}]  denoise 1 / 3 / 5 levels "
                  f"{d['1']['median']:.3f} / {d['3']['median']:.3f} / {d['5']['median']:.3f} ms "
                  f"[{d['5']['min']:.3f}, {d['5']['max']:.3f}]  one S = 1 pass {ps['median']:.3f} ms [{ps['min']:.3f}, {ps['max']:.3f}]", flush=True)
            for lv in res["levels"]:
                rate = f"{lv['GB_per_s']:.0f} GB/s" if lv["GB_per_s"] else "n/a"
                print(f"    level {lv['level']} (spacing {lv['spacing']:2d}): {lv['step_ms']:.3f} ms, {lv['algorithmic_bytes'] / 1e6:.1f} MB algorithmic, {rate}",
                      flush=True)
            r.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
