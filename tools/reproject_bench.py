"""tools/reproject_bench.py [runs=5] [calls=50] [out.json] — time of ptss_reproject on one GPU.

1920x1080 and 3840x2160, the "mixed" preset: four frames at the default pose become the history, the camera moves ('w', 'd', 'f'),
one frame is rendered there, and ptss_reproject is timed: HIP events around `calls` back-to-back calls on the context's stream,
after a warm-up of the same shape, `runs` times; milliseconds per call, median [min, max]. Also timed: the call without a history
(out = (c, n)), ptss_denoise_history at 5 levels, and one pass of ptss_generate_frame at one sample per pixel of the same context
in the same process — the yardstick. The algorithmic bytes count every input and output element once: per pixel the accumulator
entry (12 B), the current feature (32 B), one previous feature and one history entry (32 + 16 B: neighbouring
pixels share their taps) and the entry written (16 B). Written to stdout and out.json."""
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
BYTES_PER_PIXEL = 12 + 32 + 32 + 16 + 16


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
        raise SystemExit("reproject_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    L = ptss.device_lib()
    H = ptss._hip_lib()
    results = {}
    for w, h in SIZES:
        r = ptss.Renderer(ptss.Scene("mixed"), w, h, sync_each_frame=False)
        pixels_dev = r.pixels_devptr()
        cam_a = ptss.default_camera()
        for _ in range(4):
            r.generate_frame()
        r.synchronize()
        n = r.local_pixels
        d_fa, d_ha, d_hb = (r._device_buffer(name, n * size) for name, size in (("features_a", 32), ("history_a", 16), ("history_b", 16)))
        d_fb, d_out = r.features_devptr(), r._device_buffer("denoised", n * 4)
        p = ptss.default_reproject_params()
        ptss._check(L.ptss_render_features(r._ctx, d_fa, None))
        ptss._check(L.ptss_reproject(r._ctx, d_fa, None, None, None, C.byref(p), d_ha, None))
        cam_b = ptss.default_camera()
        for k in "wdf":
            ptss.move_camera(cam_b, k)
        r.set_camera(cam_b)
        r.generate_frame()
        ptss._check(L.ptss_render_features(r._ctx, d_fb, None))
        r.synchronize()
        res = {"reproject_ms": timed(lambda: ptss._check(L.ptss_reproject(r._ctx, d_fb, C.byref(cam_a), d_fa, d_ha, C.byref(p), d_hb, None))),
               "no_history_ms": timed(lambda: ptss._check(L.ptss_reproject(r._ctx, d_fb, None, None, None, C.byref(p), d_hb, None)))}
        ptss._check(L.ptss_reproject(r._ctx, d_fb, C.byref(cam_a), d_fa, d_ha, C.byref(p), d_hb, None))
        with_history = float((r.read_history(d_hb)["weight"] > 1).mean())
        dn = ptss.default_denoise_params(levels=5)
        res["denoise_history_5_ms"] = timed(lambda: ptss._check(L.ptss_denoise_history(r._ctx, d_hb, d_fb, C.byref(dn), d_out, None)))
        res["pass_ms"] = timed(lambda: r.generate_frame(pixels_dev))
        res["algorithmic_bytes"] = n * BYTES_PER_PIXEL
        res["GB_per_s"] = res["algorithmic_bytes"] / (res["reproject_ms"]["median"] * 1e6)
        res["pixels_with_history"] = with_history
        results[f"mixed/{w}x{h}"] = res
        a, b, d, ps = res["reproject_ms"], res["no_history_ms"], res["denoise_history_5_ms"], res["pass_ms"]
        print(f"mixed/{w}x{h}: reproject {a['median']:.3f} ms [{a['min']:.3f}, {a['max']:.3f}] ({res['algorithmic_bytes'] / 1e6:.1f} MB algorithmic, "
              f"{res['GB_per_s']:.0f} GB/s, {100 * with_history:.1f} % of the pixels with history)  without a history {b['median']:.3f} ms "
              f"[{b['min']:.3f}, {b['max']:.3f}]  denoise_history 5 levels {d['median']:.3f} ms [{d['min']:.3f}, {d['max']:.3f}]  "
              f"one S = 1 pass {ps['median']:.3f} ms [{ps['min']:.3f}, {ps['max']:.3f}]", flush=True)
        r.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
