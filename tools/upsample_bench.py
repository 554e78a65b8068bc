"""tools/upsample_bench.py [runs=5] [calls=50] [out.json] — what rendering below display size costs and saves, one GPU.

960x540 -> 1920x1080 and 1920x1080 -> 3840x2160 at factor 2, the "mixed" and "mesh" presets, one sample per tick. Per figure: HIP
events around `calls` back-to-back calls on the context's stream, after a warm-up of the same shape, `runs` times; milliseconds per
call, median [min, max]. Measured in one process, the small context and the large one side by side:
  ptss_render_features_scaled of the small context    against  ptss_render_features of the large one (the same kernel, the same rays)
  ptss_upsample (bytes only)                          against  one ptss_denoise level at the large size; with its algorithmic bytes
                                                               (36 + 36 / f^2 per hi-res pixel) and the GB/s they amount to
  the small path: frame + features + 5 denoise levels + scaled features + upsample
                                                      against  the large path: frame + features + 5 denoise levels
No ratio is fixed in advance; they are printed as measured. Written to stdout and out.json."""
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
FACTOR = 2
SIZES = [(960, 540), (1920, 1080)]
SCENES = ["mixed", "mesh"]


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


def show(t):
    return f"{t['median']:.3f} ms [{t['min']:.3f}, {t['max']:.3f}]"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("upsample_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    L = ptss.device_lib()
    results = {}
    for name in SCENES:
        for w, h in SIZES:
            scene = ptss.Scene(name)
            lo = ptss.Renderer(scene, w, h, sync_each_frame=False)
            hi = ptss.Renderer(scene, w * FACTOR, h * FACTOR, sync_each_frame=False)
            up = ptss.default_upsample_params(factor=FACTOR)
            one, five = ptss.default_denoise_params(levels=1), ptss.default_denoise_params(levels=5)
            lo_pix, lo_feat, lo_den, lo_hi_feat = lo.pixels_devptr(), lo.features_devptr(), lo._device_buffer("denoised", w * h * 4), \
                lo.features_scaled_devptr(FACTOR)
            lo_out = lo._device_buffer("upsampled", w * h * FACTOR * FACTOR * 4)
            hi_pix, hi_feat, hi_den = hi.pixels_devptr(), hi.features_devptr(), hi._device_buffer("denoised", w * h * FACTOR * FACTOR * 4)
            check = ptss._check

            def small_path():
                lo.generate_frame()
                check(L.ptss_render_features(lo._ctx, lo_feat, None))
                check(L.ptss_denoise(lo._ctx, lo_feat, C.byref(five), lo_den, None))
                check(L.ptss_render_features_scaled(lo._ctx, FACTOR, lo_hi_feat, None))
                check(L.ptss_upsample(lo._ctx, lo_den, lo_feat, lo_hi_feat, C.byref(up), lo_out, None, None))

            def large_path():
                hi.generate_frame()
                check(L.ptss_render_features(hi._ctx, hi_feat, None))
                check(L.ptss_denoise(hi._ctx, hi_feat, C.byref(five), hi_den, None))

            small_path()
            large_path()   # every buffer holds what the single calls below read
            res = {
                "features_scaled_ms": timed(lambda: check(L.ptss_render_features_scaled(lo._ctx, FACTOR, lo_hi_feat, None))),
                "features_large_context_ms": timed(lambda: check(L.ptss_render_features(hi._ctx, hi_feat, None))),
                "upsample_ms": timed(lambda: check(L.ptss_upsample(lo._ctx, lo_den, lo_feat, lo_hi_feat, C.byref(up), lo_out, None, None))),
                "denoise_one_level_large_ms": timed(lambda: check(L.ptss_denoise(hi._ctx, hi_feat, C.byref(one), hi_den, None))),
                "small_frame_ms": timed(lo.generate_frame),
                "large_frame_ms": timed(hi.generate_frame),
                "small_path_ms": timed(small_path),
                "large_path_ms": timed(large_path),
            }
            hi_pixels = w * h * FACTOR * FACTOR
            res["upsample_algorithmic_bytes"] = int(hi_pixels * 36 + w * h * 36)
            res["upsample_GBps"] = res["upsample_algorithmic_bytes"] / (res["upsample_ms"]["median"] * 1e-3) / 1e9
            res["ratio_features_scaled_over_large_context"] = res["features_scaled_ms"]["median"] / res["features_large_context_ms"]["median"]
            res["ratio_upsample_over_denoise_level"] = res["upsample_ms"]["median"] / res["denoise_one_level_large_ms"]["median"]
            res["ratio_small_path_over_large_path"] = res["small_path_ms"]["median"] / res["large_path_ms"]["median"]
            key = f"{name}/{w}x{h}->{w * FACTOR}x{h * FACTOR}"
            results[key] = res
            print(f"{key}:", flush=True)
            print(f"    scaled features {show(res['features_scaled_ms'])}; features of the large context {show(res['features_large_context_ms'])}; "
                  f"ratio {res['ratio_features_scaled_over_large_context']:.3f}")
            print(f"    upsample {show(res['upsample_ms'])}, {res['upsample_algorithmic_bytes'] / 1e6:.1f} MB algorithmic = "
                  f"{res['upsample_GBps']:.0f} GB/s; one denoise level at the large size {show(res['denoise_one_level_large_ms'])}; "
                  f"ratio {res['ratio_upsample_over_denoise_level']:.3f}")
            print(f"    frame alone: small {show(res['small_frame_ms'])}, large {show(res['large_frame_ms'])}")
            print(f"    small path {show(res['small_path_ms'])}; large path {show(res['large_path_ms'])}; "
                  f"ratio {res['ratio_small_path_over_large_path']:.3f}", flush=True)
            assert lo.upsample_launches() > 0
            lo.close()
            hi.close()
    out = {"runs": runs, "calls": calls, "unit": "ms per call", "factor": FACTOR, "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
