"""tools/film_bench.py [runs=5] [window_ms=100] [out.json] — what the film of a path query costs (ptss_generate_rays, ptss_accumulate_paths,
ptss_ray_features) on one GPU.

1920x1080, one process. Per figure: HIP events around a window of back-to-back calls on the current stream — as many calls as fill
`window_ms` (at least five; counted from a pilot window), since the streaming calls take tens of microseconds each —, after a warm-up
of the same shape, `runs` times; milliseconds per call, median [min, max], and the calls per window.
  generate     ptss_generate_rays over the whole film, jitter 1, for each model
  accumulate   ptss_accumulate_paths: the identity map without outputs, the identity map with pixels and history, a permuted index
               with pixels and history
  features     ptss_ray_features of the film's jitter = 0 pinhole rays against ptss_render_features of the same context ("mixed")
Each against its algorithmic bytes (what the call must read and write once: streams 24 B in and out, rays 32 B, results 16 B, a film
entry 16 B in and out, a pixel 4 B, a history entry 16 B, an index entry 4 B per launch that reads it, a feature row 32 B) and against
a device-to-device copy moving the same number of bytes (half read, half written), timed in the same run.
  round        generate + ptss_trace_paths + accumulate (pixels on) against one S = 1 ptss_generate_frame and against ptss_trace_paths
               alone, on "mixed" and "mesh": what the film adds to a path query. And the round once more with the trace on the refill
               schedule (ptss_trace_paths_opt, PTSS_PATHS_REFILL).
No figure is fixed in advance. Written to stdout and out.json."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
window_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 100.0
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080
N = W * H
SEED = 0x5EED


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed(fn):
    for _ in range(3):
        fn()   # warm-up of this shape
    torch.cuda.synchronize()
    calls = max(5, min(20000, int(window_ms / max(window(fn, 5), 1e-4)) + 1))   # the pilot window sizes the timed ones
    ms = sorted(window(fn, calls) for _ in range(runs))
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1], "calls": calls}


def copy_of(nbytes):
    """A device-to-device copy that moves nbytes in all: nbytes / 2 read, nbytes / 2 written."""
    src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src))


def against_bytes(t, bytes_per_ray):
    nbytes = bytes_per_ray * N
    c = copy_of(nbytes)
    return {"ms": t, "bytes_per_ray": bytes_per_ray, "GB_per_s": nbytes / t["median"] / 1e6, "copy_ms": c, "copy_GB_per_s": nbytes / c["median"] / 1e6,
            "rate_over_copy": c["median"] / t["median"]}


def show(what, r):
    t, c = r["ms"], r["copy_ms"]
    print(f"{what}: {t['median']:.4f} ms [{t['min']:.4f}, {t['max']:.4f}], {r['bytes_per_ray']} B/ray = {r['GB_per_s']:.0f} GB/s; a copy of those bytes "
          f"{c['median']:.4f} ms [{c['min']:.4f}, {c['max']:.4f}] = {r['copy_GB_per_s']:.0f} GB/s; rate / copy's {r['rate_over_copy']:.2f}", flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("film_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    cam = ptss.default_camera()
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    d_rng = r.seed_path_rng(N, SEED, device=True)
    d_rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    for kind in ("pinhole", "thinlens", "equirect"):
        film = ptss.film_camera(kind, W, H, cam, lens_radius=0.05, focus_distance=5.0)
        res = against_bytes(timed(lambda: r.generate_rays(film, d_rng, rays=d_rays)), 24 + 24 + 32)
        results[f"generate/{kind}"] = res
        show(f"generate {kind}", res)

    d_res = torch.rand((N, 4), dtype=torch.float32, device="cuda")
    d_film = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.int32).contiguous()
    cases = (("identity", None, None, None, 16 + 16 + 16), ("identity, pixels and history", None, d_px, d_hist, 16 + 16 + 16 + 4 + 16),
             ("permuted index, pixels and history", perm, d_px, d_hist, (16 + 4 + 16 + 16) + (4 + 16 + 4 + 16)))
    for what, index, px, hist, nbytes in cases:
        d_film.zero_()   # samples stay far below 2^24 over the calls of one figure
        res = against_bytes(timed(lambda: r.accumulate_paths(d_res, d_film, index=index, pixels=px, history=hist)), nbytes)
        results[f"accumulate/{what}"] = res
        show(f"accumulate {what}", res)

    centre = r.generate_rays(ptss.film_camera("pinhole", W, H, cam, jitter=0), d_rng)
    res = against_bytes(timed(lambda: r.ray_features(centre)), 32 + 32)
    d_feat = r.features_devptr()
    stream = torch.cuda.current_stream().cuda_stream
    L = ptss.device_lib()
    render = timed(lambda: ptss._check(L.ptss_render_features(r._ctx, d_feat, stream)))
    res["render_features_ms"] = render
    res["over_render_features"] = res["ms"]["median"] / render["median"]
    results["features/mixed"] = res
    show("ray_features (mixed)", res)
    print(f"  ptss_render_features of the same context: {render['median']:.4f} ms [{render['min']:.4f}, {render['max']:.4f}]; "
          f"ray_features / render_features {res['over_render_features']:.2f}", flush=True)
    r.close()

    for name in ("mixed", "mesh"):
        r = ptss.Renderer(ptss.Scene(name), W, H, seed=SEED, sync_each_frame=False)
        iterations = int(r.cfg.maxIterations)
        film = ptss.film_camera("pinhole", W, H, cam)
        d_rng = r.seed_path_rng(N, SEED, device=True)
        d_film.zero_()

        def whole():
            r.generate_rays(film, d_rng, rays=d_rays)
            out = r.trace_paths(d_rays, d_rng, iterations)
            r.accumulate_paths(out, d_film, pixels=d_px)

        def whole_refill():
            r.generate_rays(film, d_rng, rays=d_rays)
            out = r.trace_paths(d_rays, d_rng, iterations, schedule="refill")
            r.accumulate_paths(out, d_film, pixels=d_px)

        frame = timed(lambda: r.generate_frame())
        rounds = timed(whole)
        refill = timed(whole_refill)
        paths = timed(lambda: r.trace_paths(d_rays, d_rng, iterations))
        res = {"maxIterations": iterations, "frame_ms": frame, "round_ms": rounds, "paths_ms": paths, "round_over_frame": rounds["median"] / frame["median"],
               "round_over_paths": rounds["median"] / paths["median"], "film_adds_ms": rounds["median"] - paths["median"], "refill_round_ms": refill,
               "refill_round_over_frame": refill["median"] / frame["median"], "refill_round_over_round": refill["median"] / rounds["median"]}
        results[f"round/{name}"] = res
        print(f"round {name}, {iterations} iterations: frame {frame['median']:.3f} ms [{frame['min']:.3f}, {frame['max']:.3f}]; generate + trace + "
              f"accumulate {rounds['median']:.3f} ms [{rounds['min']:.3f}, {rounds['max']:.3f}] = {res['round_over_frame']:.2f} x frame; trace alone "
              f"{paths['median']:.3f} ms [{paths['min']:.3f}, {paths['max']:.3f}]: the film adds {res['film_adds_ms']:.3f} ms = "
              f"{100 * (res['round_over_paths'] - 1):.1f} %; the round with the refill trace {refill['median']:.3f} ms [{refill['min']:.3f}, "
              f"{refill['max']:.3f}] = {res['refill_round_over_frame']:.2f} x frame = {res['refill_round_over_round']:.2f} x the round", flush=True)
        r.close()
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
