"""tools/splat_bench.py [runs=5] [window_ms=50] [out.json] — what the filtered linear film costs (ptss_generate_rays_positions,
ptss_splat_paths, ptss_splat_paths_homed, ptss_resolve_splat) on one GPU.

1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  homed        ptss_splat_paths_homed on one sample per pixel in pixel order (a real round's positions and radiance), tent R = 1 and
               Gaussian R = 2, beside ptss_splat_paths on the same batch, ptss_accumulate_paths_linear on the identity map and a device copy
               of the homed call's algorithmic bytes (16 B result, 8 B position and 32 B entry read, 32 B written: 88 B per pixel)
  scatter      ptss_splat_paths on that batch in pixel order and in a random permutation, beside ptss_accumulate_paths_linear on the
               permuted index
  resolve      ptss_resolve_splat with all three outputs beside ptss_resolve_linear and a device copy of their bytes
  generate     ptss_generate_rays_positions beside ptss_generate_rays
  round        generate with positions + refill trace + homed splat + resolve on "mixed", beside the linear round of §3.29
No figure is fixed in advance. Written to stdout and out.json."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402
import linear_bench as lb  # noqa: E402  (window, timed_legs, against_copy, fmt: one set of timing helpers)

W, H, N, SEED = lb.W, lb.H, lb.N, lb.SEED
out_path = lb.out_path


def main():
    if not torch.cuda.is_available():
        raise SystemExit("splat_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params = ptss.linear_params()
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    pos = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    splat = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    linear = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    d_means = torch.zeros((N, 4), dtype=torch.float32, device="cuda")

    r.generate_rays(film_cam, rng, rays=rays, positions=pos)   # a real round: its positions and its radiance
    d_res = r.trace_paths(rays, rng, iterations).clone()
    perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res_perm, pos_perm = d_res[perm].contiguous(), pos[perm].contiguous()
    index_perm = perm.to(torch.int32).contiguous()
    torch.cuda.synchronize()

    def reset():
        splat.zero_()
        linear.zero_()

    tent, gauss = ptss.splat_filter("tent", 1.0), ptss.splat_filter("gaussian", 2.0, 2.0)
    for what, flt in (("tent R=1", tent), ("gaussian R=2", gauss)):
        res = lb.against_copy({"call": lambda: r.splat_paths(d_res, pos, splat, W, H, filter=flt, params=params, homed_first_pixel=0),
                               "scatter": lambda: r.splat_paths(d_res, pos, splat, W, H, filter=flt, params=params),
                               "linear": lambda: r.accumulate_paths_linear(d_res, linear, params=params)}, 88 * N, reset)
        results[f"homed/{what}"] = res
        print(f"splat_paths_homed {what}: {lb.fmt(res['ms'])} = {res['GB_per_s']:.0f} GB/s of its 88 B per pixel; a copy of those bytes "
              f"{lb.fmt(res['copy_ms'])}; splat_paths on the same batch {lb.fmt(res['scatter_ms'])}: homed / scatter {res['call_over_scatter']:.3f}; "
              f"accumulate_paths_linear, identity {lb.fmt(res['linear_ms'])}: homed / linear {res['call_over_linear']:.2f}", flush=True)
    t = lb.timed_legs({"pixel order": lambda: r.splat_paths(d_res, pos, splat, W, H, filter=tent, params=params),
                       "permuted": lambda: r.splat_paths(res_perm, pos_perm, splat, W, H, filter=tent, params=params),
                       "linear, permuted index": lambda: r.accumulate_paths_linear(d_res, linear, index=index_perm, params=params)}, reset)
    t["permuted_over_linear"] = t["permuted"]["median"] / t["linear, permuted index"]["median"]
    results["scatter/tent R=1"] = t
    print(f"splat_paths tent R=1: pixel order {lb.fmt(t['pixel order'])}, permuted {lb.fmt(t['permuted'])}; accumulate_paths_linear on the permuted "
          f"index {lb.fmt(t['linear, permuted index'])}: scatter / linear {t['permuted_over_linear']:.2f}", flush=True)
    reset()
    r.splat_paths(d_res, pos, splat, W, H, filter=tent, params=params, homed_first_pixel=0)
    r.accumulate_paths_linear(d_res, linear, params=params)
    res = lb.against_copy({"call": lambda: r.resolve_splat(splat, params=params, linear=d_means, pixels=d_px, history=d_hist),
                           "linear": lambda: r.resolve_linear(linear, params=params, linear=d_means, pixels=d_px, history=d_hist)}, 68 * N)
    results["resolve"] = res
    print(f"resolve_splat, three outputs: {lb.fmt(res['ms'])}; a copy of its 68 B per pixel {lb.fmt(res['copy_ms'])}; resolve_linear "
          f"{lb.fmt(res['linear_ms'])}: splat / linear {res['call_over_linear']:.2f}", flush=True)
    t = lb.timed_legs({"positions": lambda: r.generate_rays(film_cam, rng, rays=rays, positions=pos),
                       "plain": lambda: r.generate_rays(film_cam, rng, rays=rays)})
    t["positions_over_plain"] = t["positions"]["median"] / t["plain"]["median"]
    results["generate"] = t
    print(f"generate_rays with positions {lb.fmt(t['positions'])}, without {lb.fmt(t['plain'])}: {t['positions_over_plain']:.3f}", flush=True)

    def round_splat():
        r.generate_rays(film_cam, rng, rays=rays, positions=pos)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.splat_paths(o, pos, splat, W, H, filter=tent, params=params, homed_first_pixel=0)
        r.resolve_splat(splat, params=params, linear=d_means, pixels=d_px, history=d_hist)

    def round_linear():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=params)
        r.resolve_linear(linear, params=params, linear=d_means, pixels=d_px, history=d_hist)

    t = lb.timed_legs({"splat": round_splat, "linear": round_linear}, reset)
    t["splat_over_linear"] = t["splat"]["median"] / t["linear"]["median"]
    results["round"] = t
    print(f"round on mixed (generate, refill trace, film, resolve): homed tent {lb.fmt(t['splat'])}, linear {lb.fmt(t['linear'])}: "
          f"splat / linear {t['splat_over_linear']:.3f}", flush=True)
    stats = r.splat_stats()
    results["stats"] = {"dropped": stats[3], "clamped": stats[4]}
    r.close()
    out = {"runs": lb.runs, "window_ms": lb.window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
