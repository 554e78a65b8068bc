"""tools/linear_bench.py [runs=5] [window_ms=50] [out.json] — what the linear film costs (ptss_accumulate_paths_linear,
ptss_resolve_linear) on one GPU.

1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  accumulate   ptss_accumulate_paths_linear on the identity map (16 B result and 32 B entry read, 32 B written: 80 B per ray), on a plan's
               sorted index ("mixed" after 8 uniform rounds, §3.28's set-up: 20 B per ray and 64 B per named pixel) and on a random
               permutation (84 B per ray), each against a device copy of its algorithmic bytes and against ptss_accumulate_paths (sums only,
               no pixels, no history) on the same map
  resolve      ptss_resolve_linear with all three outputs (32 B read, 36 B written) against a device copy of those bytes
  round        generate + refill trace + linear accumulate + resolve on "mixed", against the same round with ptss_accumulate_paths (pixels
               and history)
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
window_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 50.0
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080
N = W * H
SEED = 0x5EED
MAX_CALLS = 2000   # a pixel of a sorted index takes many samples per call: the 8-bit film stays far below 2^24


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed_legs(legs, reset=None):
    """legs: name -> fn. Every leg warmed, then `runs` rounds in which the legs take turns, one window each."""
    calls = {}
    for name, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(5, min(MAX_CALLS, int(window_ms / max(window(fn, 5), 1e-4)) + 1))
    ms = {name: [] for name in legs}
    for _ in range(runs):
        for name, fn in legs.items():
            if reset:
                reset()
            ms[name].append(window(fn, calls[name]))
    return {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "calls": calls[name]} for name, v in ms.items()}


def fmt(t):
    return f"{t['median']:.4f} ms [{t['min']:.4f}, {t['max']:.4f}]"


def against_copy(legs, nbytes, reset=None):
    """legs["call"] (and any others) beside a device copy of nbytes (half read, half written)."""
    src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    t = timed_legs(dict(legs, copy=lambda: dst.copy_(src)), reset)
    out = {"ms": t["call"], "bytes": nbytes, "GB_per_s": nbytes / t["call"]["median"] / 1e6, "copy_ms": t["copy"],
           "copy_GB_per_s": nbytes / t["copy"]["median"] / 1e6, "rate_over_copy": t["copy"]["median"] / t["call"]["median"]}
    for name in legs:
        if name != "call":
            out[name + "_ms"] = t[name]
            out["call_over_" + name] = t["call"]["median"] / t[name]["median"]
    return out


def show(what, r):
    line = (f"{what}: {fmt(r['ms'])}, {r['bytes'] / N:.1f} B per ray = {r['GB_per_s']:.0f} GB/s; a copy of those bytes {fmt(r['copy_ms'])} = "
            f"{r['copy_GB_per_s']:.0f} GB/s; rate / copy's {r['rate_over_copy']:.2f}")
    if "plain_ms" in r:
        line += f"; accumulate_paths on the same map {fmt(r['plain_ms'])}: linear / plain {r['call_over_plain']:.2f}"
    print(line, flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("linear_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    cam = ptss.default_camera()
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film_cam = ptss.film_camera("pinhole", W, H, cam)
    params = ptss.linear_params()
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    film8 = torch.zeros((N, 4), dtype=torch.int32, device="cuda")
    moments = torch.zeros(N, dtype=torch.int64, device="cuda")
    linear = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    d_means = torch.zeros((N, 4), dtype=torch.float32, device="cuda")

    # §3.28's set-up: 8 uniform rounds of "mixed", then the plan's index; the linear film takes the same samples
    plan_params = ptss.plan_params()
    for _ in range(plan_params.minSamples):
        r.generate_rays(film_cam, rng, rays=rays)
        out = r.trace_paths(rays, rng, iterations)
        r.accumulate_paths_stats(out, film8, moments, pixels=d_px)
        r.accumulate_paths_linear(out, linear, params=params)
    plan = torch.zeros(N, dtype=torch.int32, device="cuda")
    r.plan_samples(film8, moments, N, plan_params, cdf=torch.zeros(ptss.plan_cdf_entries(N), dtype=torch.int64, device="cuda"), index=plan)
    torch.cuda.synchronize()
    runs_of = torch.unique_consecutive(plan, return_counts=True)[1]
    named = int(len(runs_of))
    results["sorted/index"] = {"pixels_named": named, "longest_run": int(runs_of.max()), "mean_run": float(runs_of.float().mean())}
    print(f"the plan's index names {named} pixels in runs of {float(runs_of.float().mean()):.2f} on average, {int(runs_of.max())} at most", flush=True)
    perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.int32).contiguous()

    d_res = out.clone()   # the radiance of a real round
    film0, linear0 = film8.clone(), linear.clone()

    def reset():
        film8.copy_(film0)
        linear.copy_(linear0)

    for what, index, nbytes in (("identity", None, 80 * N), ("plan's index", plan, 20 * N + 64 * named), ("permuted index", perm, 84 * N)):
        res = against_copy({"call": lambda: r.accumulate_paths_linear(d_res, linear, index=index, params=params),
                            "plain": lambda: r.accumulate_paths(d_res, film8, index=index)}, nbytes, reset)
        results[f"accumulate/{what}"] = res
        show(f"accumulate_paths_linear {what}", res)
    reset()
    res = against_copy({"call": lambda: r.resolve_linear(linear, params=params, linear=d_means, pixels=d_px, history=d_hist)}, 68 * N)
    results["resolve"] = res
    show("resolve_linear, three outputs", res)

    def round_linear():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=params)
        r.resolve_linear(linear, params=params, linear=d_means, pixels=d_px, history=d_hist)

    def round_plain():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths(o, film8, pixels=d_px, history=d_hist)

    t = timed_legs({"linear": round_linear, "plain": round_plain}, reset)
    t["linear_over_plain"] = t["linear"]["median"] / t["plain"]["median"]
    results["round"] = t
    print(f"round on mixed (generate, refill trace, accumulate, resolve): linear {fmt(t['linear'])}, accumulate_paths {fmt(t['plain'])}: "
          f"linear / plain {t['linear_over_plain']:.3f}", flush=True)
    r.close()
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
