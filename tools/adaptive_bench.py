"""tools/adaptive_bench.py [runs=5] [window_ms=50] [out.json] [reference_rounds=4096] — what adaptive film sampling costs and what it buys
(ptss_accumulate_paths_stats, ptss_plan_samples) on one GPU.

Timing, 1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape,
`runs` windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  plan         ptss_plan_samples of a film of "mixed" after 8 uniform rounds, n = width * height, against its algorithmic bytes (film 16 B
               and moment 8 B read, cdf 8 B and index 4 B written) and a device copy of those bytes
  stats        ptss_accumulate_paths_stats: the identity map without and with pixels and history, against their algorithmic bytes
               (ptss_accumulate_paths' plus the moment's 8 B in and out) and a device copy
  sorted       ptss_accumulate_paths_stats against ptss_accumulate_paths on the plan's own index (sorted, duplicates in runs), and both
               on the permuted index of §3.26
Quality, "mixed" and "cornell" at 256x256: 8 uniform + 24 planned rounds against 32 uniform rounds — the same ray count — as the mean
squared error of the display pixels against a film of `reference_rounds` uniform rounds, with the share of the planned rays that went
to the noisiest tenth of the pixels (by the reference film's own variance). No figure is fixed in advance. Written to stdout and out.json."""
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
reference_rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 4096
W, H = 1920, 1080
N = W * H
SEED = 0x5EED
MAX_CALLS = 2000   # a pixel of a sorted index takes many samples per call: the film stays far below 2^24


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


def with_copy(fn, nbytes, reset=None):
    src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")   # nbytes / 2 read, nbytes / 2 written
    dst = torch.empty_like(src)
    t = timed_legs({"call": fn, "copy": lambda: dst.copy_(src)}, reset)
    return {"ms": t["call"], "bytes": nbytes, "GB_per_s": nbytes / t["call"]["median"] / 1e6, "copy_ms": t["copy"],
            "copy_GB_per_s": nbytes / t["copy"]["median"] / 1e6, "rate_over_copy": t["copy"]["median"] / t["call"]["median"]}


def fmt(t):
    return f"{t['median']:.4f} ms [{t['min']:.4f}, {t['max']:.4f}]"


def show(what, r):
    print(f"{what}: {fmt(r['ms'])}, {r['bytes'] / N:.0f} B per pixel = {r['GB_per_s']:.0f} GB/s; a copy of those bytes {fmt(r['copy_ms'])} = "
          f"{r['copy_GB_per_s']:.0f} GB/s; rate / copy's {r['rate_over_copy']:.2f}", flush=True)


class Film:
    """A film with moments on the device, and one round of the loop."""

    def __init__(self, r, width, height, cam, seed):
        self.r, self.P = r, width * height
        self.cam = ptss.film_camera("pinhole", width, height, cam)
        self.iterations = int(r.cfg.maxIterations)
        self.rng = r.seed_path_rng(self.P, seed, device=True)
        self.rays = torch.zeros((self.P, 8), dtype=torch.float32, device="cuda")
        self.film = torch.zeros((self.P, 4), dtype=torch.int32, device="cuda")
        self.moments = torch.zeros(self.P, dtype=torch.int64, device="cuda")
        self.pixels = torch.zeros((self.P, 4), dtype=torch.uint8, device="cuda")
        self.cdf = torch.zeros(ptss.plan_cdf_entries(self.P), dtype=torch.int64, device="cuda")
        self.index = torch.zeros(self.P, dtype=torch.int32, device="cuda")
        self.info = torch.zeros(4, dtype=torch.int64, device="cuda")

    def round(self, planned):
        index = self.index if planned else None
        self.r.generate_rays(self.cam, self.rng, index=index, rays=self.rays)
        out = self.r.trace_paths(self.rays, self.rng, self.iterations)
        self.r.accumulate_paths_stats(out, self.film, self.moments, index=index, pixels=self.pixels)

    def plan(self, params):
        self.r.plan_samples(self.film, self.moments, self.P, params, cdf=self.cdf, index=self.index, info=self.info)


def timing(results):
    cam = ptss.default_camera()
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    f = Film(r, W, H, cam, SEED)
    params = ptss.plan_params()
    for _ in range(params.minSamples):
        f.round(False)
    f.plan(params)
    torch.cuda.synchronize()
    info = ptss.plan_info_dict(f.info.cpu().numpy())
    results["plan/info"] = info
    print(f"the film of mixed after {params.minSamples} uniform rounds: {info}", flush=True)
    res = with_copy(lambda: f.plan(params), (16 + 8 + 8 + 4) * N)
    results["plan"] = res
    show("plan_samples, n = width * height", res)

    d_res = torch.rand((N, 4), dtype=torch.float32, device="cuda")
    film0, moments0 = f.film.clone(), f.moments.clone()
    d_film, d_m = torch.zeros_like(f.film), torch.zeros_like(f.moments)
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")

    def reset():
        d_film.copy_(film0)
        d_m.copy_(moments0)

    for what, px, hist, nbytes in (("identity", None, None, 16 + 32 + 16), ("identity, pixels and history", d_px, d_hist, 16 + 32 + 16 + 20)):
        res = with_copy(lambda: r.accumulate_paths_stats(d_res, d_film, d_m, pixels=px, history=hist), nbytes * N, reset)
        results[f"stats/{what}"] = res
        show(f"accumulate_paths_stats {what}", res)
    perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.int32).contiguous()
    plan = f.index.clone()
    runs_of = torch.unique_consecutive(plan, return_counts=True)[1]
    results["sorted/index"] = {"pixels_named": int(len(runs_of)), "longest_run": int(runs_of.max()), "mean_run": float(runs_of.float().mean())}
    print(f"the plan's index names {len(runs_of)} pixels in runs of {float(runs_of.float().mean()):.2f} on average, {int(runs_of.max())} at most", flush=True)
    for what, index in (("plan's index", plan), ("permuted index", perm)):
        t = timed_legs({"stats": lambda: r.accumulate_paths_stats(d_res, d_film, d_m, index=index, pixels=d_px, history=d_hist),
                        "plain": lambda: r.accumulate_paths(d_res, d_film, index=index, pixels=d_px, history=d_hist)}, reset)
        t["stats_over_plain"] = t["stats"]["median"] / t["plain"]["median"]
        results[f"sorted/{what}"] = t
        print(f"{what}, pixels and history: accumulate_paths_stats {fmt(t['stats'])}, accumulate_paths {fmt(t['plain'])}: "
              f"stats / plain {t['stats_over_plain']:.2f}", flush=True)
    r.close()


def quality(results):
    S = 256
    P = S * S
    for name in ("mixed", "cornell"):
        r = ptss.Renderer(ptss.Scene(name), S, S, seed=SEED, sync_each_frame=False)
        cam = ptss.default_camera()
        ref = Film(r, S, S, cam, SEED + 1)
        for _ in range(reference_rounds):
            ref.round(False)
        torch.cuda.synchronize()
        n = ref.film[:, 3].double()
        s, q = ref.film[:, :3].double(), ref.moments.double()
        variance = q / n - (s / n.unsqueeze(1)).pow(2).sum(dim=1)   # the summed variance of the three display channels
        noisiest = torch.zeros(P, dtype=torch.bool, device="cuda")
        noisiest[torch.argsort(variance, descending=True)[:P // 10]] = True
        truth = ref.pixels[:, :3].double()
        params = ptss.plan_params()
        uniform, adaptive = Film(r, S, S, cam, SEED), Film(r, S, S, cam, SEED)
        for _ in range(32):
            uniform.round(False)
        planned_to_noisiest = planned = 0
        for k in range(32):
            if k >= params.minSamples:
                adaptive.plan(params)
                counts = torch.bincount(adaptive.index.long(), minlength=P)
                planned_to_noisiest += int(counts[noisiest].sum())
                planned += int(counts.sum())
            adaptive.round(k >= params.minSamples)
        adaptive.plan(params)
        torch.cuda.synchronize()
        mse_u = float((uniform.pixels[:, :3].double() - truth).pow(2).mean())
        mse_a = float((adaptive.pixels[:, :3].double() - truth).pow(2).mean())
        assert int(uniform.film[:, 3].sum()) == int(adaptive.film[:, 3].sum()) == 32 * P
        res = {"size": f"{S}x{S}", "reference_rounds": reference_rounds, "mse_uniform_32": mse_u, "mse_8_uniform_24_planned": mse_a,
               "mse_ratio": mse_a / mse_u if mse_u else None, "share_of_planned_rays_to_noisiest_tenth": planned_to_noisiest / planned,
               "samples_min_max": [int(adaptive.film[:, 3].min()), int(adaptive.film[:, 3].max())], "final_info": ptss.plan_info_dict(adaptive.info.cpu().numpy())}
        results[f"quality/{name}"] = res
        print(f"quality {name} {S}x{S} against {reference_rounds} uniform rounds: MSE of the display pixels 32 uniform rounds {mse_u:.3f}, 8 uniform + 24 "
              f"planned {mse_a:.3f} (ratio {res['mse_ratio']:.3f}); {100 * res['share_of_planned_rays_to_noisiest_tenth']:.1f} % of the planned rays went to the "
              f"noisiest tenth of the pixels; samples per pixel {res['samples_min_max']}; final plan {res['final_info']}", flush=True)
        r.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    timing(results)
    quality(results)
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
