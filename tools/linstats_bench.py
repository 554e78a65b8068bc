"""tools/linstats_bench.py [runs=5] [window_ms=50] [out.json] [reference_rounds=4096] — what adaptive sampling on the linear film costs and
what it buys (ptss_accumulate_paths_linear_stats, ptss_plan_samples_linear) on one GPU.

Timing, 1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape,
`runs` windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  accumulate   ptss_accumulate_paths_linear_stats with a film on the identity map (16 B result, 32 B entry and 32 B moment row read, 64 B
               written: 144 B per ray), on the linear plan's sorted index ("mixed" after 8 uniform rounds: 20 B per ray and 128 B per named
               pixel) and on a random permutation (148 B per ray), each against a device copy of its algorithmic bytes and against
               ptss_accumulate_paths_linear on the same map; and with a NULL film on the plan's index
  plan         ptss_plan_samples_linear (32 B read, 12 B written per pixel) against ptss_plan_samples (24 B read, 12 B written) on films of
               the same size and the same scene, each beside a device copy of its bytes
  round        generate + refill trace + accumulate with moments + plan + resolve on "mixed", against §3.29's linear round (generate +
               refill trace + linear accumulate + resolve)
Quality, "mixed" and "cornell" at 256x256: 8 uniform + 24 planned rounds against 32 uniform rounds — the same ray count — on a linear film,
planned by ptss_plan_samples_linear and, for comparison, by the 8-bit ptss_plan_samples driving the same linear film; against a linear
film of `reference_rounds` uniform rounds: the mean squared error of the linear means, and the mean relative squared error
(x - ref)^2 / (ref + floor)^2. No figure is fixed in advance. Written to stdout and out.json."""
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


def show(what, r, other=None):
    line = (f"{what}: {fmt(r['ms'])}, {r['bytes'] / N:.1f} B per ray = {r['GB_per_s']:.0f} GB/s; a copy of those bytes {fmt(r['copy_ms'])} = "
            f"{r['copy_GB_per_s']:.0f} GB/s; rate / copy's {r['rate_over_copy']:.2f}")
    if other:
        line += f"; {other} on the same map {fmt(r['plain_ms'])}: ratio {r['call_over_plain']:.2f}"
    print(line, flush=True)


class Film:
    """A linear film with its luminance moments and, for the 8-bit plan, an 8-bit film with its moments, on the device."""

    def __init__(self, r, width, height, cam, seed):
        self.r, self.P = r, width * height
        self.cam = ptss.film_camera("pinhole", width, height, cam)
        self.iterations = int(r.cfg.maxIterations)
        self.params = ptss.linear_params()
        self.rng = r.seed_path_rng(self.P, seed, device=True)
        self.rays = torch.zeros((self.P, 8), dtype=torch.float32, device="cuda")
        self.linear = torch.zeros((self.P, 4), dtype=torch.int64, device="cuda")
        self.moments = torch.zeros((self.P, 4), dtype=torch.int64, device="cuda")
        self.film8 = torch.zeros((self.P, 4), dtype=torch.int32, device="cuda")
        self.moments8 = torch.zeros(self.P, dtype=torch.int64, device="cuda")
        self.cdf = torch.zeros(ptss.plan_cdf_entries(self.P), dtype=torch.int64, device="cuda")
        self.index = torch.zeros(self.P, dtype=torch.int32, device="cuda")
        self.info = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.means = torch.zeros((self.P, 4), dtype=torch.float32, device="cuda")

    def round(self, planned, eight_bit=False, schedule=None):
        index = self.index if planned else None
        self.r.generate_rays(self.cam, self.rng, index=index, rays=self.rays)
        out = self.r.trace_paths(self.rays, self.rng, self.iterations, schedule=schedule)
        self.r.accumulate_paths_linear_stats(out, self.linear, self.moments, index=index, params=self.params)
        if eight_bit:
            self.r.accumulate_paths_stats(out, self.film8, self.moments8, index=index)
        return out

    def plan(self, plan):
        self.r.plan_samples_linear(self.moments, self.P, self.params, plan, cdf=self.cdf, index=self.index, info=self.info)

    def plan8(self, plan):
        self.r.plan_samples(self.film8, self.moments8, self.P, plan, cdf=self.cdf, index=self.index, info=self.info)

    def resolve(self):
        self.r.resolve_linear(self.linear, params=self.params, linear=self.means, pixels=None, history=None)
        return self.means[:, :3].double()


def timing(results):
    cam = ptss.default_camera()
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    f = Film(r, W, H, cam, SEED)
    plan, plan8 = ptss.linear_plan_params(), ptss.plan_params()
    for _ in range(plan.minSamples):
        out = f.round(False, eight_bit=True)
    f.plan(plan)
    torch.cuda.synchronize()
    info = ptss.plan_info_dict(f.info.cpu().numpy())
    results["plan/info"] = info
    print(f"the moments of mixed after {plan.minSamples} uniform rounds: {info}", flush=True)
    index = f.index.clone()
    runs_of = torch.unique_consecutive(index, return_counts=True)[1]
    named = int(len(runs_of))
    results["sorted/index"] = {"pixels_named": named, "longest_run": int(runs_of.max()), "mean_run": float(runs_of.float().mean())}
    print(f"the plan's index names {named} pixels in runs of {float(runs_of.float().mean()):.2f} on average, {int(runs_of.max())} at most", flush=True)
    perm = torch.randperm(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)).to(torch.int32).contiguous()

    d_res = out.clone()   # the radiance of a real round
    linear0, moments0 = f.linear.clone(), f.moments.clone()
    linear, moments = f.linear, f.moments

    def reset():
        linear.copy_(linear0)
        moments.copy_(moments0)

    for what, idx, nbytes in (("identity", None, 144 * N), ("plan's index", index, 20 * N + 128 * named), ("permuted index", perm, 148 * N)):
        res = against_copy({"call": lambda: r.accumulate_paths_linear_stats(d_res, linear, moments, index=idx, params=f.params),
                            "plain": lambda: r.accumulate_paths_linear(d_res, linear, index=idx, params=f.params)}, nbytes, reset)
        results[f"accumulate/{what}"] = res
        show(f"accumulate_paths_linear_stats {what}", res, "accumulate_paths_linear")
    res = against_copy({"call": lambda: r.accumulate_paths_linear_stats(d_res, None, moments, index=index, params=f.params)}, 20 * N + 64 * named, reset)
    results["accumulate/plan's index, NULL film"] = res
    show("accumulate_paths_linear_stats plan's index, NULL film", res)
    reset()

    legs = {"call": lambda: f.plan(plan), "plain": lambda: f.plan8(plan8)}
    res = against_copy(legs, (32 + 12) * N)
    results["plan"] = res
    print(f"plan_samples_linear, n = width * height: {fmt(res['ms'])}, 44 B per pixel = {res['GB_per_s']:.0f} GB/s; a copy of those bytes "
          f"{fmt(res['copy_ms'])}; plan_samples (36 B per pixel) {fmt(res['plain_ms'])}: linear / 8-bit {res['call_over_plain']:.2f}", flush=True)

    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    f.plan(plan)

    def round_stats():
        r.generate_rays(f.cam, f.rng, index=f.index, rays=f.rays)
        o = r.trace_paths(f.rays, f.rng, f.iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear_stats(o, linear, moments, index=f.index, params=f.params)
        f.plan(plan)
        r.resolve_linear(linear, params=f.params, linear=f.means, pixels=d_px, history=d_hist)

    def round_linear():
        r.generate_rays(f.cam, f.rng, rays=f.rays)
        o = r.trace_paths(f.rays, f.rng, f.iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=f.params)
        r.resolve_linear(linear, params=f.params, linear=f.means, pixels=d_px, history=d_hist)

    t = timed_legs({"planned": round_stats, "linear": round_linear}, reset)
    t["planned_over_linear"] = t["planned"]["median"] / t["linear"]["median"]
    results["round"] = t
    print(f"round on mixed: generate(index), refill trace, accumulate with moments, plan, resolve {fmt(t['planned'])}; the linear round of "
          f"§3.29 {fmt(t['linear'])}: planned / linear {t['planned_over_linear']:.3f}", flush=True)
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
        truth = ref.resolve().clone()
        plan, plan8 = ptss.linear_plan_params(), ptss.plan_params()
        floor = float(plan.floor)
        uniform, relative, eight = Film(r, S, S, cam, SEED), Film(r, S, S, cam, SEED), Film(r, S, S, cam, SEED)
        for _ in range(32):
            uniform.round(False)
        for k in range(32):
            if k >= plan.minSamples:
                relative.plan(plan)
            relative.round(k >= plan.minSamples)
        for k in range(32):
            if k >= plan8.minSamples:
                eight.plan8(plan8)
            eight.round(k >= plan8.minSamples, eight_bit=True)
        relative.plan(plan)
        torch.cuda.synchronize()
        res = {"size": f"{S}x{S}", "reference_rounds": reference_rounds, "floor": floor, "final_info": ptss.plan_info_dict(relative.info.cpu().numpy())}
        for what, film in (("uniform_32", uniform), ("relative_plan_8_24", relative), ("eight_bit_plan_8_24", eight)):
            x = film.resolve()
            assert int((film.linear[:, 3] & 0xffffffff).sum()) == 32 * P
            res["mse_" + what] = float((x - truth).pow(2).mean())
            res["rel_mse_" + what] = float(((x - truth).pow(2) / (truth + floor).pow(2)).mean())
            res["samples_min_max_" + what] = [int((film.linear[:, 3] & 0xffffffff).min()), int((film.linear[:, 3] & 0xffffffff).max())]
        for what in ("relative_plan_8_24", "eight_bit_plan_8_24"):
            res["mse_ratio_" + what] = res["mse_" + what] / res["mse_uniform_32"]
            res["rel_mse_ratio_" + what] = res["rel_mse_" + what] / res["rel_mse_uniform_32"]
        results[f"quality/{name}"] = res
        print(f"quality {name} {S}x{S}, linear means against {reference_rounds} uniform rounds: MSE uniform {res['mse_uniform_32']:.6g}, relative plan "
              f"{res['mse_relative_plan_8_24']:.6g} (x {res['mse_ratio_relative_plan_8_24']:.3f}), 8-bit plan {res['mse_eight_bit_plan_8_24']:.6g} "
              f"(x {res['mse_ratio_eight_bit_plan_8_24']:.3f}); relative MSE uniform {res['rel_mse_uniform_32']:.6g}, relative plan "
              f"{res['rel_mse_relative_plan_8_24']:.6g} (x {res['rel_mse_ratio_relative_plan_8_24']:.3f}), 8-bit plan "
              f"{res['rel_mse_eight_bit_plan_8_24']:.6g} (x {res['rel_mse_ratio_eight_bit_plan_8_24']:.3f}); samples per pixel under the relative plan "
              f"{res['samples_min_max_relative_plan_8_24']}; final plan {res['final_info']}", flush=True)
        r.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("linstats_bench: no GPU (a measurement does not fall back)")
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
