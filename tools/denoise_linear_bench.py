"""tools/denoise_linear_bench.py [runs=5] [window_ms=50] [out.json] — what denoising a linear film costs and what it buys
(ptss_denoise_linear) on one GPU. Everything is reported, nothing is gated.

Times: 1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape,
`runs` windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  prepare      is not separable from a call's first pass from outside, so it is timed as the levels = 0 call: its <Final> instantiation,
               the same reads of the film and one 32-byte write in place of 36 bytes, without the reads of moments and features
               ("prepare_final"; "prepare_by_difference" is that call again, timed as the leg under level 0)
  level i      the call at levels = i + 1 with pass i staged against the same call with pass i from global memory, every earlier pass
               from global memory in both legs (ptss_debug_denoise_linear_form 4 + mask), so the two legs differ in pass i alone; the
               pass's own time is the call minus the call at one level less. Beside it ptss_denoise's level time in this process
               ((5 levels - 1 level) / 4 of ptss_denoise_history), and a device copy of the pass's algorithmic bytes: 36 B read and
               16 B written per pixel
  staged wins  at a spacing only if the staged leg is faster in every interleaved pair of windows
  call         the whole call at 5 levels in the shipped table of forms, all global, all staged
  round        generate + refill trace + accumulate with stats + meter + update + glare build + glare resolve on "mixed" against the
               same round with ptss_denoise_linear in front of the meter
Before anything is timed the forms' films are compared with each other byte for byte at 1080p (the tests compare them with the probe).

Image error: 640x360, "cornell" and "mixed", one run each at 4 and 16 samples per pixel against a film of 4,096 samples per pixel of
the same streams' continuation. Relative mean squared error of the linear means, mean over pixels and channels of (x - ref)^2 /
(ref^2 + 0.01): (a) unfiltered, (b) ptss_denoise_linear at its defaults; and on the display bytes, mean squared error over 0..255:
(a), (b) and (c) today's path, resolve -> ptss_denoise_history at its defaults. The glare pyramid's level 1 (default glare parameters,
threshold 1) against the reference's, relative mean squared error with 0.01 as well, with and without the filter in front. One run
each: this tells the size of the effect on these two scenes at these sample counts, not its spread over seeds, scenes or cameras."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
window_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 50.0
out_path = sys.argv[3] if len(sys.argv) > 3 else None
W, H = 1920, 1080
N = W * H
EW, EH = 640, 360
SEED = 0x5EED
MAX_CALLS = 2000
REFERENCE_SAMPLES = 4096


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed_legs(legs):
    """legs: name -> fn. Every leg warmed, then `runs` rounds in which the legs take turns, one window each -> per leg the windows."""
    calls = {}
    for name, fn in legs.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(5, min(MAX_CALLS, int(window_ms / max(window(fn, 5), 1e-4)) + 1))
    ms = {name: [] for name in legs}
    for _ in range(runs):
        for name, fn in legs.items():
            ms[name].append(window(fn, calls[name]))
    return ms


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "windows": list(v)}


def fmt(t):
    return f"{t['median']:.4f} ms [{t['min']:.4f}, {t['max']:.4f}]"


def rendered(r, scene_w, scene_h, rounds, film_cam, params, rng, rays, film, moments, iterations):
    for _ in range(rounds):
        r.generate_rays(film_cam, rng, rays=rays)
        out = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear_stats(out, film, moments, params=params)


def timing(results):
    cam = ptss.default_camera()
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    L = ptss.device_lib()
    iterations = int(r.cfg.maxIterations)
    film_cam = ptss.film_camera("pinhole", W, H, cam)
    params, meter = ptss.linear_params(), ptss.meter_params(rate=0.5)
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    features = r.ray_features(r.generate_rays(ptss.film_camera("pinhole", W, H, cam, jitter=0), rng, rays=rays))
    film = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    moments = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    clean = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    work = torch.zeros(ptss.denoise_linear_workspace(W, H), dtype=torch.uint8, device="cuda")
    rendered(r, W, H, 8, film_cam, params, rng, rays, film, moments, iterations)
    torch.cuda.synchronize()

    def call(levels, form, out=clean):
        d = ptss.denoise_linear_params(levels=levels)

        def run():
            r.debug_denoise_linear_form(form)
            r.denoise_linear(film, W, H, moments, features, params, d, out=out, workspace=work)
        return run

    # the forms write the same film
    films = {}
    for name, form in (("table", 0), ("global", 1), ("staged", 2)):
        out = torch.full((N, 4), -1, dtype=torch.int64, device="cuda")
        call(5, form, out)()
        torch.cuda.synchronize()
        films[name] = out.cpu().numpy().tobytes()
    if not (films["table"] == films["global"] == films["staged"]):
        raise SystemExit("denoise_linear_bench: the forms' films differ at 1080p")
    print("the table of forms, all passes from global memory and all passes staged write the same film at 5 levels", flush=True)

    # ptss_denoise's level time, in this process
    hist = torch.rand((N, 4), dtype=torch.float32, device="cuda") * 255.0
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_lin = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    r.resolve_linear(film, params=params, linear=d_lin, pixels=d_px, history=hist)   # the display values ptss_denoise_history filters
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def old(levels):
        p = ptss.default_denoise_params(levels=levels)
        return lambda: ptss._check(L.ptss_denoise_history(r._ctx, C.c_void_p(hist.data_ptr()), C.c_void_p(features.data_ptr()), C.byref(p),
                                                          C.c_void_p(d_px.data_ptr()), stream))

    pass_bytes = 52 * N
    src = torch.empty(pass_bytes // 8, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    ms = timed_legs({"old5": old(5), "old1": old(1), "copy": lambda: dst.copy_(src), "prepare": call(0, 1)})
    old_level = [(a - b) / 4 for a, b in zip(ms["old5"], ms["old1"])]
    results["ptss_denoise_level"] = stat(old_level)
    results["copy_of_a_pass"] = dict(stat(ms["copy"]), bytes=pass_bytes)
    results["prepare_final"] = stat(ms["prepare"])
    print(f"ptss_denoise: one level {fmt(stat(old_level))} (5 levels {fmt(stat(ms['old5']))}, 1 level {fmt(stat(ms['old1']))}); a device copy of a "
          f"pass's algorithmic bytes ({pass_bytes / 1e6:.1f} MB) {fmt(stat(ms['copy']))}; the levels = 0 call {fmt(stat(ms['prepare']))}", flush=True)

    # each level in both forms
    verdict = {}
    for i in range(6):
        legs = {"global": call(i + 1, 4), "below": call(i, 4)}
        if i < 3:
            legs["staged"] = call(i + 1, 4 + (1 << i))
        ms = timed_legs(legs)
        g = [a - b for a, b in zip(ms["global"], ms["below"])]
        res = {"spacing": 1 << i, "global_pass": stat(g), "global_call": stat(ms["global"])}
        line = f"level {i} (spacing {1 << i}): from global memory {fmt(stat(g))}"
        if i < 3:
            s = [a - b for a, b in zip(ms["staged"], ms["below"])]
            wins = all(a < b for a, b in zip(ms["staged"], ms["global"]))
            res.update(staged_pass=stat(s), staged_call=stat(ms["staged"]), staged_wins_every_pair=wins)
            verdict[1 << i] = wins
            line += f", staged {fmt(stat(s))}: staged {'wins every pair' if wins else 'does not win every pair'}"
        else:
            line += ", no staged kernel"
        if i == 0:
            results["prepare_by_difference"] = stat(ms["below"])   # the levels = 0 call is prepare <Final> alone
        results[f"level/{i}"] = res
        print(line, flush=True)
    results["staged_wins"] = verdict

    ms = timed_legs({"table": call(5, 0), "global": call(5, 1), "staged": call(5, 2)})
    results["call5"] = {k: stat(v) for k, v in ms.items()}
    print("the whole call at 5 levels: " + ", ".join(f"{k} {fmt(stat(v))}" for k, v in ms.items()), flush=True)
    r.debug_denoise_linear_form(0)

    # the round
    d_bins = torch.zeros(ptss.METER_BINS, dtype=torch.int32, device="cuda")
    d_state = torch.zeros(6, dtype=torch.int64, device="cuda")
    glare = ptss.glare_params(levels=6, threshold=0.5, strength=0.1)
    d_pyr = torch.zeros((ptss.glare_layout(W, H, 6)[1], 4), dtype=torch.int64, device="cuda")
    outs = dict(linear=d_lin, pixels=d_px, history=hist)
    denoise = ptss.denoise_linear_params()

    def round_of(filtered):
        def run():
            r.generate_rays(film_cam, rng, rays=rays)
            o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
            r.accumulate_paths_linear_stats(o, film, moments, params=params)
            shown = film
            if filtered:
                r.denoise_linear(film, W, H, moments, features, params, denoise, out=clean, workspace=work)
                shown = clean
            d_bins.zero_()
            r.meter_linear(shown, histogram=d_bins)
            r.meter_exposure(d_bins, d_state, params, meter)
            r.glare_build(shown, W, H, params, glare, "linear", d_pyr)
            r.resolve_linear(shown, params=params, metered=d_state, glare=(W, H, glare, d_pyr), **outs)
        return run

    ms = timed_legs({"denoised": round_of(True), "plain": round_of(False)})
    results["round"] = {k: stat(v) for k, v in ms.items()}
    results["round"]["denoised_over_plain"] = statistics.median(ms["denoised"]) / statistics.median(ms["plain"])
    print(f"round on mixed (generate, refill trace, accumulate with stats, [denoise,] meter, update, glare build, glare resolve): denoised "
          f"{fmt(stat(ms['denoised']))}, plain {fmt(stat(ms['plain']))}: ratio {results['round']['denoised_over_plain']:.3f}", flush=True)
    r.close()


def rel_mse(x, ref):
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


def means_of(film, params):
    w = film.view(np.uint64).reshape(-1, 4)
    n = np.maximum(w[:, 3] & np.uint64(0xffffffff), np.uint64(1)).astype(np.float64)
    return w[:, :3].astype(np.float64) / n[:, None] * 2.0 ** -params.scaleLog2


def errors(results):
    n = EW * EH
    params, denoise, glare = ptss.linear_params(), ptss.denoise_linear_params(), ptss.glare_params(threshold=1.0)
    level1 = ((EW + 1) // 2) * ((EH + 1) // 2)
    for scene in ("cornell", "mixed"):
        r = ptss.Renderer(ptss.Scene(scene), EW, EH, seed=SEED, sync_each_frame=False)
        iterations = int(r.cfg.maxIterations)
        cam = ptss.default_camera()
        film_cam = ptss.film_camera("pinhole", EW, EH, cam)
        rng = r.seed_path_rng(n, SEED, device=True)
        rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
        features = r.ray_features(r.generate_rays(ptss.film_camera("pinhole", EW, EH, cam, jitter=0), rng, rays=rays))
        film = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        moments = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        clean = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        d_pyr = torch.zeros((ptss.glare_layout(EW, EH, glare.levels)[1], 4), dtype=torch.int64, device="cuda")
        L = ptss.device_lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def shown(f):
            lin = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            px = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            hs = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
            r.resolve_linear(f, params=params, linear=lin, pixels=px, history=hs)
            r.glare_build(f, EW, EH, params, glare, "linear", d_pyr)
            torch.cuda.synchronize()
            pyr = d_pyr[:level1].cpu().numpy().view(np.uint64)[:, :3].astype(np.float64) * 2.0 ** -params.scaleLog2
            return means_of(f.cpu().numpy(), params), px.cpu().numpy()[:, :3].astype(np.float64), hs, pyr

        taken, at = 0, {}
        for spp in (4, 16, REFERENCE_SAMPLES):
            rendered(r, EW, EH, spp - taken, film_cam, params, rng, rays, film, moments, iterations)
            taken = spp
            if spp == REFERENCE_SAMPLES:
                at["ref"] = shown(film)
                break
            r.denoise_linear(film, EW, EH, moments, features, params, denoise, out=clean)
            raw, filtered = shown(film), shown(clean)
            old_px = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            p = ptss.default_denoise_params()
            ptss._check(L.ptss_denoise_history(r._ctx, C.c_void_p(raw[2].data_ptr()), C.c_void_p(features.data_ptr()), C.byref(p),
                                               C.c_void_p(old_px.data_ptr()), stream))
            torch.cuda.synchronize()
            at[spp] = (raw, filtered, old_px.cpu().numpy()[:, :3].astype(np.float64))
        ref = at["ref"]
        for spp in (4, 16):
            raw, filtered, old = at[spp]
            res = {"linear_relmse_unfiltered": rel_mse(raw[0], ref[0]), "linear_relmse_filtered": rel_mse(filtered[0], ref[0]),
                   "display_mse_unfiltered": float(np.mean((raw[1] - ref[1]) ** 2)), "display_mse_filtered": float(np.mean((filtered[1] - ref[1]) ** 2)),
                   "display_mse_ptss_denoise": float(np.mean((old - ref[1]) ** 2)),
                   "glare1_relmse_unfiltered": rel_mse(raw[3], ref[3]), "glare1_relmse_filtered": rel_mse(filtered[3], ref[3])}
            results[f"error/{scene}/{spp}"] = res
            print(f"{scene} at {spp} spp against {REFERENCE_SAMPLES}: " + ", ".join(f"{k} {v:.4g}" for k, v in res.items()), flush=True)
        r.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("denoise_linear_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    what = os.environ.get("PTSS_DENOISE_LINEAR_BENCH", "times,errors")
    if "times" in what:
        timing(results)
    if "errors" in what:
        errors(results)
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "error_size": f"{EW}x{EH}",
           "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
