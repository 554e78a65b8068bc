"""tools/meter_bench.py [runs=5] [window_ms=50] [out.json] — what metering a linear film costs (ptss_meter_linear, ptss_meter_splat,
ptss_meter_exposure, ptss_resolve_linear_metered, ptss_resolve_splat_metered) on one GPU.

1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  histogram    each form of the LDS step (a: one LDS atomic per lane, b: runs of one bin summed first, c: a loop over the wave's distinct
               bins) on three films — a rendered "mixed" film, a film with every pixel in one bin, a film with 64 different bins in every
               64 pixels — against a device copy of the algorithmic bytes (32 B per pixel read; the copy reads half and writes half). The
               three forms exist in the measurement build only: run with PTSS_LIBNAME=libptss_knobs.so (tools/build_variants.py knobs),
               which reads PTSS_METER_FORM at every launch; with the shipped library only the kept form is timed. ptss_meter_splat on
               the filtered twin of the rendered film, the kept form. In the measurement build also the kept form under grid caps of 64 to
               2048 workgroups (PTSS_METER_GRID_CAP)
  exposure     ptss_meter_exposure, one update
  resolve      each metered resolve beside its plain sibling, three outputs (32 B read, 36 B written)
  round        generate + refill trace + linear accumulate + resolve on "mixed" (the linear round of tools/linear_bench.py) against the
               same round with meter + update + metered resolve, the histogram zeroed on the stream
Every form's histogram is compared with the host probe's before it is timed. No figure is fixed in advance. Written to stdout and out.json."""
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
SEED = 0x5EED
MAX_CALLS = 2000
KNOBS = "knobs" in os.environ.get("PTSS_LIBNAME", "")
FORMS = {"a": "0", "b": "1", "c": "2"} if KNOBS else {"kept": None}


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed_legs(legs):
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
            ms[name].append(window(fn, calls[name]))
    return {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "calls": calls[name]} for name, v in ms.items()}


def fmt(t):
    return f"{t['median']:.4f} ms [{t['min']:.4f}, {t['max']:.4f}]"


def with_form(form, fn):
    """fn with PTSS_METER_FORM set as the measurement build reads it (at every launch); the shipped library ignores it."""
    def run():
        if form is not None:
            os.environ["PTSS_METER_FORM"] = form
        fn()
    return run


def bin_film(bins):
    """A linear film on the device whose pixel i lands in bin bins[i] (e >= 3): grey, one sample."""
    b = np.asarray(bins, dtype=np.int64) - 1
    Y = ((8 + b % 8) << (b // 8)) >> 3
    rows = np.zeros((len(b), 4), dtype=np.int64)
    rows[:, 0] = rows[:, 1] = rows[:, 2] = Y
    rows[:, 3] = 1
    return torch.from_numpy(rows).cuda()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("meter_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {"forms": list(FORMS)}
    cam = ptss.default_camera()
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film_cam = ptss.film_camera("pinhole", W, H, cam)
    params, meter = ptss.linear_params(), ptss.meter_params(rate=0.5)
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    pos = torch.zeros((N, 2), dtype=torch.float32, device="cuda")
    linear = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    filtered = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    d_means = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    d_bins = torch.zeros(ptss.METER_BINS, dtype=torch.int32, device="cuda")
    d_state = torch.zeros(6, dtype=torch.int64, device="cuda")

    for _ in range(8):   # the rendered films: eight rounds of "mixed" into the linear film and into its filtered twin
        r.generate_rays(film_cam, rng, rays=rays, positions=pos)
        out = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(out, linear, params=params)
        r.splat_paths(out, pos, filtered, W, H, params=params, homed_first_pixel=0)
    torch.cuda.synchronize()
    films = {"mixed": linear, "one bin": bin_film(np.full(N, 137)), "64 bins per wave": bin_film(30 + 4 * (np.arange(N) % 64) + (np.arange(N) // 64) % 4)}

    # every form writes the probe's bytes
    for what, film in films.items():
        want = ptss.probe_meter_linear(film.cpu().numpy().view(np.uint64))
        for name, form in FORMS.items():
            d_bins.zero_()
            with_form(form, lambda: r.meter_linear(film, histogram=d_bins))()
            torch.cuda.synchronize()
            if not np.array_equal(d_bins.cpu().numpy().view(np.uint32), want):
                raise SystemExit(f"meter_bench: form {name} on {what} differs from the probe")
        results[f"histogram/{what}/bins_used"] = int(np.count_nonzero(want))
    print("every form's histogram equals the host probe's on the three films", flush=True)

    src = torch.empty(32 * N // 8, dtype=torch.int32, device="cuda")   # a copy of 32 B per pixel: half read, half written
    dst = torch.empty_like(src)
    for what, film in films.items():
        legs = {name: with_form(form, lambda film=film: r.meter_linear(film, histogram=d_bins)) for name, form in FORMS.items()}
        legs["copy"] = lambda: dst.copy_(src)
        t = timed_legs(legs)
        res = {"bytes": 32 * N, "copy_ms": t["copy"], "copy_GB_per_s": 32 * N / t["copy"]["median"] / 1e6}
        line = f"meter_linear on {what}:"
        for name in FORMS:
            res[name] = {"ms": t[name], "GB_per_s": 32 * N / t[name]["median"] / 1e6, "rate_over_copy": t["copy"]["median"] / t[name]["median"]}
            line += f" {name} {fmt(t[name])} = {res[name]['GB_per_s']:.0f} GB/s ({res[name]['rate_over_copy']:.2f} of the copy's rate);"
        print(line + f" a copy of those bytes {fmt(t['copy'])} = {res['copy_GB_per_s']:.0f} GB/s", flush=True)
        results[f"histogram/{what}"] = res
    os.environ.pop("PTSS_METER_FORM", None)   # from here on: the kept form
    if KNOBS:   # the grid cap of the kept form (the measurement build reads PTSS_METER_GRID_CAP at every launch; 2025 workgroups of 1024 cover 1080p)
        def capped(cap, film):
            def run():
                os.environ["PTSS_METER_GRID_CAP"] = str(cap)
                r.meter_linear(film, histogram=d_bins)
            return run
        for what, film in films.items():
            t = timed_legs({str(cap): capped(cap, film) for cap in (64, 128, 256, 512, 1024, 2048)})
            results[f"grid cap/{what}"] = t
            print(f"meter_linear on {what}, workgroups at most: " + "; ".join(f"{cap} {fmt(v)}" for cap, v in t.items()), flush=True)
        os.environ.pop("PTSS_METER_GRID_CAP", None)

    t = timed_legs({"splat": lambda: r.meter_splat(filtered, histogram=d_bins), "linear": lambda: r.meter_linear(linear, histogram=d_bins)})
    results["histogram/filtered"] = t
    print(f"meter_splat on the filtered mixed film {fmt(t['splat'])}; meter_linear beside it {fmt(t['linear'])}", flush=True)

    d_bins.zero_()
    r.meter_linear(linear, histogram=d_bins)
    t = timed_legs({"exposure": lambda: r.meter_exposure(d_bins, d_state, params, meter)})
    results["exposure"] = t["exposure"]
    print(f"meter_exposure: {fmt(t['exposure'])}", flush=True)

    outs = dict(linear=d_means, pixels=d_px, history=d_hist)
    for what, film, call in (("linear", linear, r.resolve_linear), ("splat", filtered, r.resolve_splat)):
        t = timed_legs({"metered": lambda: call(film, params=params, metered=d_state, **outs), "plain": lambda: call(film, params=params, **outs)})
        t["metered_over_plain"] = t["metered"]["median"] / t["plain"]["median"]
        results[f"resolve/{what}"] = t
        print(f"resolve_{what}, three outputs (68 B per pixel): metered {fmt(t['metered'])}, plain {fmt(t['plain'])}: metered / plain {t['metered_over_plain']:.3f}", flush=True)

    def round_plain():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=params)
        r.resolve_linear(linear, params=params, **outs)

    def round_metered():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=params)
        d_bins.zero_()
        r.meter_linear(linear, histogram=d_bins)
        r.meter_exposure(d_bins, d_state, params, meter)
        r.resolve_linear(linear, params=params, metered=d_state, **outs)

    t = timed_legs({"metered": round_metered, "plain": round_plain})
    t["metered_over_plain"] = t["metered"]["median"] / t["plain"]["median"]
    results["round"] = t
    print(f"round on mixed (generate, refill trace, accumulate, [zero, meter, update,] resolve): metered {fmt(t['metered'])}, plain {fmt(t['plain'])}: "
          f"metered / plain {t['metered_over_plain']:.3f}", flush=True)
    state = d_state.cpu().numpy().view(ptss.METER_STATE_DTYPE)[0]
    results["final_state"] = {k: (float(state[k]) if state[k].dtype.kind == "f" else int(state[k])) for k in state.dtype.names}
    print("the meter's state after the rounds:", results["final_state"], flush=True)
    r.close()
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0),
           "library": os.environ.get("PTSS_LIBNAME", "libptss.so"), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
