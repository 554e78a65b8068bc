"""tools/glare_bench.py [runs=5] [window_ms=50] [out.json] — what glare on a linear film costs (ptss_glare_build,
ptss_resolve_linear_glare, ptss_resolve_splat_glare) on one GPU.

1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  build        ptss_glare_build at 1, 4 and 8 levels on a rendered "mixed" film and on its filtered twin, against a device copy of its
               algorithmic bytes: the film read once (32 B per pixel), every level written once as d_k, read once by the level above,
               read and written once more where it becomes u_k, and read once by the level below (the resolve's read of u_1 is the
               resolve's). The copy reads half of those bytes and writes half
  reduce       the tiled reduce (one level: the reduce is the whole build) against the untiled form, which divides every film pixel
               for each of the four texels that read it
  tail         all small levels in one single-workgroup launch against one launch per level and direction
               The untiled reduce and the form without a tail exist in the measurement build only: run with PTSS_LIBNAME=libptss_knobs.so
               (tools/build_variants.py knobs), which reads PTSS_GLARE_UNTILED and PTSS_GLARE_TAIL at every build; the shipped library
               times the kept forms only
  resolve      each glare resolve beside its plain sibling, three outputs
  round        generate + refill trace + linear accumulate + meter + update + metered resolve on "mixed" (the metered round of
               tools/meter_bench.py) against the same round with build + glare resolve in place of the metered resolve
Every form's pyramid is compared with the host probe's before it is timed. No figure is fixed in advance. Written to stdout and out.json."""
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
LEVELS = (1, 4, 8)


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


def with_env(env, fn):
    """fn with the measurement build's switches set as it reads them (at every build); the shipped library ignores them."""
    def run():
        for k, v in env.items():
            os.environ[k] = v
        fn()
    return run


def algorithmic_bytes(levels):
    sizes = [w * h for w, h, _ in ptss.glare_layout(W, H, levels)[0]]
    total = 32 * N
    for k, n in enumerate(sizes, start=1):
        touches = 1 + (3 if k < levels else 0) + (1 if k > 1 else 0)   # d_k written; read by the down, read and written as u_k; read by the up below
        total += 32 * n * touches
    return total


def main():
    if not torch.cuda.is_available():
        raise SystemExit("glare_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {"knobs": KNOBS}
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
    d_pyr = torch.zeros((ptss.glare_layout(W, H, 8)[1], 4), dtype=torch.int64, device="cuda")

    for _ in range(8):   # the rendered films: eight rounds of "mixed" into the linear film and into its filtered twin
        r.generate_rays(film_cam, rng, rays=rays, positions=pos)
        out = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(out, linear, params=params)
        r.splat_paths(out, pos, filtered, W, H, params=params, homed_first_pixel=0)
    torch.cuda.synchronize()
    films = {"linear": linear, "splat": filtered}
    forms = {"kept": {}}
    if KNOBS:
        forms = {"kept": {"PTSS_GLARE_TAIL": "1", "PTSS_GLARE_UNTILED": "0"}, "no tail": {"PTSS_GLARE_TAIL": "0", "PTSS_GLARE_UNTILED": "0"},
                 "untiled": {"PTSS_GLARE_TAIL": "1", "PTSS_GLARE_UNTILED": "1"}}

    def build(kind, levels, threshold=0.5):
        glare = ptss.glare_params(levels=levels, threshold=threshold)
        entries = ptss.glare_layout(W, H, levels)[1]
        return lambda: r.glare_build(films[kind], W, H, params, glare, kind, d_pyr[:entries])

    # every form writes the probe's bytes
    for kind, film in films.items():
        host = film.cpu().numpy().view(np.uint64)
        for levels in LEVELS:
            want = ptss.probe_glare_build(host, W, H, params, ptss.glare_params(levels=levels, threshold=0.5), film_kind=kind)
            for name, env in forms.items():
                d_pyr.fill_(-1)
                before = r.glare_launches()
                with_env(env, build(kind, levels))()
                torch.cuda.synchronize()
                after = r.glare_launches()
                got = d_pyr[:len(want)].cpu().numpy().view(np.uint64)
                if got.tobytes() != want.tobytes():
                    raise SystemExit(f"glare_bench: form {name} on the {kind} film at {levels} levels differs from the probe")
                results[f"launches/{kind}/{levels}/{name}"] = after[1] - before[1]
        results[f"lit/{kind}"] = int((want.view(np.uint64).reshape(-1, 4)[:, :3] != 0).any(axis=1).sum())
    print("every form's pyramid equals the host probe's on both films at 1, 4 and 8 levels; kernels per build:",
          {k: v for k, v in results.items() if k.startswith("launches/linear")}, flush=True)

    for kind in films:
        for levels in LEVELS:
            nbytes = algorithmic_bytes(levels)
            src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")   # a copy of those bytes: half read, half written
            dst = torch.empty_like(src)
            legs = {name: with_env(env, build(kind, levels)) for name, env in forms.items() if not (name == "no tail" and levels == 1)}
            legs["copy"] = lambda: dst.copy_(src)
            t = timed_legs(legs)
            res = {"bytes": nbytes, "copy_ms": t["copy"], "copy_GB_per_s": nbytes / t["copy"]["median"] / 1e6}
            line = f"glare_build on the {kind} film, {levels} levels ({nbytes / 1e6:.1f} MB):"
            for name in legs:
                if name == "copy":
                    continue
                res[name] = {"ms": t[name], "GB_per_s": nbytes / t[name]["median"] / 1e6, "rate_over_copy": t["copy"]["median"] / t[name]["median"]}
                line += f" {name} {fmt(t[name])} = {res[name]['GB_per_s']:.0f} GB/s ({res[name]['rate_over_copy']:.2f} of the copy's rate);"
            print(line + f" a copy of those bytes {fmt(t['copy'])} = {res['copy_GB_per_s']:.0f} GB/s", flush=True)
            results[f"build/{kind}/{levels}"] = res
            del src, dst
    for k in ("PTSS_GLARE_TAIL", "PTSS_GLARE_UNTILED"):
        os.environ.pop(k, None)   # from here on: the kept forms

    r.meter_linear(linear, histogram=d_bins)   # a state that holds the film's own exposure: the resolves' float steps see real values
    r.meter_exposure(d_bins, d_state, params, meter)
    outs = dict(linear=d_means, pixels=d_px, history=d_hist)
    glare = ptss.glare_params(levels=6, threshold=0.5, strength=0.1)
    entries = ptss.glare_layout(W, H, 6)[1]
    for kind, call in (("linear", r.resolve_linear), ("splat", r.resolve_splat)):
        film = films[kind]
        r.glare_build(film, W, H, params, glare, kind, d_pyr[:entries])
        t = timed_legs({"glare": lambda: call(film, params=params, glare=(W, H, glare, d_pyr[:entries]), **outs),
                        "glare with a state": lambda: call(film, params=params, metered=d_state, glare=(W, H, glare, d_pyr[:entries]), **outs),
                        "plain": lambda: call(film, params=params, **outs)})
        t["glare_over_plain"] = t["glare"]["median"] / t["plain"]["median"]
        results[f"resolve/{kind}"] = t
        print(f"resolve_{kind}, three outputs: glare {fmt(t['glare'])}, with a state {fmt(t['glare with a state'])}, plain {fmt(t['plain'])}: "
              f"glare / plain {t['glare_over_plain']:.3f}", flush=True)
        b = timed_legs({"build": lambda: r.glare_build(film, W, H, params, glare, kind, d_pyr[:entries])})
        results[f"build6/{kind}"] = b["build"]
        print(f"glare_build on the {kind} film, 6 levels (the default): {fmt(b['build'])}", flush=True)

    def round_metered():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=params)
        d_bins.zero_()
        r.meter_linear(linear, histogram=d_bins)
        r.meter_exposure(d_bins, d_state, params, meter)
        r.resolve_linear(linear, params=params, metered=d_state, **outs)

    def round_glare():
        r.generate_rays(film_cam, rng, rays=rays)
        o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(o, linear, params=params)
        d_bins.zero_()
        r.meter_linear(linear, histogram=d_bins)
        r.meter_exposure(d_bins, d_state, params, meter)
        r.glare_build(linear, W, H, params, glare, "linear", d_pyr[:entries])
        r.resolve_linear(linear, params=params, metered=d_state, glare=(W, H, glare, d_pyr[:entries]), **outs)

    t = timed_legs({"glare": round_glare, "metered": round_metered})
    t["glare_over_metered"] = t["glare"]["median"] / t["metered"]["median"]
    results["round"] = t
    print(f"round on mixed (generate, refill trace, accumulate, zero, meter, update, [build,] resolve): with glare {fmt(t['glare'])}, metered "
          f"{fmt(t['metered'])}: glare / metered {t['glare_over_metered']:.3f}", flush=True)
    r.close()
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0),
           "library": os.environ.get("PTSS_LIBNAME", "libptss.so"), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
