"""tools/tone_bench.py [runs=5] [window_ms=50] [out.json] — what tone curves on a linear film cost (ptss_tone_build, ptss_resolve_toned;
DESIGN.md §3.37) on one GPU, and what they do to an image.

1920x1080, one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  forms        the two lookups (ptss_debug_tone_form 1: the table staged in LDS and a binary search; 2: a guess from the hardware log2 / exp2
               settled against the table in global memory) against each other, per bit depth and film kind, on the default curve
               (filmic, sRGB), three outputs; "every pair": whether one form was faster in every interleaved pair of windows
  resolve      the toned resolve (the shipped form) beside the plain, the metered and the glare resolve of the same film, and beside a device
               copy of its algorithmic bytes (32 B read, 36 B written per pixel)
  build        ptss_tone_build alone, 8 and 10 bits
  round        generate + refill trace + linear accumulate + meter + update + glare build + glare resolve on "mixed" (the glare round of
               tools/glare_bench.py) against the same round with the toned resolve in place of the glare resolve
  image        ONE RUN EACH, a statistic and not a timing: "mixed" and "cornell" at 640x360, 64 samples per pixel, auto-exposure and glare
               (default parameters), shown through the clamp, Reinhard and filmic, per channel and by luminance, 2.2 power, 8 bits: the share
               of pixels with a channel at level 255, and the count of distinct levels in use
Every form's output is compared with the host probe's (on a 64 x 48 corner of the film) before it is timed. No figure is fixed in advance.
Written to stdout and out.json."""
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
FORMS = {"staged": 1, "guess": 2}


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
    return {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "calls": calls[name], "windows": v} for name, v in ms.items()}


def fmt(t):
    return f"{t['median']:.4f} ms [{t['min']:.4f}, {t['max']:.4f}]"


def render(r, name_w, name_h, rounds, splat_too=True):
    """`rounds` samples per pixel of the renderer's scene into a linear film and its filtered twin, on the device."""
    n = name_w * name_h
    film_cam = ptss.film_camera("pinhole", name_w, name_h, ptss.default_camera())
    params = ptss.linear_params()
    rng = r.seed_path_rng(n, SEED, device=True)
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    pos = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    linear = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    filtered = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    iterations = int(r.cfg.maxIterations)
    for _ in range(rounds):
        r.generate_rays(film_cam, rng, rays=rays, positions=pos)
        out = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
        r.accumulate_paths_linear(out, linear, params=params)
        if splat_too:
            r.splat_paths(out, pos, filtered, name_w, name_h, params=params, homed_first_pixel=0)
    torch.cuda.synchronize()
    return film_cam, params, rng, rays, linear, filtered


def main():
    if not torch.cuda.is_available():
        raise SystemExit("tone_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film_cam, params, rng, rays, linear, filtered = render(r, W, H, 8)
    meter = ptss.meter_params(rate=0.5)
    d_px = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
    d_hist = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    d_means = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    d_bins = torch.zeros(ptss.METER_BINS, dtype=torch.int32, device="cuda")
    d_state = torch.zeros(6, dtype=torch.int64, device="cuda")
    glare = ptss.glare_params(levels=6, threshold=0.5, strength=0.1)
    entries = ptss.glare_layout(W, H, 6)[1]
    d_pyr = torch.zeros((entries, 4), dtype=torch.int64, device="cuda")
    films = {"linear": (linear, r.resolve_linear), "splat": (filtered, r.resolve_splat)}
    outs = dict(linear=d_means, pixels=d_px, history=d_hist)
    r.meter_linear(linear, histogram=d_bins)   # a state that holds the film's own exposure: the float steps see real values
    r.meter_exposure(d_bins, d_state, params, meter)
    tones, tables = {}, {}
    for bits in (8, 10):
        tones[bits] = ptss.tone_params(bits=bits)
        tables[bits] = torch.zeros(ptss.tone_table_floats(bits), dtype=torch.float32, device="cuda")
        r.tone_build(tones[bits], tables[bits])
        torch.cuda.synchronize()
        if tables[bits].cpu().numpy().view(np.uint32).tobytes() != ptss.probe_tone_build(tones[bits]).view(np.uint32).tobytes():
            raise SystemExit(f"tone_bench: the device's table at {bits} bits differs from the probe's")

    # every form writes the probe's bytes (a 64 x 48 corner: the probe counts K comparisons per channel)
    corner = 64 * 48
    state_host = d_state.cpu().numpy().view(ptss.METER_STATE_DTYPE)
    for kind, (film, call) in films.items():
        host = film[:corner].cpu().numpy().view(np.uint64)
        for bits in (8, 10):
            want = ptss.probe_resolve_toned(host, tones[bits], tables[bits].cpu().numpy(), params=params, state=state_host, film_kind=kind)
            for name, form in FORMS.items():
                r.debug_tone_form(form)
                call(film, count=corner, params=params, metered=d_state, tone=(tones[bits], tables[bits]), **outs)
                torch.cuda.synchronize()
                got = (d_means[:corner].cpu().numpy(), d_px[:corner].cpu().numpy(), d_hist[:corner].cpu().numpy())
                if any(a.tobytes() != np.ascontiguousarray(b).tobytes() for a, b in zip(got, want)):
                    raise SystemExit(f"tone_bench: form {name} on the {kind} film at {bits} bits differs from the probe")
    r.debug_tone_form(0)
    print("both forms write the host probe's bytes on both films at 8 and 10 bits", flush=True)

    def toned(kind, bits, form, **kw):
        film, call = films[kind]

        def run():
            r.debug_tone_form(form)
            call(film, params=params, tone=(tones[bits], tables[bits]), **kw, **outs)
        return run

    for kind in films:
        for bits in (8, 10):
            t = timed_legs({name: toned(kind, bits, form, metered=d_state) for name, form in FORMS.items()})
            pairs = list(zip(t["staged"]["windows"], t["guess"]["windows"]))
            every = "staged" if all(a < b for a, b in pairs) else "guess" if all(b < a for a, b in pairs) else "neither"
            t["faster_in_every_pair"] = every
            t["staged_over_guess"] = t["staged"]["median"] / t["guess"]["median"]
            results[f"forms/{kind}/{bits}"] = t
            print(f"forms on the {kind} film at {bits} bits, metered, three outputs: staged {fmt(t['staged'])}, guess {fmt(t['guess'])}: staged / guess "
                  f"{t['staged_over_guess']:.3f}; faster in every pair: {every}", flush=True)

    nbytes = 68 * N
    src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")   # a copy of those bytes: half read, half written
    dst = torch.empty_like(src)
    for kind, (film, call) in films.items():
        r.glare_build(film, W, H, params, glare, kind, d_pyr)
        g = (W, H, glare, d_pyr)
        legs = {"toned 8": toned(kind, 8, 0), "toned 10": toned(kind, 10, 0), "toned 8 metered": toned(kind, 8, 0, metered=d_state),
                "toned 8 glare": toned(kind, 8, 0, metered=d_state, glare=g), "plain": lambda: call(film, params=params, **outs),
                "metered": lambda: call(film, params=params, metered=d_state, **outs),
                "glare": lambda: call(film, params=params, metered=d_state, glare=g, **outs), "copy": lambda: dst.copy_(src)}
        t = timed_legs(legs)
        t["toned_over_plain"] = t["toned 8"]["median"] / t["plain"]["median"]
        t["toned_metered_over_metered"] = t["toned 8 metered"]["median"] / t["metered"]["median"]
        t["toned_glare_over_glare"] = t["toned 8 glare"]["median"] / t["glare"]["median"]
        t["toned_GB_per_s"] = nbytes / t["toned 8"]["median"] / 1e6
        t["copy_GB_per_s"] = nbytes / t["copy"]["median"] / 1e6
        results[f"resolve/{kind}"] = t
        print(f"resolve of the {kind} film, three outputs ({nbytes / 1e6:.1f} MB): toned 8 bits {fmt(t['toned 8'])} = {t['toned_GB_per_s']:.0f} GB/s, 10 bits "
              f"{fmt(t['toned 10'])}, plain {fmt(t['plain'])} (toned / plain {t['toned_over_plain']:.3f}); metered: toned {fmt(t['toned 8 metered'])}, "
              f"plain {fmt(t['metered'])} ({t['toned_metered_over_metered']:.3f}); glare: toned {fmt(t['toned 8 glare'])}, plain {fmt(t['glare'])} "
              f"({t['toned_glare_over_glare']:.3f}); a copy of those bytes {fmt(t['copy'])} = {t['copy_GB_per_s']:.0f} GB/s", flush=True)
    del src, dst

    t = timed_legs({f"build {bits}": (lambda b=bits: r.tone_build(tones[b], tables[b])) for bits in (8, 10)})
    results["build"] = t
    print(f"tone_build alone: 8 bits {fmt(t['build 8'])}, 10 bits {fmt(t['build 10'])}", flush=True)

    def round_with(resolve):
        def run():
            r.generate_rays(film_cam, rng, rays=rays)
            o = r.trace_paths(rays, rng, iterations, schedule=ptss.PATHS_REFILL)
            r.accumulate_paths_linear(o, linear, params=params)
            d_bins.zero_()
            r.meter_linear(linear, histogram=d_bins)
            r.meter_exposure(d_bins, d_state, params, meter)
            r.glare_build(linear, W, H, params, glare, "linear", d_pyr)
            resolve()
        return run

    g = (W, H, glare, d_pyr)
    t = timed_legs({"toned": round_with(lambda: r.resolve_linear(linear, params=params, metered=d_state, glare=g, tone=(tones[8], tables[8]), **outs)),
                    "glare": round_with(lambda: r.resolve_linear(linear, params=params, metered=d_state, glare=g, **outs))})
    t["toned_over_glare"] = t["toned"]["median"] / t["glare"]["median"]
    results["round"] = t
    print(f"round on mixed (generate, refill trace, accumulate, zero, meter, update, glare build, resolve): toned {fmt(t['toned'])}, glare "
          f"{fmt(t['glare'])}: toned / glare {t['toned_over_glare']:.3f}", flush=True)
    r.close()

    # the image statistic: one run each
    sw, sh, spp = 640, 360, 64
    for scene in ("mixed", "cornell"):
        s = ptss.Renderer(ptss.Scene(scene), sw, sh, seed=SEED, sync_each_frame=False)
        _, sparams, _, _, film, _ = render(s, sw, sh, spp, splat_too=False)
        n = sw * sh
        bins = torch.zeros(ptss.METER_BINS, dtype=torch.int32, device="cuda")
        state = torch.zeros(6, dtype=torch.int64, device="cuda")
        s.meter_linear(film, histogram=bins)
        s.meter_exposure(bins, state, sparams, ptss.meter_params())
        sglare = ptss.glare_params()
        pyr = torch.zeros((ptss.glare_layout(sw, sh, sglare.levels)[1], 4), dtype=torch.int64, device="cuda")
        s.glare_build(film, sw, sh, sparams, sglare, "linear", pyr)
        px = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
        for curve in ("clamp", "reinhard", "filmic"):
            for luminance in (False, True):
                tone = ptss.tone_params(curve, "gamma22", 8, luminance)
                table = torch.zeros(ptss.tone_table_floats(8), dtype=torch.float32, device="cuda")
                s.tone_build(tone, table)
                s.resolve_linear(film, params=sparams, metered=state, glare=(sw, sh, sglare, pyr), linear=None, pixels=px, history=None, tone=(tone, table))
                torch.cuda.synchronize()
                rgb = px.cpu().numpy()[:, :3]
                share, distinct = float((rgb == 255).any(axis=1).mean()), int(len(np.unique(rgb)))
                results[f"image/{scene}/{curve}/{'luminance' if luminance else 'channel'}"] = {"share_at_top": share, "distinct_levels": distinct}
                print(f"image {scene} {sw}x{sh} {spp} spp, auto-exposure and glare, {curve} {'by luminance' if luminance else 'per channel'}: "
                      f"{100 * share:.2f} % of pixels with a channel at 255, {distinct} distinct levels (one run)", flush=True)
        s.close()
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "size": f"{W}x{H}", "device": torch.cuda.get_device_name(0),
           "library": os.environ.get("PTSS_LIBNAME", "libptss.so"), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
