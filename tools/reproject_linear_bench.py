#!/usr/bin/env python3
"""tools/reproject_linear_bench.py [runs] [window_ms] [out.json] — ptss_reproject_linear at 1080p on `mixed` after a 'w', 'd', 'f' move
(DESIGN.md §3.35): the call on the linear and on the filtered film, with and without moments, interleaved in one process with
ptss_reproject on the context's accumulator (the same two poses, the same features) and with a device copy of each form's algorithmic
bytes; and the first round after the move into the seeded film beside a plain round.
Every figure is the median over `runs` windows of about `window_ms` of back-to-back launches between two events (the rules of the
other tools here: warm up first, interleave what is compared, report the spread).

Algorithmic bytes per pixel: the feature row of the new pose (32), per counting tap of the previous pose the material word, the
geometry row, the film entry (4 + 16 + 32) and with moments the moment row (32), written the film row (32) and with moments the moment
row (32). With four taps of which neighbours share all but one column and one row, the previous pose's rows are read about once per
pixel: 32 + 32 + 32 + 32 = 128 B without moments, 192 B with."""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
import ptss   # noqa: E402
import torch  # noqa: E402

W, H = 1920, 1080
N = W * H
BOUNCES = 4


def moved(cam, keys):
    out = ptss.Camera()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(ptss.Camera))
    for k in keys:
        assert ptss.move_camera(out, k)
    return out


def window(fn, ms):
    """ms per call of fn over a window of about `ms` milliseconds of back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    reps = max(3, int(ms / max(a.elapsed_time(b), 1e-3)))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def pairs(legs, runs, ms):
    """The legs measured in turn, `runs` times over: {name: (median ms, min, max)}."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in legs}
    for _ in range(runs):
        for k, fn in legs.items():
            seen[k].append(window(fn, ms))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in seen.items()}


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    ms = float(sys.argv[2]) if len(sys.argv) > 2 else 50.0
    out_path = sys.argv[3] if len(sys.argv) > 3 else None
    seed = 0xABCDEF
    r = ptss.Renderer(ptss.Scene("mixed"), W, H, max_iterations=BOUNCES, seed=seed)
    dev = torch.device("cuda")
    params, reproject = ptss.linear_params(), ptss.reproject_linear_params()
    cam_a = moved(ptss.default_camera(), "w")
    cam_b = moved(cam_a, "df")
    centre = {k: ptss.film_camera("pinhole", W, H, c, jitter=0) for k, c in (("a", cam_a), ("b", cam_b))}
    film_cam = {k: ptss.film_camera("pinhole", W, H, c, jitter=1) for k, c in (("a", cam_a), ("b", cam_b))}
    rng = r.seed_path_rng(N, seed, device=True)
    rays = torch.empty((N, 8), dtype=torch.float32, device=dev)
    features = {}
    for k in ("a", "b"):
        r.generate_rays(centre[k], rng, rays=rays)
        features[k] = r.ray_features(rays).clone()
    flt = ptss.splat_filter("tent", 1.0)
    film = {kind: torch.zeros((N, 4), dtype=torch.int64, device=dev) for kind in ("linear", "splat")}
    moments = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    pos = torch.empty((N, 2), dtype=torch.float32, device=dev)

    def one_round(cam, linear, mom):
        r.generate_rays(cam, rng, rays=rays, positions=pos)
        res = r.trace_paths(rays, rng, BOUNCES)
        r.accumulate_paths_linear_stats(res, linear, mom, params=params)
        return res

    for _ in range(8):   # the history: eight rounds at pose A into both films
        res = one_round(film_cam["a"], film["linear"], moments)
        r.splat_paths(res, pos, film["splat"], W, H, filter=flt, params=params, homed_first_pixel=0)
    out = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    mout = torch.zeros((N, 4), dtype=torch.int64, device=dev)
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    src = {b: torch.empty(b * N // 2, dtype=torch.uint8, device=dev) for b in (128, 192)}
    dst = {b: torch.empty_like(src[b]) for b in src}

    def call(kind, with_moments):
        r.reproject_linear(centre["b"], features["b"], centre["a"], features["a"], film[kind], moments if with_moments else None, params, reproject,
                           film_kind=kind, out=out, moments_out=mout if with_moments else None, info=None)

    legs = {}
    for kind in ("linear", "splat"):
        for with_moments in (True, False):
            legs[f"reproject_linear {kind}{' + moments' if with_moments else ''}"] = (lambda k=kind, m=with_moments: call(k, m))
    # ptss_reproject between the same two poses on this context's own accumulator and features (tools/reproject_bench.py's setup)
    L = ptss.device_lib()
    r.set_camera(cam_a)
    for _ in range(4):
        r.generate_frame()
    d_fa, d_ha, d_hb = (r._device_buffer(name, N * size) for name, size in (("features_a", 32), ("history_a", 16), ("history_b", 16)))
    d_fb = r.features_devptr()
    rp = ptss.default_reproject_params()
    ptss._check(L.ptss_render_features(r._ctx, d_fa, None))
    ptss._check(L.ptss_reproject(r._ctx, d_fa, None, None, None, C.byref(rp), d_ha, None))
    r.set_camera(cam_b)
    r.generate_frame()
    ptss._check(L.ptss_render_features(r._ctx, d_fb, None))
    r.synchronize()
    legs["ptss_reproject (display history, 108 B per pixel)"] = lambda: ptss._check(
        L.ptss_reproject(r._ctx, d_fb, C.byref(cam_a), d_fa, d_ha, C.byref(rp), d_hb, None))
    legs["device copy of 128 B per pixel"] = lambda: dst[128].copy_(src[128])
    legs["device copy of 192 B per pixel"] = lambda: dst[192].copy_(src[192])
    result = {"size": [W, H], "runs": runs, "window_ms": ms, "legs": pairs(legs, runs, ms)}
    info.zero_()
    r.reproject_linear(centre["b"], features["b"], centre["a"], features["a"], film["linear"], moments, params, reproject, film_kind="linear", out=out,
                       moments_out=mout, info=info)
    torch.cuda.synchronize()
    result["info"] = dict(zip(("seeded", "offFilm", "noTap", "noVariance"), (int(v) for v in info.cpu())))
    empty, empty_m = torch.zeros_like(out), torch.zeros_like(mout)
    rounds = {"a round at B into the seeded film": lambda: one_round(film_cam["b"], out, mout),
              "a round at B into an empty film": lambda: one_round(film_cam["b"], empty, empty_m)}
    result["rounds"] = pairs(rounds, runs, ms)
    for group in ("legs", "rounds"):
        for k, (med, lo, hi) in result[group].items():
            print(f"{k:48s} {med:8.4f} ms  (min {lo:.4f}, max {hi:.4f})")
    print("info", result["info"])
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    r.close()


if __name__ == "__main__":
    main()
