#!/usr/bin/env python3
"""tools/lightmap_bench.py [runs=5] [window_ms=50] [out.json] — what reading a baked light map back costs (ptss_lookup_lightmap;
DESIGN.md §3.39) on one GPU. Everything is reported, nothing is gated.

Times: one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
Per scene — the 1,296-triangle mesh scene of tools/surface_bench.py (tests/scene_update_common.m1296) and the `mixed` preset (16 triangles,
22 spheres) — the hits are ptss_intersect of the centre rays of a 1920 x 1080 pinhole camera, the map is a bake of four rounds through
ptss_surface_atlas_blocks into 2048 columns with one gutter pass, and both flags are on:
  forms     form 1 (one lane per hit) against form 2 (four lanes per hit) per filter; a form wins only if it is faster in every
            interleaved pair of windows
  shipped   form 0, bilinear, beside a device copy of its algorithmic bytes (per hit two hit rows, one block row, four texels, one
            row out: 32 + 16 + 128 + 32 = 208 B), ptss_upsample_linear at f = 1 over a 1080p film (the nearest existing four-tap gather
            with wide divisions), and the same call over 64 hits (what the wrapper and a launch cost)
  ones      the lookup on the same map normalised to samples == 1 rows (no division of a tap) against the baked map
  round     the whole view — ptss_generate_rays (jitter 0) + ptss_intersect + lookup + ptss_resolve_linear — against one path-traced
            film round of the same size: generate + ptss_trace_paths + ptss_accumulate_paths_linear + ptss_resolve_linear
Before anything is timed the two forms are compared byte for byte per filter (the tests compare them with the probe)."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (initialises the HIP runtime first, as bench.py does)
import ptss  # noqa: E402
from scene_update_common import m1296  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
window_ms = float(sys.argv[2]) if len(sys.argv) > 2 else 50.0
out_path = sys.argv[3] if len(sys.argv) > 3 else None
SEED = 0x5EED
MAX_CALLS = 2000
W, H = 1920, 1080
N = W * H
ATLAS_WIDTH = 2048
HIT_BYTES = 32 + 16 + 4 * 32 + 32
FILTERS = ("nearest", "bilinear")


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


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


def copy_leg(nbytes):
    """A device copy whose traffic (read + write) is nbytes."""
    src = torch.empty(nbytes // 8, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


def bench_scene(name, scene, texels_per_unit):
    tri, sph = ptss.scene_records(scene)
    r = ptss.Renderer(scene, 64, 64, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film = ptss.linear_params()
    bt, bs, points, texels, height = ptss.surface_atlas_blocks(tri, sph, texels_per_unit, ATLAS_WIDTH, 1, 64)
    K, P = len(points), ATLAS_WIDTH * height
    d_points, d_texels = dev(points, np.int32).reshape(-1, 4), dev(texels, np.int32)
    d_bt = dev(bt, np.int32).reshape(-1, 4) if len(bt) else None
    d_bs = dev(bs, np.int32).reshape(-1, 4) if len(bs) else None

    # ---- the bake: four rounds, one gutter pass ----
    cosine = ptss.surface_params("cosine")
    b_rng = r.seed_path_rng(K, SEED, device=True)
    b_rays = torch.zeros((K, 8), dtype=torch.float32, device="cuda")
    raw = torch.zeros((P, 4), dtype=torch.int64, device="cuda")
    for _ in range(4):
        r.generate_rays_surface(d_points, b_rng, cosine, rays=b_rays)
        r.accumulate_paths_linear(r.trace_paths(b_rays, b_rng, iterations), raw, index=d_texels, params=film)
    baked = r.dilate_linear(raw, ATLAS_WIDTH, height)
    torch.cuda.synchronize()
    host = baked.cpu().numpy().view(np.uint64)
    samples = host[:, 3] & np.uint64(0xffffffff)
    ones = host.copy()
    full = samples > 0
    for c in range(3):
        ones[full, c] = (host[full, c] + samples[full] // np.uint64(2)) // samples[full]
    ones[full, 3] = 1
    d_ones = dev(ones, np.int64).reshape(-1, 4)
    del b_rng, b_rays, raw

    # ---- the hits of a 1080p camera ----
    centre = ptss.film_camera("pinhole", W, H, ptss.default_camera(), jitter=0)
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    r.generate_rays(centre, rng, rays=rays)
    hits = r.intersect(rays).clone()
    out = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    info = torch.zeros(4, dtype=torch.int32, device="cuda")
    params = {f: ptss.lightmap_params(ATLAS_WIDTH, height, f, modulate=True, emission=True) for f in FILTERS}

    def lookup(form, filter, map_=baked, h=hits, o=out):
        def run():
            r.debug_lightmap_form(form)
            r.lookup_lightmap(h, map_, params[filter], d_bt, d_bs, film=film, out=o)
        return run

    for filter in FILTERS:
        got = []
        for form in (1, 2):
            out.fill_(-1)
            lookup(form, filter)()
            torch.cuda.synchronize()
            got.append(out.cpu().numpy().tobytes())
        if got[0] != got[1]:
            raise SystemExit(f"lightmap_bench: the two forms differ ({name}, {filter})")
    r.debug_lightmap_form(0)
    r.lookup_lightmap(hits, baked, params["bilinear"], d_bt, d_bs, film=film, out=out, info=info)
    counts = [int(v) for v in info.cpu().numpy()]
    res = {"hits": N, "atlas": [ATLAS_WIDTH, height], "points": K, "triangles": len(tri), "spheres": len(sph), "counts": counts}
    print(f"{name}: {N} hits, atlas {ATLAS_WIDTH} x {height} ({K} texels of {len(tri)} triangles and {len(sph)} spheres); filtered, empty, no block, "
          f"rejected = {counts}", flush=True)

    # ---- form 1 against form 2, per filter ----
    res["forms"] = {}
    for filter in FILTERS:
        ms = timed_legs({"one_lane": lookup(1, filter), "quad": lookup(2, filter)})
        quad_wins = all(a < b for a, b in zip(ms["quad"], ms["one_lane"]))
        lane_wins = all(a < b for a, b in zip(ms["one_lane"], ms["quad"]))
        res["forms"][filter] = {k: stat(v) for k, v in ms.items()}
        res["forms"][filter].update(quad_wins_every_pair=quad_wins, one_lane_wins_every_pair=lane_wins)
        verdict = "four lanes win every pair" if quad_wins else "one lane wins every pair" if lane_wins else "neither wins every pair"
        print(f"  {filter}: one lane per hit {fmt(stat(ms['one_lane']))}, four lanes per hit {fmt(stat(ms['quad']))}: {verdict}", flush=True)

    # ---- the shipped form beside a copy, the upsample at f = 1, a call of 64 hits, the map of samples == 1 rows ----
    features = r.ray_features(rays).clone()
    frame = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    frame[:, :3] = 12345 * 7
    frame[:, 3] = 7
    up_out = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    up = ptss.upsample_linear_params(1)
    small_out = out[:64].clone()
    ms = timed_legs({"shipped": lookup(0, "bilinear"), "samples_1_map": lookup(0, "bilinear", map_=d_ones), "copy": copy_leg(N * HIT_BYTES),
                     "upsample_linear_f1": lambda: r.upsample_linear(frame, W, H, features, features, film, up, out=up_out),
                     "call_of_64_hits": lookup(0, "bilinear", h=hits[:64], o=small_out)})
    res["shipped"] = {k: stat(v) for k, v in ms.items()}
    res["shipped"].update(copy_bytes=N * HIT_BYTES)
    print(f"  shipped form, bilinear: {fmt(stat(ms['shipped']))}; on the map of samples == 1 rows {fmt(stat(ms['samples_1_map']))}; copy of "
          f"{N * HIT_BYTES / 1e6:.0f} MB {fmt(stat(ms['copy']))}; ptss_upsample_linear at f = 1 {fmt(stat(ms['upsample_linear_f1']))}; the same call over "
          f"64 hits {fmt(stat(ms['call_of_64_hits']))}", flush=True)
    del features, frame, up_out

    # ---- the whole view against a path-traced film round ----
    means = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    jittered = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    f_film = torch.zeros((N, 4), dtype=torch.int64, device="cuda")

    def view_round():
        r.generate_rays(centre, rng, rays=rays)
        r.lookup_lightmap(r.intersect(rays), baked, params["bilinear"], d_bt, d_bs, film=film, out=out)
        r.resolve_linear(out, params=film, linear=means, pixels=None, history=None)

    def film_round():
        r.generate_rays(jittered, rng, rays=rays)
        res_ = r.trace_paths(rays, rng, iterations)
        r.accumulate_paths_linear(res_, f_film, params=film)
        r.resolve_linear(f_film, params=film, linear=means, pixels=None, history=None)

    ms = timed_legs({"view": view_round, "film": film_round})
    res["round"] = {k: stat(v) for k, v in ms.items()}
    res["round"].update(iterations=iterations, view_over_film=statistics.median(ms["view"]) / statistics.median(ms["film"]))
    print(f"  view round (generate, intersect, lookup, resolve) {fmt(stat(ms['view']))}; path-traced film round, {iterations} iterations "
          f"{fmt(stat(ms['film']))}: ratio {res['round']['view_over_film']:.4f}", flush=True)
    r.close()
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("lightmap_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {"m1296": bench_scene("m1296", m1296(), 100.0), "mixed": bench_scene("mixed", ptss.Scene("mixed"), 40.0)}
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
