#!/usr/bin/env python3
"""tools/surface_bench.py [runs=5] [window_ms=50] [out.json] — what rays from surface points and the gutter fill cost
(ptss_generate_rays_surface, ptss_dilate_linear) on one GPU. Everything is reported, nothing is gated.

Times: one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  generate  2^21 rays over the atlas of the 1,296-triangle mesh scene (tests/scene_update_common.m1296: a mesh image), cosine mode,
            without surfels: in point order (ray i leaves from point i mod K) and with a permuted index, beside ptss_generate_rays at
            the same n (a 2048 x 1024 pinhole film with jitter) and a device copy of the call's algorithmic bytes — per ray its index
            (4 B), its point row (16 B), six rows of its triangle (96 B), its stream in and out (48 B) and its ray (32 B): 196 B;
            and the same call over 64 rays: what the wrapper and a launch cost, the floor under every figure of this tool
  dilate    2048 x 2048, a film with 60 % of its texels filled: the nine rows from global memory (form 1) against the tile staged in
            LDS (form 2), beside a device copy of the film in and out (64 B a texel)
  staged wins  only if the staged leg is faster in every interleaved pair of windows
  round     generate -> ptss_trace_paths -> ptss_accumulate_paths_linear: a bake round over K texels (cosine, indexed by texel)
            against a film round of as many pinhole rays (no index)
Before anything is timed the two dilate forms are compared byte for byte (the tests compare them with the probe)."""
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
N = 1 << 21
RAY_BYTES = 4 + 16 + 96 + 48 + 32


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    scene = m1296()
    tri = ptss.scene_records(scene)[0]
    r = ptss.Renderer(scene, 64, 64, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    points, texels, height = ptss.surface_atlas(tri, 100.0, 2048, 1, 64)
    K = len(points)
    d_points = dev(points, np.int32).reshape(-1, 4)
    cosine = ptss.surface_params("cosine")
    g = np.random.default_rng(1)

    # ---- the generator at 2^21 rays ----
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    in_order = dev((np.arange(N) % K).astype(np.uint32), np.int32)
    permuted = dev(g.permutation(N).astype(np.uint64) % K, np.int64).to(torch.int32)
    film_cam = ptss.film_camera("pinhole", 2048, 1024, ptss.default_camera())
    ms = timed_legs({"point_order": lambda: r.generate_rays_surface(d_points, rng, cosine, index=in_order, rays=rays),
                     "permuted": lambda: r.generate_rays_surface(d_points, rng, cosine, index=permuted, rays=rays),
                     "generate_rays": lambda: r.generate_rays(film_cam, rng, rays=rays), "copy": copy_leg(N * RAY_BYTES),
                     "call_of_64_rays": lambda: r.generate_rays_surface(d_points, rng[:64], cosine, index=in_order[:64], rays=rays[:64])})
    results["generate"] = {k: stat(v) for k, v in ms.items()}
    results["generate"].update(rays=N, points=K, atlas=[2048, height], copy_bytes=N * RAY_BYTES, rejected=r.surface_rejected())
    print(f"generate, {N} rays over {K} points of {len(tri)} triangles: point order {fmt(stat(ms['point_order']))}, permuted index "
          f"{fmt(stat(ms['permuted']))}; ptss_generate_rays {fmt(stat(ms['generate_rays']))}; copy of {N * RAY_BYTES / 1e6:.0f} MB {fmt(stat(ms['copy']))}; "
          f"the same call over 64 rays (what the wrapper and a launch cost) {fmt(stat(ms['call_of_64_rays']))}",
          flush=True)
    del rng, rays, in_order, permuted

    # ---- the gutter fill at 2048 x 2048 ----
    W = H = 2048
    film = np.zeros(W * H, dtype=ptss.LINEAR_DTYPE)
    n = g.integers(1, 64, W * H).astype(np.uint32) * (g.random(W * H) < 0.6)
    for ch in "rgb":
        film[ch] = g.integers(0, 1 << 30, W * H).astype(np.uint64) * n
    film["samples"] = n
    d_film = dev(film, np.int64).reshape(-1, 4)
    outs = []
    for form in (1, 2):
        o = torch.full((W * H, 4), -1, dtype=torch.int64, device="cuda")
        r.debug_dilate_linear_form(form)
        r.dilate_linear(d_film, W, H, out=o)
        torch.cuda.synchronize()
        outs.append(o.cpu().numpy().tobytes())
    if outs[0] != outs[1]:
        raise SystemExit("surface_bench: the two dilate forms differ")
    d_out = torch.zeros((W * H, 4), dtype=torch.int64, device="cuda")

    def dilate(form):
        def run():
            r.debug_dilate_linear_form(form)
            r.dilate_linear(d_film, W, H, out=d_out)
        return run

    t_film, t_out = d_film[:256].clone(), d_out[:256].clone()
    ms = timed_legs({"global": dilate(1), "staged": dilate(2), "copy": copy_leg(64 * W * H),
                     "call_of_16x16": lambda: r.dilate_linear(t_film, 16, 16, out=t_out)})
    r.debug_dilate_linear_form(0)
    wins = all(a < b for a, b in zip(ms["staged"], ms["global"]))
    results["dilate"] = {k: stat(v) for k, v in ms.items()}
    results["dilate"].update(size=[W, H], staged_wins_every_pair=wins, copy_bytes=64 * W * H)
    print(f"dilate {W} x {H}: global {fmt(stat(ms['global']))}, staged {fmt(stat(ms['staged']))}: staged "
          f"{'wins every pair' if wins else 'does not win every pair'}; copy of {64 * W * H / 1e6:.0f} MB {fmt(stat(ms['copy']))}; the same call over 16 x 16 {fmt(stat(ms['call_of_16x16']))}", flush=True)
    del d_film, d_out

    # ---- a bake round against a film round of as many rays ----
    fw = 1024
    fh = K // fw
    M = fw * fh
    params = ptss.linear_params()
    b_rng, f_rng = r.seed_path_rng(M, SEED, device=True), r.seed_path_rng(M, SEED, device=True)
    b_rays, f_rays = (torch.zeros((M, 8), dtype=torch.float32, device="cuda") for _ in range(2))
    b_film = torch.zeros((2048 * height, 4), dtype=torch.int64, device="cuda")
    f_film = torch.zeros((M, 4), dtype=torch.int64, device="cuda")
    d_texels = dev(texels[:M], np.int32)
    cam = ptss.film_camera("pinhole", fw, fh, ptss.default_camera())

    def bake_round():
        r.generate_rays_surface(d_points, b_rng, cosine, rays=b_rays)
        out = r.trace_paths(b_rays, b_rng, iterations)
        r.accumulate_paths_linear(out, b_film, index=d_texels, params=params)

    def film_round():
        r.generate_rays(cam, f_rng, rays=f_rays)
        out = r.trace_paths(f_rays, f_rng, iterations)
        r.accumulate_paths_linear(out, f_film, params=params)

    ms = timed_legs({"bake": bake_round, "film": film_round})
    results["round"] = {k: stat(v) for k, v in ms.items()}
    results["round"].update(rays=M, iterations=iterations, bake_over_film=statistics.median(ms["bake"]) / statistics.median(ms["film"]))
    print(f"a round of {M} rays, {iterations} iterations: bake {fmt(stat(ms['bake']))}, film {fmt(stat(ms['film']))}: ratio "
          f"{results['round']['bake_over_film']:.3f}", flush=True)
    r.close()
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
