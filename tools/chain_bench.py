#!/usr/bin/env python3
"""tools/chain_bench.py [runs=5] [window_ms=50] [out.json] — what following mirrors and glass in a ray query costs and what it buys the
light-map view (ptss_intersect_chain, ptss_lookup_lightmap_chain) on one GPU. Everything is reported, nothing is gated.

Times: one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window, and a leg wins
only if it is faster in every interleaved pair.
Per scene — `mixed` (16 triangles, 22 spheres; mirrors and glass among them) and the mesh scene (the `mesh` preset, 1,296 + 16 triangles,
its icosphere turned into a flagged mirror as tests/test_gpu_specular_features.mirror_mesh does: a mesh image whose chains leave from its
triangles) — the rays are the centre rays of a 1920 x 1080 pinhole camera:
  schedules  PTSS_CHAIN_LANE_PER_RAY against PTSS_CHAIN_REFILL (maxWorkgroups 0) at maxSteps 1, 4 and 8, after a byte comparison
  links      the call at maxSteps 4 beside ptss_intersect of the same rays times (1 + mean steps): what the chain's queries would cost
             as whole-batch intersections
  features   the call at maxSteps 4 beside ptss_render_features_specular(4) of the same camera (specularFeatureKernel: the same chain
             from the context's own camera, a feature row out)
  lookup     ptss_lookup_lightmap_chain beside ptss_lookup_lightmap on the chain's hits (bilinear, both flags)
  round      the whole view at N = 4 — generate (jitter 0) + ptss_intersect_chain + tinted lookup + resolve — beside the view at N = 0
             (ptss_intersect + plain lookup) and beside one path-traced film round of the same size
Image error (`mixed` and `default`, 256 x 192, one run each): the view at N = 0 and N = 4 from a bake of 64 rounds against a path-traced
film of 4,096 samples per pixel, as relative MSE = sum (view - truth)^2 / sum truth^2 over the linear means of all pixels and channels;
the same over the pixels whose chain followed at least one link."""
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
SEED = 0x5EED
MAX_CALLS = 2000
W, H = 1920, 1080
N = W * H
ATLAS_WIDTH = 2048
STEPS = (1, 4, 8)


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


def mirror_mesh():
    s = ptss.Scene("mesh")
    m = s.desc.materials[s.desc.numMaterials - 1]
    m.diffAvg, m.specAvg, m.flags = 0.0, 0.9, b"\x01"
    return s


def bake(r, scene, texels_per_unit, rounds, film):
    """A light map through ptss_surface_atlas_blocks into ATLAS_WIDTH columns, one gutter pass -> (map, block tables, height)."""
    tri, sph = ptss.scene_records(scene)
    iterations = int(r.cfg.maxIterations)
    bt, bs, points, texels, height = ptss.surface_atlas_blocks(tri, sph, texels_per_unit, ATLAS_WIDTH, 1, 64)
    K, P = len(points), ATLAS_WIDTH * height
    d_points, d_texels = dev(points, np.int32).reshape(-1, 4), dev(texels, np.int32)
    d_bt = dev(bt, np.int32).reshape(-1, 4) if len(bt) else None
    d_bs = dev(bs, np.int32).reshape(-1, 4) if len(bs) else None
    cosine = ptss.surface_params("cosine")
    rng = r.seed_path_rng(K, SEED, device=True)
    rays = torch.zeros((K, 8), dtype=torch.float32, device="cuda")
    raw = torch.zeros((P, 4), dtype=torch.int64, device="cuda")
    for _ in range(rounds):
        r.generate_rays_surface(d_points, rng, cosine, rays=rays)
        r.accumulate_paths_linear(r.trace_paths(rays, rng, iterations), raw, index=d_texels, params=film)
    baked = r.dilate_linear(raw, ATLAS_WIDTH, height)
    torch.cuda.synchronize()
    return baked, d_bt, d_bs, height


def wins(ms, a, b):
    if all(x < y for x, y in zip(ms[a], ms[b])):
        return a
    if all(y < x for x, y in zip(ms[a], ms[b])):
        return b
    return None


def bench_scene(name, scene, texels_per_unit):
    r = ptss.Renderer(scene, W, H, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film = ptss.linear_params()
    baked, d_bt, d_bs, height = bake(r, scene, texels_per_unit, 4, film)
    centre = ptss.film_camera("pinhole", W, H, ptss.default_camera(), jitter=0)
    rng = r.seed_path_rng(N, SEED, device=True)
    rays = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    r.generate_rays(centre, rng, rays=rays)
    chain = torch.zeros((N, 8), dtype=torch.float32, device="cuda")
    res = {"rays": N, "iterations": iterations, "schedules": {}}

    # ---- the two schedules ----
    mean_steps = {}
    for max_steps in STEPS:
        got = []
        for schedule in ("lane", "refill"):
            hits, rows = r.intersect_chain(rays, max_steps, schedule)
            torch.cuda.synchronize()
            got.append((hits.cpu().numpy().tobytes(), rows.cpu().numpy().tobytes()))
        if got[0] != got[1]:
            raise SystemExit(f"chain_bench: the two schedules differ ({name}, maxSteps {max_steps})")
        steps = rows.cpu().numpy().view(np.uint32)[:, 3]
        mean_steps[max_steps] = float(steps.mean())
        ms = timed_legs({"lane": lambda: r.intersect_chain(rays, max_steps, "lane", chain=chain),
                         "refill": lambda: r.intersect_chain(rays, max_steps, "refill", chain=chain)})
        winner = wins(ms, "lane", "refill")
        ratio = statistics.median(ms["refill"]) / statistics.median(ms["lane"])
        res["schedules"][max_steps] = {"lane": stat(ms["lane"]), "refill": stat(ms["refill"]), "refill_over_lane": ratio, "wins_every_pair": winner,
                                       "mean_steps": mean_steps[max_steps], "rays_with_steps": float((steps > 0).mean())}
        print(f"{name}, maxSteps {max_steps} (mean steps {mean_steps[max_steps]:.3f}, {100 * (steps > 0).mean():.1f} % of the rays follow a link): one lane per ray "
              f"{fmt(stat(ms['lane']))}, refill {fmt(stat(ms['refill']))}: refill / lane {ratio:.3f}, "
              f"{winner + ' wins every pair' if winner else 'neither wins every pair'}", flush=True)

    # ---- beside ptss_intersect times (1 + mean steps), beside specularFeatureKernel ----
    L = ptss.device_lib()
    d_feat, d_steps = r.features_specular_devptr(), r._device_buffer("specular_steps", r.local_pixels * 4)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def features():
        if L.ptss_render_features_specular(r._ctx, 4, d_feat, d_steps, stream) != 0:
            raise SystemExit("chain_bench: ptss_render_features_specular failed")

    ms = timed_legs({"chain": lambda: r.intersect_chain(rays, 4, None, chain=chain), "hits_only": lambda: r.intersect_chain(rays, 4, None, chain=False),
                     "intersect": lambda: r.intersect(rays), "features_specular": features})
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["links"] = {k: stat(v) for k, v in ms.items()}
    res["links"].update(mean_steps=mean_steps[4], intersect_times_links=med["intersect"] * (1 + mean_steps[4]),
                        chain_over_intersect_times_links=med["chain"] / (med["intersect"] * (1 + mean_steps[4])),
                        chain_over_features=med["chain"] / med["features_specular"])
    print(f"{name}, maxSteps 4, the default schedule: chain {fmt(stat(ms['chain']))} (without dev_chain {fmt(stat(ms['hits_only']))}); ptss_intersect "
          f"{fmt(stat(ms['intersect']))} x (1 + {mean_steps[4]:.3f}) = {res['links']['intersect_times_links']:.4f} ms: ratio "
          f"{res['links']['chain_over_intersect_times_links']:.3f}; ptss_render_features_specular(4) {fmt(stat(ms['features_specular']))}: ratio "
          f"{res['links']['chain_over_features']:.3f}", flush=True)

    # ---- the tinted lookup beside the plain one ----
    hits, rows = r.intersect_chain(rays, 4)
    hits, rows = hits.clone(), rows.clone()
    out = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
    params = ptss.lightmap_params(ATLAS_WIDTH, height, "bilinear", modulate=True, emission=True)
    ms = timed_legs({"plain": lambda: r.lookup_lightmap(hits, baked, params, d_bt, d_bs, film=film, out=out),
                     "tinted": lambda: r.lookup_lightmap(hits, baked, params, d_bt, d_bs, film=film, out=out, chain=rows)})
    res["lookup"] = {k: stat(v) for k, v in ms.items()}
    res["lookup"].update(tinted_over_plain=statistics.median(ms["tinted"]) / statistics.median(ms["plain"]))
    print(f"{name}, lookup: plain {fmt(stat(ms['plain']))}, tinted {fmt(stat(ms['tinted']))}: ratio {res['lookup']['tinted_over_plain']:.3f}", flush=True)

    # ---- the whole view at N = 4 and N = 0, a path-traced film round ----
    means = torch.zeros((N, 4), dtype=torch.float32, device="cuda")
    jittered = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    f_film = torch.zeros((N, 4), dtype=torch.int64, device="cuda")

    def view_chain():
        r.generate_rays(centre, rng, rays=rays)
        h, c = r.intersect_chain(rays, 4, None, chain=chain)
        r.lookup_lightmap(h, baked, params, d_bt, d_bs, film=film, out=out, chain=c)
        r.resolve_linear(out, params=film, linear=means, pixels=None, history=None)

    def view_plain():
        r.generate_rays(centre, rng, rays=rays)
        r.lookup_lightmap(r.intersect(rays), baked, params, d_bt, d_bs, film=film, out=out)
        r.resolve_linear(out, params=film, linear=means, pixels=None, history=None)

    def film_round():
        r.generate_rays(jittered, rng, rays=rays)
        res_ = r.trace_paths(rays, rng, iterations)
        r.accumulate_paths_linear(res_, f_film, params=film)
        r.resolve_linear(f_film, params=film, linear=means, pixels=None, history=None)

    ms = timed_legs({"view_4": view_chain, "view_0": view_plain, "film": film_round})
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["round"] = {k: stat(v) for k, v in ms.items()}
    res["round"].update(view_4_over_view_0=med["view_4"] / med["view_0"], view_4_over_film=med["view_4"] / med["film"],
                        view_0_over_film=med["view_0"] / med["film"])
    print(f"{name}, round: view at N = 4 {fmt(stat(ms['view_4']))}, view at N = 0 {fmt(stat(ms['view_0']))}, path-traced film round ({iterations} iterations) "
          f"{fmt(stat(ms['film']))}: N = 4 / N = 0 {res['round']['view_4_over_view_0']:.3f}, N = 4 / film {res['round']['view_4_over_film']:.4f}, "
          f"N = 0 / film {res['round']['view_0_over_film']:.4f}", flush=True)
    r.close()
    return res


def image_error(name, scene, texels_per_unit, w=256, h=192, samples=4096, bake_rounds=64):
    n = w * h
    r = ptss.Renderer(scene, w, h, seed=SEED, sync_each_frame=False)
    iterations = int(r.cfg.maxIterations)
    film = ptss.linear_params()
    baked, d_bt, d_bs, height = bake(r, scene, texels_per_unit, bake_rounds, film)
    params = ptss.lightmap_params(ATLAS_WIDTH, height, "bilinear", modulate=True, emission=True)
    rng = r.seed_path_rng(n, SEED, device=True)
    rays = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    means = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    truth_film = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    jittered = ptss.film_camera("pinhole", w, h, ptss.default_camera())
    for _ in range(samples):
        r.generate_rays(jittered, rng, rays=rays)
        r.accumulate_paths_linear(r.trace_paths(rays, rng, iterations), truth_film, params=film)
    r.resolve_linear(truth_film, params=film, linear=means, pixels=None, history=None)
    torch.cuda.synchronize()
    truth = means.cpu().numpy()[:, :3].astype(np.float64)
    r.generate_rays(ptss.film_camera("pinhole", w, h, ptss.default_camera(), jitter=0), rng, rays=rays)
    out = {"size": [w, h], "samples": samples, "bake_rounds": bake_rounds, "iterations": iterations}
    views = {}
    for steps in (0, 4):
        hits, rows = r.intersect_chain(rays, steps)
        view = r.lookup_lightmap(hits, baked, params, d_bt, d_bs, film=film, chain=rows)
        r.resolve_linear(view, params=film, linear=means, pixels=None, history=None)
        torch.cuda.synchronize()
        views[steps] = means.cpu().numpy()[:, :3].astype(np.float64)
        followed = rows.cpu().numpy().view(np.uint32)[:, 3] > 0
    rel = lambda a, mask: float(((a[mask] - truth[mask]) ** 2).sum() / max((truth[mask] ** 2).sum(), 1e-300))
    everywhere = np.ones(n, dtype=bool)
    for steps in (0, 4):
        out[f"relative_mse_n{steps}"] = rel(views[steps], everywhere)
        out[f"relative_mse_n{steps}_behind_a_link"] = rel(views[steps], followed)
    out["pixels_behind_a_link"] = float(followed.mean())
    print(f"image error, {name}, {w} x {h}, truth {samples} spp, bake {bake_rounds} rounds: relative MSE of the view at N = 0 {out['relative_mse_n0']:.4f}, "
          f"at N = 4 {out['relative_mse_n4']:.4f}; over the {100 * followed.mean():.1f} % of the pixels whose chain follows a link: N = 0 "
          f"{out['relative_mse_n0_behind_a_link']:.4f}, N = 4 {out['relative_mse_n4_behind_a_link']:.4f}", flush=True)
    r.close()
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("chain_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {"mixed": bench_scene("mixed", ptss.Scene("mixed"), 40.0), "mirror_mesh": bench_scene("mirror_mesh", mirror_mesh(), 40.0)}
    errors = {"mixed": image_error("mixed", ptss.Scene("mixed"), 40.0), "default": image_error("default", ptss.Scene("default"), 40.0)}
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "device": torch.cuda.get_device_name(0), "results": results, "image_error": errors}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
