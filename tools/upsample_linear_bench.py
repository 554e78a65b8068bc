#!/usr/bin/env python3
"""tools/upsample_linear_bench.py [runs=5] [window_ms=50] [out.json] — what upsampling a linear film costs and what it buys
(ptss_upsample_linear) on one GPU. Everything is reported, nothing is gated.

Times: one process, HIP events around windows of back-to-back calls on the current stream after a warm-up of the same shape, `runs`
windows per figure, milliseconds per call as median [min, max]; the legs of a comparison take turns window by window.
  call     to 1920x1080 and to 3840x2160 at factors 2 and 4 (from 960x540 and 480x270; from 1920x1080 and 960x540), and to 1920x1080 at
           factors 1 and 3 (from 1920x1080 and 640x360: every factor has a verdict), on a linear and on
           a filtered film of two rounds of "mixed": every tap from global memory (form 1) against the lo pixels of a tile divided
           once and staged in LDS (form 2), beside a device copy of the call's algorithmic bytes — per hi pixel its feature (32 B) and
           its film row (32 B), per lo pixel its film entry and its feature (64 B): 64 + 64 / f^2 — and ptss_upsample between the same
           sizes with the same features (8-bit pixels: 36 + 36 / f^2 bytes per hi pixel)
  staged wins  at a factor and kind only if the staged leg is faster in every interleaved pair of windows
  path     to 1920x1080 on "mixed", the same ray budget per display pixel: four rounds at 960x540 + denoise + upsample by 2 + meter +
           update + glare build + glare resolve, against one round at 1920x1080 + denoise + meter + update + glare build + glare resolve;
           and the small path with ONE round, a quarter of the rays: what §3.22 timed for the 8-bit route
Before anything is timed the forms' films are compared with each other byte for byte (the tests compare them with the probe).

Image error: "cornell" and "mixed" to 640x360 by factor 2, one run each, against a film of 4,096 samples per pixel at the large size.
Relative mean squared error of the linear means, mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01): (a) 16 rounds at
320x180, denoised, upsampled; (b) 4 rounds at 640x360, the same rays per display pixel, denoised; (c) as (b), not denoised. On the
display bytes, mean squared error over 0..255: (a), (b) and (d) today's route — resolve the small denoised film, then ptss_upsample of
its bytes. One run each: this tells the size of the effect on these two scenes at this budget, not its spread over seeds, scenes or
cameras."""
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
REFERENCE_SAMPLES = 4096
EW, EH = 320, 180   # the small film of the error runs


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


def zeros(n, columns=4, dtype=torch.int64):
    return torch.zeros((n, columns), dtype=dtype, device="cuda")


class Film:
    """A context of w x h on `scene` with its rays, streams, a linear film with moments and (filtered=True) a tent-filtered twin."""

    def __init__(self, scene, w, h, filtered=False):
        self.w, self.h, self.n = w, h, w * h
        self.r = ptss.Renderer(ptss.Scene(scene), w, h, seed=SEED, sync_each_frame=False)
        self.iterations = int(self.r.cfg.maxIterations)
        self.cam = ptss.default_camera()
        self.film_cam = ptss.film_camera("pinhole", w, h, self.cam)
        self.params = ptss.linear_params()
        self.rng = self.r.seed_path_rng(self.n, SEED, device=True)
        self.rays = zeros(self.n, 8, torch.float32)
        self.pos = zeros(self.n, 2, torch.float32)
        self.film, self.moments, self.clean = zeros(self.n), zeros(self.n), zeros(self.n)
        self.splat = zeros(self.n) if filtered else None
        self.flt = ptss.splat_filter("tent", 1.0)
        self.work = torch.zeros(ptss.denoise_linear_workspace(w, h), dtype=torch.uint8, device="cuda")
        self.features = self.centre(1)

    def centre(self, s):
        """The features of the centre rays of the same camera at s times the size."""
        n = self.n * s * s
        rng = self.r.seed_path_rng(n, SEED, device=True)
        rays = zeros(n, 8, torch.float32)
        self.r.generate_rays(ptss.film_camera("pinhole", self.w * s, self.h * s, self.cam, jitter=0), rng, rays=rays)
        return self.r.ray_features(rays).clone()

    def rounds(self, k):
        for _ in range(k):
            self.r.generate_rays(self.film_cam, self.rng, rays=self.rays, positions=self.pos)
            out = self.r.trace_paths(self.rays, self.rng, self.iterations, schedule=ptss.PATHS_REFILL)
            self.r.accumulate_paths_linear_stats(out, self.film, self.moments, params=self.params)
            if self.splat is not None:
                self.r.splat_paths(out, self.pos, self.splat, self.w, self.h, filter=self.flt, params=self.params, homed_first_pixel=0)

    def denoise(self):
        self.r.denoise_linear(self.film, self.w, self.h, self.moments, self.features, self.params, ptss.denoise_linear_params(), out=self.clean,
                              workspace=self.work)


def timing(results):
    L = ptss.device_lib()
    verdict = {}
    for (w, h) in ((480, 270), (640, 360), (960, 540), (1920, 1080)):
        s = Film("mixed", w, h, filtered=True)
        s.rounds(2)
        torch.cuda.synchronize()
        for f in (1, 2, 3, 4):
            W, H = w * f, h * f
            if (W, H) not in ((1920, 1080), (3840, 2160)) or (f in (1, 3) and W != 1920):
                continue
            fhi = s.centre(f)
            up = ptss.upsample_linear_params(f)
            out = zeros(W * H)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            lo_px = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda")
            hi_px = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
            s.r.resolve_linear(s.film, params=s.params, linear=zeros(w * h, 4, torch.float32), pixels=lo_px, history=zeros(w * h, 4, torch.float32))
            old = ptss.default_upsample_params(factor=f)
            copy_bytes = 64 * W * H + 64 * w * h
            src = torch.empty(copy_bytes // 8, dtype=torch.int32, device="cuda")
            dst = torch.empty_like(src)
            for kind, film in (("linear", s.film), ("splat", s.splat)):
                def call(form, target=out, film=film, kind=kind):
                    def run():
                        s.r.debug_upsample_linear_form(form)
                        s.r.upsample_linear(film, w, h, s.features, fhi, s.params, up, film_kind=kind, out=target)
                    return run
                films = []
                for form in (0, 1, 2):
                    o = torch.full((W * H, 4), -1, dtype=torch.int64, device="cuda")
                    call(form, o)()
                    torch.cuda.synchronize()
                    films.append(o.cpu().numpy().tobytes())
                if not films[0] == films[1] == films[2]:
                    raise SystemExit(f"upsample_linear_bench: the forms' films differ at {w}x{h} by {f} ({kind})")
                legs = {"global": call(1), "staged": call(2), "copy": lambda: dst.copy_(src),
                        "ptss_upsample": lambda: ptss._check(L.ptss_upsample(s.r._ctx, C.c_void_p(lo_px.data_ptr()), C.c_void_p(s.features.data_ptr()),
                                                                             C.c_void_p(fhi.data_ptr()), C.byref(old), C.c_void_p(hi_px.data_ptr()), None,
                                                                             stream))}
                ms = timed_legs(legs)
                wins = all(a < b for a, b in zip(ms["staged"], ms["global"]))
                key = f"call/{W}x{H}/f{f}/{kind}"
                results[key] = {k: stat(v) for k, v in ms.items()}
                results[key].update(staged_wins_every_pair=wins, copy_bytes=copy_bytes)
                verdict[f"{W}x{H}/f{f}/{kind}"] = wins
                print(f"{w}x{h} -> {W}x{H} (f = {f}, {kind}): global {fmt(stat(ms['global']))}, staged {fmt(stat(ms['staged']))}: staged "
                      f"{'wins every pair' if wins else 'does not win every pair'}; copy of {copy_bytes / 1e6:.1f} MB {fmt(stat(ms['copy']))}; "
                      f"ptss_upsample {fmt(stat(ms['ptss_upsample']))}", flush=True)
            s.r.debug_upsample_linear_form(0)
        s.r.close()
    results["staged_wins"] = verdict

    # the whole path to 1080p
    meter = ptss.meter_params(rate=0.5)
    glare = ptss.glare_params(levels=6, threshold=0.5, strength=0.1)
    W, H = 1920, 1080
    small, large = Film("mixed", W // 2, H // 2), Film("mixed", W, H)
    fhi = small.centre(2)
    up = ptss.upsample_linear_params(2)
    big = zeros(W * H)
    d_bins = torch.zeros(ptss.METER_BINS, dtype=torch.int32, device="cuda")
    d_state = torch.zeros(6, dtype=torch.int64, device="cuda")
    d_pyr = zeros(ptss.glare_layout(W, H, 6)[1])
    outs = dict(linear=zeros(W * H, 4, torch.float32), pixels=torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda"), history=zeros(W * H, 4, torch.float32))

    def tail(s, shown):
        d_bins.zero_()
        s.r.meter_linear(shown, histogram=d_bins)
        s.r.meter_exposure(d_bins, d_state, s.params, meter)
        s.r.glare_build(shown, W, H, s.params, glare, "linear", d_pyr)
        s.r.resolve_linear(shown, params=s.params, metered=d_state, glare=(W, H, glare, d_pyr), **outs)

    def small_path(rounds=4):
        small.rounds(rounds)
        small.denoise()
        small.r.upsample_linear(small.clean, W // 2, H // 2, small.features, fhi, small.params, up, out=big)
        tail(small, big)

    def large_path():
        large.rounds(1)
        large.denoise()
        tail(large, large.clean)

    ms = timed_legs({"small": small_path, "large": large_path, "small_one_round": lambda: small_path(1)})
    results["path"] = {k: stat(v) for k, v in ms.items()}
    results["path"]["small_over_large"] = statistics.median(ms["small"]) / statistics.median(ms["large"])
    results["path"]["small_one_round_over_large"] = statistics.median(ms["small_one_round"]) / statistics.median(ms["large"])
    print(f"to 1080p on mixed, one ray per display pixel: four rounds at 540p + denoise + upsample + meter + glare + resolve "
          f"{fmt(stat(ms['small']))}; one round at 1080p + denoise + meter + glare + resolve {fmt(stat(ms['large']))}: ratio "
          f"{results['path']['small_over_large']:.3f}; the small path with one round (a quarter of the rays) {fmt(stat(ms['small_one_round']))}: "
          f"ratio {results['path']['small_one_round_over_large']:.3f}", flush=True)
    small.r.close()
    large.r.close()


def rel_mse(x, ref):
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


def means_of(film, params):
    w = film.cpu().numpy().view(np.uint64).reshape(-1, 4)
    n = np.maximum(w[:, 3] & np.uint64(0xffffffff), np.uint64(1)).astype(np.float64)
    return w[:, :3].astype(np.float64) / n[:, None] * 2.0 ** -params.scaleLog2


def errors(results):
    f, budget = 2, 4   # rounds at the large size; f^2 times as many at the small one
    W, H = EW * f, EH * f
    L = ptss.device_lib()
    for scene in ("cornell", "mixed"):
        small, large = Film(scene, EW, EH), Film(scene, W, H)
        params = small.params
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def display(s, film, n):
            px = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            s.r.resolve_linear(film, params=params, linear=zeros(n, 4, torch.float32), pixels=px, history=zeros(n, 4, torch.float32))
            torch.cuda.synchronize()
            return px

        fhi = small.centre(f)
        small.rounds(budget * f * f)
        small.denoise()
        big = zeros(W * H)
        info = torch.zeros(3, dtype=torch.int64, device="cuda")
        small.r.upsample_linear(small.clean, EW, EH, small.features, fhi, params, ptss.upsample_linear_params(f), out=big, info=info)
        a_lin, a_px = means_of(big, params), display(small, big, W * H).cpu().numpy()[:, :3].astype(np.float64)
        lo_px = display(small, small.clean, EW * EH)   # today's route: resolve small, then ptss_upsample of the bytes
        hi_px = torch.zeros((W * H, 4), dtype=torch.uint8, device="cuda")
        old = ptss.default_upsample_params(factor=f)
        ptss._check(L.ptss_upsample(small.r._ctx, C.c_void_p(lo_px.data_ptr()), C.c_void_p(small.features.data_ptr()), C.c_void_p(fhi.data_ptr()),
                                    C.byref(old), C.c_void_p(hi_px.data_ptr()), None, stream))
        torch.cuda.synchronize()
        d_px = hi_px.cpu().numpy()[:, :3].astype(np.float64)
        large.rounds(budget)
        large.denoise()
        b_lin, b_px = means_of(large.clean, params), display(large, large.clean, W * H).cpu().numpy()[:, :3].astype(np.float64)
        c_lin = means_of(large.film, params)
        large.rounds(REFERENCE_SAMPLES - budget)
        ref_lin, ref_px = means_of(large.film, params), display(large, large.film, W * H).cpu().numpy()[:, :3].astype(np.float64)
        res = {"linear_relmse_small_denoised_upsampled": rel_mse(a_lin, ref_lin), "linear_relmse_large_denoised": rel_mse(b_lin, ref_lin),
               "linear_relmse_large_plain": rel_mse(c_lin, ref_lin), "display_mse_small_denoised_upsampled": float(np.mean((a_px - ref_px) ** 2)),
               "display_mse_large_denoised": float(np.mean((b_px - ref_px) ** 2)),
               "display_mse_resolve_small_then_ptss_upsample": float(np.mean((d_px - ref_px) ** 2)),
               "info": dict(zip(("filtered", "fallback", "empty"), (int(v) for v in info.cpu())))}
        results[f"error/{scene}"] = res
        print(f"{scene} to {W}x{H}, {budget} rays per display pixel against {REFERENCE_SAMPLES}: " +
              ", ".join(f"{k} {v:.4g}" if not isinstance(v, dict) else f"{k} {v}" for k, v in res.items()), flush=True)
        small.r.close()
        large.r.close()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("upsample_linear_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    results = {}
    what = os.environ.get("PTSS_UPSAMPLE_LINEAR_BENCH", "times,errors")
    if "times" in what:
        timing(results)
    if "errors" in what:
        errors(results)
    out = {"runs": runs, "window_ms": window_ms, "unit": "ms per call", "error_size": f"{EW}x{EH} -> {2 * EW}x{2 * EH}",
           "device": torch.cuda.get_device_name(0), "results": results}
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
