"""ptss_main --film KIND --linear [exposure] --filter box|tent|gaussian[,radius[,alpha]]: rounds go through
ptss_generate_rays_positions, the trace and ptss_splat_paths_homed, and ptss_resolve_splat makes the screenshot, the PFM beside it and,
with --denoise, the history the filter takes. The files are the ones the Python face computes from the same calls; without --filter the
program writes the bytes of --linear alone."""
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, N, SCENES, W
from test_gpu_linear_main import ARGS, BOUNCES, MAIN, NAME, SEED, TICKS, read_pfm, read_tga, run_main

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spec, flt, extra, exposure", [("tent", ("tent", 1.0, 2.0), [], None),
                                                        ("gaussian,2,2", ("gaussian", 2.0, 2.0), ["--refill", "--denoise", "2"], 0.5)])
def test_filter_writes_the_python_faces_files(tmp_path, spec, flt, extra, exposure):
    run_main(["--film", "pinhole", "--linear"] + ([str(exposure)] if exposure is not None else []) + ["--filter", spec] + extra, tmp_path / "shot.tga")
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params, flt = ptss.linear_params(exposure=1.0 if exposure is None else exposure), ptss.splat_filter(*flt)
    rng, film = r.seed_path_rng(N, SEED), np.zeros(N, ptss.SPLAT_DTYPE)
    for _ in range(TICKS):
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        res, rng = r.trace_paths(rays, rng, BOUNCES, schedule=ptss.PATHS_REFILL if extra else None)
        film = r.splat_paths(res, pos, film, W, H, filter=flt, params=params, homed_first_pixel=0)
    linear, pixels, history = r.resolve_splat(film, params=params)
    assert r.splat_stats()[:4] == (0, TICKS, 1, 0) and (film["weight"] > 0).all()
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3])
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0
    if extra:
        film_cam.jitter = 0
        feat = r.ray_features(r.generate_rays(film_cam, rng)[0])
        assert np.array_equal(read_tga(tmp_path / "shot_denoised.tga"), r.denoise_history(history=history, features=feat, levels=2)[:, :3])
    r.close()


def test_without_the_flag_the_linear_films_bytes(tmp_path):
    linear = run_main(["--film", "pinhole", "--linear"], tmp_path / "linear.tga")
    pfm = open(tmp_path / "linear.pfm", "rb").read()
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    rng, film = r.seed_path_rng(N, SEED), np.zeros(N, ptss.LINEAR_DTYPE)
    for _ in range(TICKS):
        rays, rng = r.generate_rays(film_cam, rng)
        res, rng = r.trace_paths(rays, rng, BOUNCES)
        film = r.accumulate_paths_linear(res, film)
    means, pixels, _ = r.resolve_linear(film)
    assert np.array_equal(read_tga(tmp_path / "linear.tga"), pixels[:, :3]) and r.splat_stats() == (0, 0, 0, 0, 0)
    assert read_pfm(tmp_path / "linear.pfm").tobytes() == np.stack([means["r"], means["g"], means["b"]], axis=1).tobytes()
    r.close()
    boxed = run_main(["--film", "pinhole", "--linear", "--filter", "box,0.5"], tmp_path / "boxed.tga")   # the identity of §3.30, end to end
    assert boxed == linear and open(tmp_path / "boxed.pfm", "rb").read() == pfm
    tent = run_main(["--film", "pinhole", "--linear", "--filter", "tent"], tmp_path / "tent.tga")
    assert len(tent) == len(linear) and tent != linear   # a filtered film is another image


def test_filter_arguments_are_checked(tmp_path):
    for args in (["--film", "pinhole", "--filter", "tent"], ["--film", "pinhole", "--linear", "--filter", "mitchell"],
                 ["--film", "pinhole", "--linear", "--filter", "tent,wide"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--filter" in r.stderr, args
