"""ptss_main --film KIND --linear [exposure] --denoise-linear [levels[,sigmaLuminance]]: the rounds keep the luminance
moments, the features are those of the pixel-centre rays, and the denoised film is what the meter (every round), the glare, the resolve
and the PFM read. The files are the ones the Python face computes from the same calls; levels 0 and the absent flag write the same
bytes."""
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, N, W
from test_gpu_linear_main import ARGS, BOUNCES, MAIN, NAME, SEED, TICKS, read_pfm, read_tga

pytestmark = pytest.mark.gpu


def run_main(args, out):
    r = subprocess.run([MAIN] + ARGS + args + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return open(out, "rb").read(), r.stdout


def python_face(splat, key_rate, glare, denoise):
    """The rounds of ptss_main through the Python face -> (renderer, (linear, pixels, history))."""
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    cam = ptss.default_camera()
    film_cam = ptss.film_camera("pinhole", W, H, cam)
    params = ptss.linear_params()
    meter = ptss.meter_params(key=key_rate[0], rate=key_rate[1]) if key_rate else None
    rng = r.seed_path_rng(N, SEED)
    features = r.ray_features(r.generate_rays(ptss.film_camera("pinhole", W, H, cam, jitter=0), rng)[0])
    film, moments = np.zeros(N, ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE), np.zeros(N, ptss.MOMENT_DTYPE)
    state, clean = None, None
    for _ in range(TICKS):
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True) if splat else r.generate_rays(film_cam, rng) + (None,)
        res, rng = r.trace_paths(rays, rng, BOUNCES)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=ptss.splat_filter("tent"), params=params, homed_first_pixel=0)
            moments = r.accumulate_paths_linear_stats(res, None, moments, params=params)[1]
        else:
            film, moments = r.accumulate_paths_linear_stats(res, film, moments, params=params)
        if meter is not None:
            clean = r.denoise_linear(film, W, H, moments, features, params, denoise)
            state = r.meter_exposure(r.meter_linear(clean), state, params, meter)
    if meter is None:
        clean = r.denoise_linear(film, W, H, moments, features, params, denoise)
    if glare is None:
        return r, r.resolve_linear(clean, params=params, metered=state)
    return r, r.resolve_linear(clean, params=params, metered=state, glare=(W, H, glare, r.glare_build(clean, W, H, params, glare)))


@pytest.mark.parametrize("extra, key_rate, glare, arg, kw", [
    ([], None, None, "3", dict(levels=3)),
    (["--filter", "tent", "--auto-exposure", "0.18,0.5", "--glare"], (0.18, 0.5), ptss.glare_params(), "3", dict(levels=3)),
    (["--glare", "0.5,0.25,4"], None, ptss.glare_params(strength=0.5, threshold=0.25, levels=4), "4,1.5", dict(levels=4, sigma_luminance=1.5)),
    ([], None, None, None, dict())])
def test_denoise_linear_writes_the_python_faces_files(tmp_path, extra, key_rate, glare, arg, kw):
    args = ["--film", "pinhole", "--linear"] + extra + ["--denoise-linear"] + ([arg] if arg else [])
    run_main(args, tmp_path / "shot.tga")
    r, (linear, pixels, _) = python_face("--filter" in extra, key_rate, glare, ptss.denoise_linear_params(**kw))
    rounds = TICKS if key_rate else 1
    assert r.denoise_linear_launches()[0] == rounds
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3]) and 0 < int(pixels[:, :3].max())
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0
    r.close()


def test_levels_zero_writes_the_bytes_of_the_run_without_the_flag(tmp_path):
    for k, extra in enumerate(([], ["--filter", "tent"], ["--auto-exposure", "--glare", "0.3"])):
        base = ["--film", "pinhole", "--linear", "0.5"] + extra
        plain, _ = run_main(base, tmp_path / f"plain{k}.tga")
        zero, _ = run_main(base + ["--denoise-linear", "0"], tmp_path / f"zero{k}.tga")
        assert zero == plain and open(tmp_path / f"zero{k}.pfm", "rb").read() == open(tmp_path / f"plain{k}.pfm", "rb").read(), extra
    filtered, _ = run_main(["--film", "pinhole", "--linear", "0.5", "--denoise-linear"], tmp_path / "filtered.tga")
    assert len(filtered) == len(plain) and filtered != open(tmp_path / "plain0.tga", "rb").read()   # the filter changes the image


def test_denoise_linear_arguments_are_checked(tmp_path):
    for args in (["--film", "pinhole", "--denoise-linear"], ["--denoise-linear"], ["--film", "pinhole", "--linear", "--denoise-linear", "7"],
                 ["--film", "pinhole", "--linear", "--denoise-linear", "-1"], ["--film", "pinhole", "--linear", "--denoise-linear", "3,0"],
                 ["--film", "pinhole", "--linear", "--denoise-linear", "3,-2"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--denoise-linear" in r.stderr, args
