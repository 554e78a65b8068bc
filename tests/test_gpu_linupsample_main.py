"""ptss_main --film KIND --linear [exposure] --upscale-linear F: the film is traced (and, with --denoise-linear, denoised)
at the given size, the features are those of the centre rays of the same film camera at both sizes, ptss_upsample_linear makes the
large linear film, and the meter (every round), the glare, the resolve, image.tga and image.pfm work on it. The files are F times the
size and hold the bytes the Python face computes from the same calls; the option is refused without --linear."""
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, N, W
from test_gpu_linear_main import ARGS, BOUNCES, MAIN, NAME, SEED, TICKS

pytestmark = pytest.mark.gpu


def read_tga(path, w, h):
    b = open(path, "rb").read()
    assert b[2] == 2 and b[16] == 24 and (b[12] | (b[13] << 8), b[14] | (b[15] << 8)) == (w, h)
    return np.frombuffer(b, np.uint8, w * h * 3, 18).reshape(h * w, 3)[:, ::-1]   # BGR -> RGB, bottom-up order kept


def read_pfm(path, w, h):
    b = open(path, "rb").read()
    header = b"PF\n%d %d\n-1.0\n" % (w, h)
    assert b.startswith(header) and len(b) == len(header) + w * h * 12
    return np.frombuffer(b, "<f4", w * h * 3, len(header)).reshape(h * w, 3)


def python_face(film_kind, f, splat, key_rate, glare, denoise):
    """The rounds of ptss_main through the Python face -> (renderer, (linear, pixels, history), the counters)."""
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    cam = ptss.default_camera()
    film_cam = ptss.film_camera(film_kind, W, H, cam)
    params = ptss.linear_params()
    meter = ptss.meter_params(key=key_rate[0], rate=key_rate[1]) if key_rate else None
    up = ptss.upsample_linear_params(f, wrap_x=film_kind == "equirect")
    centre = lambda s: r.ray_features(r.generate_rays(ptss.film_camera(film_kind, s * W, s * H, cam, jitter=0), r.seed_path_rng(s * s * N, SEED))[0])
    flo, fhi = centre(1), centre(f)
    rng = r.seed_path_rng(N, SEED)
    film, moments = np.zeros(N, ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE), np.zeros(N, ptss.MOMENT_DTYPE)
    state, large = None, None
    info = np.zeros(1, ptss.UPSAMPLE_LINEAR_INFO_DTYPE)[0]

    def enlarge(info):
        small = r.denoise_linear(film, W, H, moments, flo, params, denoise) if denoise is not None else film
        return r.upsample_linear(small, W, H, flo, fhi, params, up, info=info)

    for _ in range(TICKS):
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True) if splat else r.generate_rays(film_cam, rng) + (None,)
        res, rng = r.trace_paths(rays, rng, BOUNCES)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=ptss.splat_filter("tent"), params=params, homed_first_pixel=0)
            if denoise is not None:
                moments = r.accumulate_paths_linear_stats(res, None, moments, params=params)[1]
        elif denoise is not None:
            film, moments = r.accumulate_paths_linear_stats(res, film, moments, params=params)
        else:
            film = r.accumulate_paths_linear(res, film, params=params)
        if meter is not None:
            large, info = enlarge(info)
            state = r.meter_exposure(r.meter_linear(large), state, params, meter)
    if meter is None:
        large, info = enlarge(info)
    if glare is None:
        return r, r.resolve_linear(large, params=params, metered=state), info
    return r, r.resolve_linear(large, params=params, metered=state, glare=(f * W, f * H, glare, r.glare_build(large, f * W, f * H, params, glare))), info


@pytest.mark.parametrize("film_kind, f, extra, key_rate, glare, denoise", [
    ("pinhole", 2, [], None, None, None),
    ("equirect", 2, [], None, None, None),
    ("pinhole", 2, ["--denoise-linear", "3", "--auto-exposure", "0.18,0.5", "--glare"], (0.18, 0.5), ptss.glare_params(), ptss.denoise_linear_params(levels=3)),
    ("equirect", 3, ["--filter", "tent", "--glare", "0.5,0.25,4"], None, ptss.glare_params(strength=0.5, threshold=0.25, levels=4), None)])
def test_upscale_linear_writes_the_python_faces_files_at_f_times_the_size(tmp_path, film_kind, f, extra, key_rate, glare, denoise):
    out = tmp_path / "shot.tga"
    run = subprocess.run([MAIN] + ARGS + ["--film", film_kind, "--linear"] + extra + ["--upscale-linear", str(f), "--out", str(out)], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    r, (linear, pixels, _), info = python_face(film_kind, f, "--filter" in extra, key_rate, glare, denoise)
    assert r.upsample_linear_launches() == (TICKS if key_rate else 1)
    assert np.array_equal(read_tga(out, f * W, f * H), pixels[:, :3]) and 0 < int(pixels[:, :3].max())
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm", f * W, f * H).tobytes() == means.tobytes() and means.max() > 0
    line = "upscale-linear: factor %d filtered %d fallback %d empty %d" % (f, info["filtered"], info["fallback"], info["empty"])
    assert line in run.stdout and int(info["filtered"]) > 0
    r.close()


def test_upscale_linear_arguments_are_checked(tmp_path):
    for args in (["--film", "pinhole", "--upscale-linear", "2"], ["--upscale-linear", "2"], ["--film", "pinhole", "--linear", "--upscale-linear", "5"],
                 ["--film", "pinhole", "--linear", "--upscale-linear", "0"], ["--film", "pinhole", "--linear", "--upscale-linear", "2", "--carry", "d"],
                 ["--film", "pinhole", "--linear", "--upscale-linear", "2", "--adaptive-linear", "2"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--upscale-linear" in r.stderr, args
