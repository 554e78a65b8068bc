"""ptss_main --film KIND --linear --carry KEYS[,maxHistory]: --ticks rounds with the luminance moments, the features of
the pixel-centre rays, the move, the features again, ptss_reproject_linear into a new film and new moments, --ticks more rounds into
them, then the usual tail. The files are the ones the Python face computes from the same calls, and the counters printed are the
call's."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, N, W
from test_gpu_linear_main import ARGS, BOUNCES, MAIN, NAME, SEED, TICKS, read_pfm, read_tga

pytestmark = pytest.mark.gpu
KEYS = "w"   # --keys: the first pose stands one step in front of the preset's camera (DESIGN.md §3.19's reason)


def python_face(keys, max_history, splat, key_rate, glare, denoise):
    """ptss_main's sequence through the Python face -> (renderer, (linear, pixels, history), the call's info)."""
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    cam = ptss.default_camera()
    for k in KEYS:
        assert ptss.move_camera(cam, k)
    params = ptss.linear_params()
    meter = ptss.meter_params(key=key_rate[0], rate=key_rate[1]) if key_rate else None
    rng = r.seed_path_rng(N, SEED)
    centre = lambda: ptss.film_camera("pinhole", W, H, cam, jitter=0)
    features = r.ray_features(r.generate_rays(centre(), rng)[0])
    film, moments = np.zeros(N, ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE), np.zeros(N, ptss.MOMENT_DTYPE)
    state, shown, info = None, None, None
    for t in range(2 * TICKS):
        if t == TICKS:   # the move
            before, features_before = centre(), features
            moved = ptss.Camera()
            C.memmove(C.byref(moved), C.byref(cam), C.sizeof(ptss.Camera))
            for k in keys:
                assert ptss.move_camera(moved, k)
            cam = moved
            features = r.ray_features(r.generate_rays(centre(), rng)[0])
            film, moments, info = r.reproject_linear(centre(), features, before, features_before, film, moments, params,
                                                     ptss.reproject_linear_params(max_history=max_history))
        film_cam = ptss.film_camera("pinhole", W, H, cam)
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True) if splat else r.generate_rays(film_cam, rng) + (None,)
        res, rng = r.trace_paths(rays, rng, BOUNCES)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=ptss.splat_filter("tent"), params=params, homed_first_pixel=0)
            moments = r.accumulate_paths_linear_stats(res, None, moments, params=params)[1]
        else:
            film, moments = r.accumulate_paths_linear_stats(res, film, moments, params=params)
        if meter is not None:
            shown = r.denoise_linear(film, W, H, moments, features, params, denoise) if denoise else film
            state = r.meter_exposure((r.meter_splat if splat and not denoise else r.meter_linear)(shown), state, params, meter)
    if meter is None:
        shown = r.denoise_linear(film, W, H, moments, features, params, denoise) if denoise else film
    resolve = r.resolve_splat if splat and not denoise else r.resolve_linear
    g = None if glare is None else (W, H, glare, r.glare_build(shown, W, H, params, glare))
    return r, resolve(shown, params=params, metered=state, glare=g), info


@pytest.mark.parametrize("extra, splat, key_rate, glare, denoise, carry, cap", [
    ([], False, None, None, None, "df", 64),
    (["--filter", "tent", "--auto-exposure", "0.18,0.5", "--glare", "--denoise-linear", "3"], True, (0.18, 0.5), ptss.glare_params(),
     ptss.denoise_linear_params(levels=3), "df,16", 16)])
def test_carry_writes_the_python_faces_files(tmp_path, extra, splat, key_rate, glare, denoise, carry, cap):
    out = tmp_path / "shot.tga"
    p = subprocess.run([MAIN] + ARGS + ["--keys", KEYS, "--film", "pinhole", "--linear"] + extra + ["--carry", carry, "--out", str(out)], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    r, (linear, pixels, _), info = python_face(carry.split(",")[0], cap, splat, key_rate, glare, denoise)
    assert r.reproject_linear_launches() == 1 and 0 < int(info["seeded"]) < N
    line = [l for l in p.stdout.splitlines() if l.startswith("carry:")]
    assert line == ["carry: seeded %d offFilm %d noTap %d noVariance %d" % tuple(int(info[k]) for k in ("seeded", "offFilm", "noTap", "noVariance"))]
    assert np.array_equal(read_tga(out), pixels[:, :3]) and 0 < int(pixels[:, :3].max())
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0
    r.close()


def test_carry_arguments_are_checked(tmp_path):
    base = ["--film", "pinhole", "--linear"]
    for args in (["--film", "pinhole", "--carry", "df"], ["--carry", "df"], base + ["--carry", ""], base + ["--carry", "dx"], base + ["--carry", "df,0"],
                 base + ["--carry", "df,8388608"], base + ["--carry", "df,x"], base + ["--carry", "df,-3"], base + ["--adaptive-linear", "2", "--carry", "df"],
                 base + ["--ticks", "0", "--carry", "df"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--carry" in r.stderr, args
