"""ptss_main --film KIND --linear [exposure] --glare [strength[,threshold[,levels]]]: after the last round the glare
pyramid of the finished film is built and the glare resolve makes the screenshot and the PFM, at the meter's exposure where
--auto-exposure keeps a state. The files are the ones the Python face computes from the same calls; without the flag the program writes
the bytes of --linear alone."""
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


def python_face(splat, refill, compensation, key_rate, glare):
    """The rounds of ptss_main through the Python face -> (renderer, film, the meter's state or None, (linear, pixels, history))."""
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params = ptss.linear_params(exposure=1.0 if compensation is None else compensation)
    meter = ptss.meter_params(key=key_rate[0], rate=key_rate[1]) if key_rate else None
    rng, film = r.seed_path_rng(N, SEED), np.zeros(N, ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE)
    state = None
    for _ in range(TICKS):
        rays, rng, pos = r.generate_rays(film_cam, rng, positions=True) if splat else r.generate_rays(film_cam, rng) + (None,)
        res, rng = r.trace_paths(rays, rng, BOUNCES, schedule=ptss.PATHS_REFILL if refill else None)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=ptss.splat_filter("tent"), params=params, homed_first_pixel=0)
        else:
            film = r.accumulate_paths_linear(res, film, params=params)
        if meter is not None:
            state = r.meter_exposure((r.meter_splat if splat else r.meter_linear)(film), state, params, meter)
    resolve = r.resolve_splat if splat else r.resolve_linear
    if glare is None:
        return r, film, state, resolve(film, params=params, metered=state)
    pyramid = r.glare_build(film, W, H, params, glare)
    return r, film, state, resolve(film, params=params, metered=state, glare=(W, H, glare, pyramid))


@pytest.mark.parametrize("extra, compensation, key_rate, glare_arg, glare_kw", [
    ([], None, None, None, dict()),
    (["--filter", "tent"], None, None, "0.3", dict(strength=0.3)),
    ([], 0.5, (0.18, 0.5), "0.5,0.25,4", dict(strength=0.5, threshold=0.25, levels=4)),
    (["--filter", "tent", "--refill"], 2.0, (0.3, 0.25), "1,0,8", dict(strength=1.0, threshold=0.0, levels=8))])
def test_glare_writes_the_python_faces_files(tmp_path, extra, compensation, key_rate, glare_arg, glare_kw):
    args = ["--film", "pinhole", "--linear"] + ([str(compensation)] if compensation is not None else []) + extra
    args += ["--auto-exposure", "%g,%g" % key_rate] if key_rate else []
    args += ["--glare"] + ([glare_arg] if glare_arg else [])
    run_main(args, tmp_path / "shot.tga")
    glare = ptss.glare_params(**glare_kw)
    r, film, state, (linear, pixels, _) = python_face("--filter" in extra, "--refill" in extra, compensation, key_rate, glare)
    assert r.glare_launches()[0::2] == (1, 1) and (state is None) == (key_rate is None)
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3]) and 0 < int(pixels[:, :3].max())
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0   # the means the glare resolve shows, unexposed
    r.close()


def test_without_the_flag_the_bytes_of_linear_alone(tmp_path):
    plain, _ = run_main(["--film", "pinhole", "--linear", "0.5"], tmp_path / "plain.tga")
    r, _, _, (linear, pixels, _) = python_face(False, False, 0.5, None, None)
    assert np.array_equal(read_tga(tmp_path / "plain.tga"), pixels[:, :3]) and r.glare_launches() == (0, 0, 0)
    r.close()
    glared, _ = run_main(["--film", "pinhole", "--linear", "0.5", "--glare", "1"], tmp_path / "glared.tga")
    assert len(glared) == len(plain) and glared != plain   # the mean of a neighbourhood is another image
    zero, _ = run_main(["--film", "pinhole", "--linear", "0.5", "--glare", "0"], tmp_path / "zero.tga")
    assert zero == plain and open(tmp_path / "zero.pfm", "rb").read() == open(tmp_path / "plain.pfm", "rb").read()   # strength 0: the plain resolve


def test_glare_arguments_are_checked(tmp_path):
    for args in (["--film", "pinhole", "--glare"], ["--glare"], ["--film", "pinhole", "--linear", "--glare", "1.5"],
                 ["--film", "pinhole", "--linear", "--glare", "0.5,0,9"], ["--film", "pinhole", "--linear", "--glare", "0.5,0,0"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--glare" in r.stderr, args
