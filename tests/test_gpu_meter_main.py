"""ptss_main --film KIND --linear [compensation] --auto-exposure [key[,rate]]: after each round the film is metered
on the device, the meter's state updated and the film resolved at the state's exposure; the program prints the final state. The files and
the state are the ones the Python face computes from the same calls; without the flag the program writes the bytes of --linear alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, N, SCENES, W
from test_gpu_linear_main import ARGS, BOUNCES, MAIN, NAME, SEED, TICKS, read_pfm, read_tga

pytestmark = pytest.mark.gpu


def run_main(args, out):
    r = subprocess.run([MAIN] + ARGS + args + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return open(out, "rb").read(), r.stdout


@pytest.mark.parametrize("extra, compensation, key_rate", [([], None, None), (["--filter", "tent"], None, None), ([], 0.5, (0.18, 0.5)),
                                                           (["--filter", "tent", "--refill"], 2.0, (0.3, 0.25))])
def test_auto_exposure_writes_the_python_faces_files(tmp_path, extra, compensation, key_rate):
    args = ["--film", "pinhole", "--linear"] + ([str(compensation)] if compensation is not None else []) + extra + ["--auto-exposure"]
    args += ["%g,%g" % key_rate] if key_rate else []
    _, stdout = run_main(args, tmp_path / "shot.tga")
    splat = "--filter" in extra
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params = ptss.linear_params(exposure=1.0 if compensation is None else compensation)
    meter = ptss.meter_params(key=key_rate[0], rate=key_rate[1]) if key_rate else ptss.meter_params()
    rng, film = r.seed_path_rng(N, SEED), np.zeros(N, ptss.SPLAT_DTYPE if splat else ptss.LINEAR_DTYPE)
    state = None
    for _ in range(TICKS):   # after each round: a zeroed histogram, meter, update, metered resolve
        if splat:
            rays, rng, pos = r.generate_rays(film_cam, rng, positions=True)
        else:
            rays, rng = r.generate_rays(film_cam, rng)
        res, rng = r.trace_paths(rays, rng, BOUNCES, schedule=ptss.PATHS_REFILL if "--refill" in extra else None)
        if splat:
            film = r.splat_paths(res, pos, film, W, H, filter=ptss.splat_filter("tent"), params=params, homed_first_pixel=0)
            state = r.meter_exposure(r.meter_splat(film), state, params, meter)
            linear, pixels, _ = r.resolve_splat(film, params=params, metered=state)
        else:
            film = r.accumulate_paths_linear(res, film, params=params)
            state = r.meter_exposure(r.meter_linear(film), state, params, meter)
            linear, pixels, _ = r.resolve_linear(film, params=params, metered=state)
    assert r.meter_launches() == (TICKS, TICKS, TICKS)
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3]) and 0 < int(pixels[:, :3].max())
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0   # the means stay unexposed
    m = re.search(r"auto-exposure: exposure (\S+) target (\S+) meanLog2 (\S+) updates (\d+) metered (\d+) black (\d+) counted (\d+) sumLog (\d+)", stdout)
    assert m, stdout
    s = state[0]
    assert [np.float32(m.group(k)) for k in (1, 2, 3)] == [s["exposure"], s["target"], s["meanLog2"]]   # %.9g round-trips a float32
    assert [int(m.group(k)) for k in (4, 5, 6, 7, 8)] == [int(s[f]) for f in ("updates", "metered", "black", "counted", "sumLog")]
    assert int(s["updates"]) == TICKS and int(s["metered"]) + int(s["black"]) == N
    r.close()


def test_without_the_flag_the_bytes_of_linear_alone(tmp_path):
    plain, stdout = run_main(["--film", "pinhole", "--linear", "0.5"], tmp_path / "plain.tga")
    assert "auto-exposure" not in stdout
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params = ptss.linear_params(exposure=0.5)
    rng, film = r.seed_path_rng(N, SEED), np.zeros(N, ptss.LINEAR_DTYPE)
    for _ in range(TICKS):
        rays, rng = r.generate_rays(film_cam, rng)
        res, rng = r.trace_paths(rays, rng, BOUNCES)
        film = r.accumulate_paths_linear(res, film, params=params)
    linear, pixels, _ = r.resolve_linear(film, params=params)
    assert np.array_equal(read_tga(tmp_path / "plain.tga"), pixels[:, :3]) and r.meter_launches() == (0, 0, 0)
    r.close()
    metered, _ = run_main(["--film", "pinhole", "--linear", "0.5", "--auto-exposure"], tmp_path / "metered.tga")
    assert len(metered) == len(plain) and metered != plain   # another exposure is another image
    assert open(tmp_path / "metered.pfm", "rb").read() == open(tmp_path / "plain.pfm", "rb").read()   # the linear means do not depend on it


def test_auto_exposure_arguments_are_checked(tmp_path):
    for args in (["--film", "pinhole", "--auto-exposure"], ["--auto-exposure"], ["--film", "pinhole", "--linear", "--auto-exposure", "0"],
                 ["--film", "pinhole", "--linear", "--auto-exposure", "0.18,1.5"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--auto-exposure" in r.stderr, args
