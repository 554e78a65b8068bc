"""ptss_main --film KIND --adaptive ROUNDS[,threshold]: the --ticks uniform rounds keep second moments, then ROUNDS
planned rounds go where ptss_plan_samples sends them. The planned image is the one the Python face computes from the same calls, the
printed ptss_plan_info is the device's, and ROUNDS = 0 writes the bytes of the run without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, N, SCENES, W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
NAME, BOUNCES, TICKS = "mixed", 4, 3
SEED = SCENES[NAME][3]
ARGS = ["--preset", NAME, "--size", f"{W}x{H}", "--ticks", str(TICKS), "--bounces", str(BOUNCES), "--seed", str(SEED), "--quiet"]
INFO = re.compile(r"adaptive: rounds (\d+) totalWeight (\d+) activePixels (\d+) unsampledPixels (\d+) cappedPixels (\d+) uniform (\d+)")


def read_tga(path):
    b = open(path, "rb").read()
    w, h = b[12] | (b[13] << 8), b[14] | (b[15] << 8)
    assert b[2] == 2 and b[16] == 24 and (w, h) == (W, H)
    return np.frombuffer(b, np.uint8, w * h * 3, 18).reshape(h * w, 3)[:, ::-1]   # BGR -> RGB, bottom-up order kept


def run_main(args, out):
    r = subprocess.run([MAIN] + ARGS + args + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return open(out, "rb").read(), r.stdout


@pytest.mark.parametrize("extra", [[], ["--refill", "--denoise", "2"]])
def test_adaptive_rounds_write_the_python_faces_image(tmp_path, extra):
    threshold = 0.75
    _, stdout = run_main(["--film", "pinhole", "--adaptive", "2,%g" % threshold] + extra, tmp_path / "shot.tga")
    m = INFO.search(stdout)
    assert m, stdout
    printed = dict(zip(("rounds", "totalWeight", "activePixels", "unsampledPixels", "cappedPixels", "uniform"), (int(v) for v in m.groups())))
    assert printed["rounds"] == 2 and printed["activePixels"] <= N
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params = ptss.plan_params(min_samples=TICKS, threshold=threshold)
    rng, film, moments, index = r.seed_path_rng(N, SEED), np.zeros(N, ptss.FILM_DTYPE), np.zeros(N, np.uint64), None
    for k in range(TICKS + 2):
        rays, rng = r.generate_rays(film_cam, rng, index=index)
        res, rng = r.trace_paths(rays, rng, BOUNCES, schedule=ptss.PATHS_REFILL if extra else None)
        film, moments, pixels, history = r.accumulate_paths_stats(res, film, moments, index=index, pixels=True if index is None else pixels,
                                                                  history=True if index is None else history)
        if k >= TICKS - 1:
            _, index, info = r.plan_samples(film, moments, N, params)
    assert {k: printed[k] for k in info} == info
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3])
    if extra:
        film_cam.jitter = 0
        feat = r.ray_features(r.generate_rays(film_cam, rng)[0])
        assert np.array_equal(read_tga(tmp_path / "shot_denoised.tga"), r.denoise_history(history=history, features=feat, levels=2)[:, :3])
    r.close()


def test_no_planned_round_writes_the_plain_films_bytes(tmp_path):
    plain, _ = run_main(["--film", "pinhole"], tmp_path / "plain.tga")
    none, stdout = run_main(["--film", "pinhole", "--adaptive", "0"], tmp_path / "none.tga")
    assert none == plain
    m = INFO.search(stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(3)) <= N and int(m.group(4)) == 0   # after --ticks rounds no pixel is unsampled


def test_adaptive_arguments_are_checked(tmp_path):
    for args in (["--adaptive", "2"], ["--film", "pinhole", "--adaptive", "-1"], ["--film", "pinhole", "--adaptive", "x"], ["--film", "pinhole", "--adaptive", "2,-1"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--adaptive" in r.stderr, args
