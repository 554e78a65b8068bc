"""ptss_main --film KIND --linear --adaptive-linear ROUNDS[,threshold[,floor]]: the --ticks uniform rounds keep luminance
moments, then ROUNDS planned rounds go where ptss_plan_samples_linear sends them. The files are the ones the Python face computes from the
same calls, the printed ptss_plan_info is the device's, and ROUNDS = 0 writes the bytes of the run without the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import ptss
from linstats_common import zero_moments
from path_query_common import H, N, SCENES, W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
NAME, BOUNCES, TICKS = "mixed", 4, 3
SEED = SCENES[NAME][3]
ARGS = ["--preset", NAME, "--size", f"{W}x{H}", "--ticks", str(TICKS), "--bounces", str(BOUNCES), "--seed", str(SEED), "--quiet"]
INFO = re.compile(r"adaptive-linear: rounds (\d+) totalWeight (\d+) activePixels (\d+) unsampledPixels (\d+) cappedPixels (\d+) uniform (\d+)")


def read_tga(path):
    b = open(path, "rb").read()
    w, h = b[12] | (b[13] << 8), b[14] | (b[15] << 8)
    assert b[2] == 2 and b[16] == 24 and (w, h) == (W, H)
    return np.frombuffer(b, np.uint8, w * h * 3, 18).reshape(h * w, 3)[:, ::-1]   # BGR -> RGB, bottom-up order kept


def read_pfm(path):
    b = open(path, "rb").read()
    header = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert b.startswith(header) and len(b) == len(header) + W * H * 12
    return np.frombuffer(b, "<f4", W * H * 3, len(header)).reshape(H * W, 3)   # bottom row first: the film's own order


def run_main(args, out):
    r = subprocess.run([MAIN] + ARGS + args + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return open(out, "rb").read(), r.stdout


@pytest.mark.parametrize("extra", [[], ["--refill"]])
def test_planned_rounds_write_the_python_faces_files(tmp_path, extra):
    threshold = 0.05
    _, stdout = run_main(["--film", "pinhole", "--linear", "--adaptive-linear", "2,%g" % threshold] + extra, tmp_path / "shot.tga")
    m = INFO.search(stdout)
    assert m, stdout
    printed = dict(zip(("rounds", "totalWeight", "activePixels", "unsampledPixels", "cappedPixels", "uniform"), (int(v) for v in m.groups())))
    assert printed["rounds"] == 2 and 0 < printed["activePixels"] <= N
    r = ptss.Renderer(ptss.Scene(NAME), W, H, max_iterations=BOUNCES, seed=SEED)
    film_cam = ptss.film_camera("pinhole", W, H, ptss.default_camera())
    params, plan = ptss.linear_params(), ptss.linear_plan_params(min_samples=TICKS, threshold=threshold)
    rng, film, moments, index = r.seed_path_rng(N, SEED), np.zeros(N, ptss.LINEAR_DTYPE), zero_moments(N), None
    for k in range(TICKS + 2):
        rays, rng = r.generate_rays(film_cam, rng, index=index)
        res, rng = r.trace_paths(rays, rng, BOUNCES, schedule=ptss.PATHS_REFILL if extra else None)
        film, moments = r.accumulate_paths_linear_stats(res, film, moments, index=index, params=params)
        if k >= TICKS - 1:
            _, index, info = r.plan_samples_linear(moments, N, params, plan)
    assert {k: printed[k] for k in info} == info
    assert int(film["samples"].sum()) == (TICKS + 2) * N and film["samples"].max() > TICKS
    linear, pixels, _ = r.resolve_linear(film, params=params)
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3])
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0
    r.close()


def test_no_planned_round_writes_the_linear_films_bytes(tmp_path):
    plain, _ = run_main(["--film", "pinhole", "--linear"], tmp_path / "plain.tga")
    none, stdout = run_main(["--film", "pinhole", "--linear", "--adaptive-linear", "0"], tmp_path / "none.tga")
    assert none == plain and open(tmp_path / "none.pfm", "rb").read() == open(tmp_path / "plain.pfm", "rb").read()
    m = INFO.search(stdout)
    assert m and int(m.group(1)) == 0 and int(m.group(3)) <= N and int(m.group(4)) == 0   # after --ticks rounds no pixel is unsampled


def test_beside_the_filter_the_meter_and_the_glare(tmp_path):
    """--adaptive-linear with --filter, --auto-exposure and --glare: no planned round writes the bytes of the run without the flag, two
    planned rounds run, report their plan and write another image of the same size."""
    flags = ["--film", "pinhole", "--linear", "--filter", "tent", "--auto-exposure", "--glare"]
    plain, _ = run_main(flags, tmp_path / "plain.tga")
    none, stdout = run_main(flags + ["--adaptive-linear", "0"], tmp_path / "none.tga")
    assert none == plain and open(tmp_path / "none.pfm", "rb").read() == open(tmp_path / "plain.pfm", "rb").read()
    assert INFO.search(stdout)
    two, stdout = run_main(flags + ["--adaptive-linear", "2,0.05,0.03125"], tmp_path / "two.tga")
    m = INFO.search(stdout)
    assert m and int(m.group(1)) == 2 and 0 < int(m.group(3)) <= N and int(m.group(4)) == 0
    assert len(two) == len(plain) and two != plain and read_pfm(tmp_path / "two.pfm").max() > 0


def test_adaptive_linear_arguments_are_checked(tmp_path):
    for args in (["--film", "pinhole", "--adaptive-linear", "2"], ["--adaptive-linear", "2"], ["--film", "pinhole", "--linear", "--adaptive-linear", "-1"],
                 ["--film", "pinhole", "--linear", "--adaptive-linear", "x"], ["--film", "pinhole", "--linear", "--adaptive-linear", "2,-1"],
                 ["--film", "pinhole", "--linear", "--adaptive-linear", "2,0.1,0"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--adaptive-linear" in r.stderr, args
