"""ptss_main --bake [texelsPerUnit[,samples[,passes]]]: the atlas of the preset's triangles at --size's width, streams
from ptss_seed_path_rng, per sample generate (cosine) -> ptss_trace_paths -> ptss_accumulate_paths_linear indexed by texel, the gutter
fills, ptss_resolve_linear. The file is the one the Python loop of the same calls computes with the host probes standing in for
generate, accumulate, dilate and resolve; only the trace stays on the device."""
import os
import subprocess

import numpy as np
import pytest

import ptss

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
PRESET, WIDTH, BOUNCES, SEED = "cornell", 40, 3, 0xBA4E


def read_pfm(path, width):
    b = open(path, "rb").read()
    head, size, scale, body = b.split(b"\n", 3)
    w, h = (int(v) for v in size.split())
    assert head == b"PF" and w == width and scale == b"-1.0" and len(body) == w * h * 12
    return np.frombuffer(body, "<f4").reshape(h * w, 3), h   # bottom row first: the atlas' own order


def run_bake(option, out, extra=()):
    args = ["--preset", PRESET, "--size", f"{WIDTH}x8", "--bounces", str(BOUNCES), "--seed", str(SEED), "--quiet", "--bake"] + ([option] if option else [])
    r = subprocess.run([MAIN] + args + list(extra) + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout


@pytest.mark.parametrize("option, texels_per_unit, samples, passes", [("0.75,3,2", 0.75, 3, 2), ("0.5,2,0", 0.5, 2, 0)])
def test_bake_writes_the_shadow_loops_file(tmp_path, option, texels_per_unit, samples, passes):
    out = tmp_path / "lightmap.pfm"
    stdout = run_bake(option, out)
    scene = ptss.Scene(PRESET)
    tri, sph = ptss.scene_records(scene)
    points, texels, height = ptss.surface_atlas(tri, texels_per_unit, WIDTH, 1, min(64, WIDTH))
    assert f"bake: atlas {WIDTH} x {height}, {len(points)} texels of {len(tri)} triangles, {samples} samples, {passes} passes, rejected 0" in stdout
    r = ptss.Renderer(scene, WIDTH, 8, max_iterations=BOUNCES, seed=SEED)
    try:
        params, cosine = ptss.linear_params(), ptss.surface_params("cosine")
        film = np.zeros(WIDTH * height, dtype=ptss.LINEAR_DTYPE)
        rng = r.seed_path_rng(len(points), SEED)
        for _ in range(samples):
            rays, rng, _, rejected = ptss.probe_surface_rays(tri, sph, points, rng, cosine)
            assert rejected == 0
            results, rng = r.trace_paths(rays, rng, BOUNCES)
            film, dropped = ptss.probe_accumulate_linear(results, film, index=texels, params=params)
            assert dropped == 0
        for _ in range(passes):
            film = ptss.probe_dilate_linear(film, WIDTH, height)
        linear = ptss.probe_resolve_linear(film, params=params, pixels=None, history=None)[0]
    finally:
        r.close()
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    got, got_height = read_pfm(out, WIDTH)
    assert got_height == height and got.tobytes() == means.tobytes()
    assert means.max() > 0 and (film["samples"][texels] >= samples).all()   # the box's light reaches the map
    if passes:
        assert (film["samples"] > 0).sum() > len(points)                   # the gutters were filled


def test_bake_defaults_and_refused_arguments(tmp_path):
    stdout = run_bake(None, tmp_path / "default.pfm", extra=["--bounces", "1"])
    assert ", 16 samples, 1 passes, rejected 0" in stdout and read_pfm(tmp_path / "default.pfm", WIDTH)[0].max() >= 0
    for args in (["--bake", "0"], ["--bake", "1,0"], ["--bake", "1,2,65"], ["--bake", "--film", "pinhole"], ["--bake", "--denoise"], ["--bake", "--gpus", "1"]):
        r = subprocess.run([MAIN, "--preset", PRESET, "--size", f"{WIDTH}x8", "--quiet"] + args + ["--out", str(tmp_path / "x.pfm")], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 2 and "--bake" in r.stderr, (args, r.stderr)
