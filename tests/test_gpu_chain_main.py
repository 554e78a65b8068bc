"""ptss_main --bake ... --bake-view [filter] --view-steps N: the view's centre rays go through ptss_intersect_chain and
the rows come from ptss_lookup_lightmap_chain. With N = 2 the view file is the one the shadow loop of the probes computes — the chain as
a composition of ptss_intersect and ptss_probe_specular_link, then ptss_probe_lookup_lightmap_chain and the host resolve —; N = 0
writes the files and the lines of the run without the flag."""
import os
import subprocess

import numpy as np
import pytest

import ptss
from lightmap_common import read_pfm
from test_gpu_chain import composed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
PRESET, WIDTH, HEIGHT, BOUNCES, SEED = "mixed", 64, 48, 3, 0xBA4E
ARGS = ["--preset", PRESET, "--size", f"{WIDTH}x{HEIGHT}", "--bounces", str(BOUNCES), "--seed", str(SEED), "--quiet", "--bake", "1.5,2,2", "--bake-view",
        "bilinear"]


def run_main(tmp_path, tag, extra):
    out = tmp_path / f"{tag}.pfm"
    run = subprocess.run([MAIN] + ARGS + extra + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    with open(out, "rb") as f, open(tmp_path / f"{tag}_view.pfm", "rb") as g:
        return run.stdout, f.read(), g.read()


def test_view_steps_two_writes_the_shadow_loops_file(tmp_path):
    stdout, _, _ = run_main(tmp_path, "two", ["--view-steps", "2"])
    scene = ptss.Scene(PRESET)
    tri, sph = ptss.scene_records(scene)
    bt, bs, points, texels, height = ptss.surface_atlas_blocks(tri, sph, 1.5, WIDTH, 1, WIDTH // 2)
    r = ptss.Renderer(scene, WIDTH, HEIGHT, max_iterations=BOUNCES, seed=SEED)
    try:
        film, cosine = ptss.linear_params(), ptss.surface_params("cosine")
        baked = np.zeros(WIDTH * height, dtype=ptss.LINEAR_DTYPE)
        rng = r.seed_path_rng(len(points), SEED)
        for _ in range(2):
            rays, rng, _, rejected = ptss.probe_surface_rays(tri, sph, points, rng, cosine)
            assert rejected == 0
            results, rng = r.trace_paths(rays, rng, BOUNCES)
            baked = ptss.probe_accumulate_linear(results, baked, index=texels, params=film)[0]
        for _ in range(2):
            baked = ptss.probe_dilate_linear(baked, WIDTH, height)
        centre = ptss.film_camera("pinhole", WIDTH, HEIGHT, jitter=0)
        view_rays = ptss.probe_film_rays(centre, np.zeros((WIDTH * HEIGHT, 6), np.uint32))[0]
        view_rays = np.ascontiguousarray(view_rays).view(np.float32).reshape(-1, 8)
        hits, chain, seen = composed(r, scene.desc, view_rays, 2)
        first = r.intersect(view_rays)
    finally:
        r.close()
    assert seen["mirrored"] > 0 and seen["refracted"] > 0 and (chain["steps"] == 2).any()
    params = ptss.lightmap_params(WIDTH, height, "bilinear", modulate=True, emission=True)
    view, info = ptss.probe_lookup_lightmap_chain(scene, hits, chain, baked, params, bt, bs, film=film)
    assert f"bake view: {WIDTH} x {HEIGHT}, bilinear, 22 sphere blocks, filtered {info[0]}, empty {info[1]}, no block {info[2]}, rejected {info[3]}" in stdout
    links, behind = int(chain["steps"].sum()), int((chain["steps"] > 0).sum())
    assert f"view steps: at most 2, {links} links followed, {behind} of {WIDTH * HEIGHT} pixels seen through a mirror or glass" in stdout, stdout
    linear = ptss.probe_resolve_linear(view, params=film, pixels=None, history=None)[0]
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    got, got_rows = read_pfm(tmp_path / "two_view.pfm", WIDTH)
    assert got_rows == HEIGHT and got.tobytes() == means.tobytes()
    # and it is not the Lambert view: pixels whose first hit has no diffuse lobe were black there and carry light here
    plain, _ = ptss.probe_lookup_lightmap(scene, first, baked, params, bt, bs, film=film)
    was_black = (chain["steps"] > 0) & (plain["r"] == 0) & (plain["g"] == 0) & (plain["b"] == 0)
    assert was_black.any() and (view["r"][was_black] > 0).any()


def test_view_steps_zero_writes_todays_files(tmp_path):
    plain = run_main(tmp_path, "plain", [])
    zero = run_main(tmp_path, "zero", ["--view-steps", "0"])
    assert zero[1] == plain[1] and zero[2] == plain[2]
    lines = lambda text: [line for line in text.splitlines() if line.startswith("bake")]
    assert lines(zero[0]) == lines(plain[0]) and len(lines(zero[0])) == 2
    assert "view steps" not in zero[0]


def test_view_steps_needs_bake_view(tmp_path):
    base = [MAIN, "--preset", PRESET, "--size", f"{WIDTH}x{HEIGHT}", "--quiet", "--out", str(tmp_path / "x.pfm")]
    for extra in (["--bake", "1.5,2,2", "--view-steps", "2"], ["--bake", "1.5,2,2", "--bake-view", "--view-steps", "9"],
                  ["--bake", "1.5,2,2", "--bake-view", "--view-steps", "-1"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--view-steps" in r.stderr, extra
