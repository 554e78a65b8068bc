"""ptss_main --bake ... --bake-view [nearest|bilinear]: the bake goes through ptss_surface_atlas_blocks (spheres get
texels), then the camera's centre rays -> ptss_intersect -> ptss_lookup_lightmap with both flags -> ptss_resolve_linear. Both files are
the ones the shadow loop of the probes computes; only the trace and the intersection stay on the device."""
import os
import subprocess

import numpy as np
import pytest

import ptss
from lightmap_common import read_pfm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
PRESET, WIDTH, HEIGHT, BOUNCES, SEED = "mixed", 64, 48, 3, 0xBA4E


@pytest.mark.parametrize("option, filter", [(["bilinear"], "bilinear"), (["nearest"], "nearest"), ([], "bilinear")])
def test_bake_view_writes_the_shadow_loops_files(tmp_path, option, filter):
    out = tmp_path / "lightmap.pfm"
    args = ["--preset", PRESET, "--size", f"{WIDTH}x{HEIGHT}", "--bounces", str(BOUNCES), "--seed", str(SEED), "--quiet", "--bake", "1.5,2,2", "--bake-view"]
    run = subprocess.run([MAIN] + args + option + ["--out", str(out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr + run.stdout
    scene = ptss.Scene(PRESET)
    tri, sph = ptss.scene_records(scene)
    assert len(sph) == 22
    bt, bs, points, texels, height = ptss.surface_atlas_blocks(tri, sph, 1.5, WIDTH, 1, WIDTH // 2)
    assert f"bake: atlas {WIDTH} x {height}, {len(points)} texels of {len(tri)} triangles, 2 samples, 2 passes, rejected 0" in run.stdout
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
        hits = r.intersect(ptss.probe_film_rays(centre, np.zeros((WIDTH * HEIGHT, 6), np.uint32))[0])
    finally:
        r.close()
    params = ptss.lightmap_params(WIDTH, height, filter, modulate=True, emission=True)
    view, info = ptss.probe_lookup_lightmap(scene, hits, baked, params, bt, bs, film=film)
    assert (f"bake view: {WIDTH} x {HEIGHT}, {filter}, 22 sphere blocks, filtered {info[0]}, empty {info[1]}, no block {info[2]}, rejected {info[3]}"
            in run.stdout), run.stdout
    for path, entries, rows in ((out, baked, height), (tmp_path / "lightmap_view.pfm", view, HEIGHT)):
        linear = ptss.probe_resolve_linear(entries, params=film, pixels=None, history=None)[0]
        means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
        got, got_rows = read_pfm(path, WIDTH)
        assert got_rows == rows and got.tobytes() == means.tobytes(), path
    lit = view["samples"] == 1
    assert info[3] == 0 and view["r"][lit & (hits["kind"] == 1)].any() and view["r"][lit & (hits["kind"] == 2)].any()   # triangles and spheres carry light


def test_bake_view_needs_bake(tmp_path):
    r = subprocess.run([MAIN, "--preset", PRESET, "--size", f"{WIDTH}x{HEIGHT}", "--quiet", "--bake-view", "--out", str(tmp_path / "x.pfm")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--bake-view" in r.stderr
