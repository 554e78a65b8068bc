"""The strip words of bounce 0 (csrc/ptstrip.h) on the host build of that very header (ptss_probe_strip_masks, libptss_host.so): a
clear bit claims that the reference's test rejects that primitive for EVERY eye ray of the strip, so a wrongly cleared bit is a
wrong image. Checked against the CPU oracle on the frame's own eye rays (ptss_camera_ray), jittered over the whole pixel with the
corners and edges of the jitter range included:

  * every primitive the oracle's closest-hit loop ends on has its bit set in that ray's strip, and — the stronger statement the
    kernel relies on — so has every primitive whose own test accepts the ray at all (limit +inf);
  * on random bounded scenes and cameras, and on the scenes a frustum cull gets wrong (tests/strip_mask_common.py), at widths 33,
    64, 65, 130 and 1920 and among 1 to 3 ranks. Misses allowed: none.
  * The words are not vacuous: on `mixed` at 1920 x 1080 a strip keeps 6.5 of the 38 primitives on average (lambert: 6.3).
  * Outside the proven domain every word is all ones, and the stand-alone build of the probe runs clean under
    -fsanitize=address,undefined.
CPU only."""
import os
import subprocess

import numpy as np
import pytest

import ptss
import refprobe
from refprobe import scene_tables
from strip_mask_common import adversarial_cases, camera, make_scene, project, quad, strip_rays, tiny_scene
from test_gpu_fuzz_scenes import random_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def bit_counts(masks, lo=0, hi=64):
    return np.array([bin((int(m) >> lo) & ((1 << (hi - lo)) - 1)).count("1") for m in masks])


def check_superset(desc, cam, w, h, band_rows, rank, world, rays, strip):
    """no ray of a strip is accepted by a primitive whose bit the strip's word has clear; returns the words"""
    masks, on, tri_pos = ptss.probe_strip_masks(desc, cam, w, h, band_rows, rank, world)
    assert on
    if len(rays) == 0:   # a rank without rows
        return masks
    assert strip.max() < len(masks)
    words = masks[strip]
    probes = refprobe.Probes("oracle")
    probes.use_scene(desc)
    tables = scene_tables(desc)
    n = len(rays)

    def kept(bit, where):   # bit: per ray or one number; where: the rays that were accepted
        if not where.any():
            return
        clear = where & (((words >> np.broadcast_to(np.asarray(bit, dtype=np.uint64), (n,))) & np.uint64(1)) == 0)
        if clear.any():
            i = int(np.nonzero(clear)[0][0])
            raise AssertionError(("accepted by a culled primitive", int(np.broadcast_to(bit, (n,))[i]), rays[i].tolist(), int(strip[i]), hex(int(words[i])),
                                  int(clear.sum())))

    # the closest hit of the oracle's intersectScene
    kind, prim, _ = probes.closest_hit(rays)
    pos = tri_pos[np.clip(prim, 0, max(len(tri_pos) - 1, 0))] if len(tri_pos) else np.zeros(n, np.int32)
    kept(np.where(kind == 1, prim, 32 + pos).clip(0, 63), kind != 0)
    # every primitive's own test, limit +inf
    for k, sp in enumerate(tables["spheres"]):
        hit, _ = probes.sphere(np.broadcast_to(np.array([*sp["position"], sp["radius"]], np.float32), (n, 4)), rays)
        kept(k, hit)
    for k, t in enumerate(tables["triangles"]):
        t18 = np.concatenate([t["vertex0"], t["vertex1"], t["vertex2"], t["normal0"], t["normal1"], t["normal2"]]).astype(np.float32)
        hit, _ = probes.triangle(np.broadcast_to(t18, (n, 18)), rays)
        kept(32 + int(tri_pos[k]), hit)
    probes.close()
    return masks


# ---- random bounded scenes and cameras ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_and_cameras(seed):
    scene, rng = random_scene(4000 + seed, ns=int(np.random.default_rng(seed).integers(1, 33)), nt=int(np.random.default_rng(seed + 9).integers(2, 33)))
    w, h = [(130, 9), (65, 20), (256, 64), (33, 17), (64, 12), (200, 31)][seed]
    world = 1 + seed % 3
    cam = camera(rng.uniform(-1, 1, 3), keys="".join(rng.choice(list("wasdqezxcvfghty"), size=4)), fov=float(rng.uniform(0.5, 2.2)),
                 z_near=float(rng.choice([-0.1, 0.37, -2.0])))
    total = 0
    for rank in range(world):
        rays, strip = strip_rays(cam, w, h, 8, rank, world, rng, lanes_per_strip=None if w * h < 3000 else 24)
        masks = check_superset(scene.desc, cam, w, h, 8, rank, world, rays, strip)
        total += len(rays)
    assert total > 1000


# ---- the scenes a cull gets wrong ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,world", [(33, 17, 1), (64, 9, 2), (65, 9, 3), (130, 9, 1), (256, 64, 2)])
def test_adversarial_scenes(w, h, world):
    rng = np.random.default_rng(w * 1000 + h)
    for name, scene, cam in adversarial_cases(w, h):
        tables = scene_tables(scene.desc)
        dense = []
        if name == "tiny":   # the tiny primitives are hit only by rays aimed at them: dense jitter grids around where they project
            dense = [project((w, h), c) for c in tables["spheres"]["position"][:9]] + [project((w, h), v) for v in tables["triangles"]["vertex0"][:4]]
        hits = 0
        for rank in range(world):
            rays, strip = strip_rays(cam, w, h, 8, rank, world, rng, lanes_per_strip=None if w * h < 3000 else 12, random_jitters=2, dense=dense)
            check_superset(scene.desc, cam, w, h, 8, rank, world, rays, strip)
            hits += len(rays)
        assert hits > 0, name


def test_tiny_primitives_are_hit_and_kept():
    """the dense grids do reach the radius-1e-3 spheres and the small triangles (the superset check above is not vacuous for them)"""
    w, h = 256, 64
    scene, cam = tiny_scene(w, h), camera()
    tables = scene_tables(scene.desc)
    rng = np.random.default_rng(5)
    dense = [project((w, h), c) for c in tables["spheres"]["position"]] + [project((w, h), v) for v in tables["triangles"]["vertex0"][:4]]
    rays, strip = strip_rays(cam, w, h, 8, 0, 1, rng, strips=[], dense=dense)
    probes = refprobe.Probes("oracle")
    probes.use_scene(scene.desc)
    kind, prim, _ = probes.closest_hit(rays)
    probes.close()
    assert len(set(prim[kind == 1].tolist())) >= 5 and len(set(prim[kind == 2].tolist()) & {0, 1, 2, 3}) >= 3
    check_superset(scene.desc, cam, w, h, 8, 0, 1, rays, strip)


def test_full_hd_strips():
    """1920 x 1080 among one and three ranks: the frame's first and last strips, the strips around a band jump, and random ones"""
    rng = np.random.default_rng(11)
    for name, scene, cam in adversarial_cases(1920, 1080)[:4:3] + [("mixed", ptss.Scene("mixed"), camera(keys="wd"))]:
        for world, rank in ((1, 0), (3, 1)):
            n = 1920 * len(ptss.tile_rows(1080, 8, rank, world)) // 64
            strips = sorted({0, 1, 29, 30, 239, 240, n - 1} | {int(v) for v in rng.integers(0, n, size=24)})
            rays, strip = strip_rays(cam, 1920, 1080, 8, rank, world, rng, strips=strips, lanes_per_strip=4, random_jitters=1)
            check_superset(scene.desc, cam, 1920, 1080, 8, rank, world, rays, strip)


# ---- not vacuous; off outside the domain -----------------------------------------------------------------------------------------
def test_words_are_not_vacuous_on_the_benchmark_scenes():
    for preset, primitives, most in (("mixed", 38, 8.0), ("lambert", 36, 8.0)):
        scene = ptss.Scene(preset)
        masks, on, _ = ptss.probe_strip_masks(scene, ptss.default_camera(), 1920, 1080)
        assert on and len(masks) == 1920 * 1080 // 64
        total = scene.desc.numSpheres + scene.desc.numTriangles
        mean = bit_counts(masks).mean()
        print(f"{preset}: {mean:.2f} of {total} bits set per strip (spheres {bit_counts(masks, 0, 32).mean():.2f}, triangles {bit_counts(masks, 32, 64).mean():.2f})")
        assert total == primitives and mean < most   # measured: mixed 6.48 of 38, lambert 6.31 of 36
        assert bit_counts(masks).min() >= 1


def test_narrow_frames_and_the_planes_padding_keep_everything():
    scene = ptss.Scene("mixed")
    masks, on, _ = ptss.probe_strip_masks(scene, ptss.default_camera(), 20, 40)   # every strip covers more than two rows
    # 800 pixels: twelve strips of 3.2 rows, half a strip over the last two rows (a rectangle pair like any other), then the plane's padding
    assert on and len(masks) == 16 and (masks[:12] == ALL).all() and masks[12] != ALL and (masks[13:] == ALL).all()
    masks, on, _ = ptss.probe_strip_masks(scene, ptss.default_camera(), 33, 17)   # a strip covers two rows at most once it starts at a row's start
    assert on and (masks != ALL).any()


@pytest.mark.parametrize("what", ["camera far away", "quaternion not unit", "zNear zero", "fov too wide", "camera out of range", "many spheres",
                                  "coordinate beyond 2^20"])
def test_outside_the_domain_nothing_is_culled(what):
    scene, cam, w, h = ptss.Scene("mixed"), ptss.default_camera(), 256, 64
    expect_on = True
    if what == "camera far away":
        cam.position.x = 3e6
    elif what == "quaternion not unit":
        cam.rotation.w = 1.1
    elif what == "zNear zero":
        cam.zNear = 0.0
    elif what == "fov too wide":
        cam.fieldOfView = 3.1
    elif what == "camera out of range":
        cam.position.y, expect_on = 1e16, False
    elif what == "many spheres":
        scene, expect_on = make_scene([((0.1 * k, 0.0, -5.0), 0.04) for k in range(40)], quad((-3, -3, -9), (6, 0, 0), (0, 6, 0))), False
    else:
        scene = make_scene([((0.0, 0.0, -5.0), 1.0), ((2e6, 0.0, -5.0), 1.0)], quad((-3, -3, -9), (6, 0, 0), (0, 6, 4e6)))
    masks, on, _ = ptss.probe_strip_masks(scene, cam, w, h)
    assert on == expect_on
    if what == "coordinate beyond 2^20":   # the two primitives with such a coordinate keep their bits everywhere; the others are still culled
        words = np.array([int(m) for m in masks[: w * h // 64]], dtype=object)
        assert all((m >> 1) & 1 and (m >> 32) & 1 and (m >> 33) & 1 for m in words) and any(not (m & 1) for m in words)
    else:
        assert (masks == ALL).all()


# ---- the probe as a stand-alone program under the sanitizers --------------------------------------------------------------------------
def test_standalone_probe_under_asan_and_ubsan(tmp_path):
    src = os.path.join(ROOT, "cuda-path-tracer-ss_amd")
    exe = str(tmp_path / "strip_masks_main")
    # only host_capi.cpp (which includes the header) is instrumented; Scene.cpp and HostOps.cpp come from the shared library
    cmd = ["g++", "-O1", "-std=c++17", "-mfma", "-mavx2", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(src, "csrc"), "-I", os.path.join(src, "host"),
           os.path.join(ROOT, "tests", "csrc", "strip_masks_main.cpp"), os.path.join(src, "host", "host_capi.cpp"), ptss.HOST_LIB,
           "-Wl,-rpath," + os.path.dirname(ptss.HOST_LIB)]
    subprocess.run(cmd + ["-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    # the same words as the shared library gives
    got = {line.split()[0]: line.split()[1:] for line in run.stdout.splitlines()}
    masks, on, _ = ptss.probe_strip_masks(ptss.Scene("mixed"), ptss.default_camera(), 130, 9)
    assert got["mixed-130x9"] == [str(int(on)), str(len(masks)), "%016x" % (int(np.bitwise_xor.reduce(masks)))]
