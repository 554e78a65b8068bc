"""First-hit features and the denoiser on the GPU (ptss_render_features / ptss_denoise).

Features: Renderer.features() against Renderer.intersect(camera_rays(...)) joined with the scene's materials, field for field and
bit for bit, and three pixels per case against the oracle's own loop over oracle_probe_sphere / oracle_probe_triangle.
Denoiser: the device against the host build of csrc/ptdenoise.h (ptss_probe_denoise) on the read-back accumulator and features,
array_equal on the bytes of a k-level run and on the floats of level k (the colour plane a run with k + 1 levels leaves behind,
ptss_read_denoise_plane), k = 1..5; levels = 0 against the frame's display pixels, frames untouched by denoising, and the quality condition: on cornell
and lambert the denoised 4-spp image is strictly closer (mean squared error of the display bytes) to a 4,096-spp render than the
raw 4-spp image. The ratios this file prints are the ones quoted in DESIGN.md §3.17."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import ptss
from test_gpu_kernel_coverage import SCENES as COVERAGE_SCENES, compare
from test_gpu_ray_query import oracle_closest, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_main")
_REACHED = set()   # feature-kernel instantiations launched across the module (test_both_feature_kernels_are_reached)

SCENE_MAKERS = {
    "default": lambda: ptss.Scene("default"),
    "cornell": lambda: ptss.Scene("cornell"),
    "mixed": lambda: ptss.Scene("mixed"),
    "stress": lambda: ptss.Scene("stress"),
    "mesh": lambda: ptss.Scene("mesh"),
    "in_place_484": lambda: COVERAGE_SCENES["plain_padded"](),
}


def moved_camera():
    cam = ptss.default_camera()
    for k in "wdfth":
        ptss.move_camera(cam, k)
    return cam


def far_camera():
    cam = ptss.default_camera()
    cam.position.z = 4e15   # beyond the 1e15 range of the bounded tests: the literal paths
    return cam


def expected_features(r, desc, cam, w, h, rows=None):
    """ptss_intersect of every pixel-centre ray, joined with the materials' diffuse colours."""
    rays = ptss.camera_rays(cam, w, h)
    if rows is not None:
        rays = rays.reshape(h, w, 8)[rows].reshape(-1, 8)
    hits = r.intersect(rays)
    f = np.zeros(len(rays), dtype=ptss.FEATURE_DTYPE)
    f["normal"], f["depth"], f["materialIdx"] = hits["normal"], hits["distance"], hits["materialIdx"]
    colours = np.array([[m.diffuseColor.x, m.diffuseColor.y, m.diffuseColor.z] for m in (desc.materials[k] for k in range(desc.numMaterials))],
                       dtype=np.float32)
    default = np.array([desc.defaultColor.x, desc.defaultColor.y, desc.defaultColor.z], dtype=np.float32)
    hit = hits["kind"] != 0
    f["albedo"] = default
    f["albedo"][hit] = colours[hits["materialIdx"][hit]]
    return rays, f


def check_features(r, desc, cam, w, h, what, rows=None):
    got = r.features()
    rays, want = expected_features(r, desc, cam, w, h, rows)
    assert got.shape == want.shape
    for field in ("normal", "depth", "albedo", "materialIdx"):
        assert got[field].tobytes() == want[field].tobytes(), (what, field)
    miss = got["materialIdx"] < 0
    assert np.isposinf(got["depth"][miss]).all() and not got["normal"][miss].any()
    # three pixels against the oracle's own sphere / triangle tests: the check does not rest on the query path alone
    for p in (0, len(rays) // 2 + w // 3, len(rays) - 1):
        kind, _, mat, dist, _, normal = oracle_closest(desc, rays[p])
        assert int(got["materialIdx"][p]) == mat, (what, p)
        assert same_bits(got["depth"][p], dist) and same_bits(got["normal"][p], normal), (what, p)
    _REACHED.update(k for k in r.launched_kernels() if k[0] == "features")


@pytest.mark.parametrize("every_sphere_loop", [False, True])
@pytest.mark.parametrize("name", list(SCENE_MAKERS))
def test_features_equal_the_queries(name, every_sphere_loop):
    scene = SCENE_MAKERS[name]()
    scene.desc.defaultColor.x, scene.desc.defaultColor.y, scene.desc.defaultColor.z = 0.25, 0.5, 0.125
    w, h = 37, 23   # W != H, neither a multiple of anything
    r = ptss.Renderer(scene, w, h, max_iterations=2, every_sphere_loop=every_sphere_loop)
    check_features(r, scene.desc, ptss.default_camera(), w, h, (name, "default camera"))   # before any frame
    r.generate_frame()
    frame_lds = {k[3] for k in r.launched_kernels() if k[0] == "bounce"}   # how this context's frames read the same scene image
    cam = moved_camera()
    r.set_camera(cam)
    check_features(r, scene.desc, cam, w, h, (name, "after ptss_set_camera"))
    cam = far_camera()
    r.set_camera(cam)
    check_features(r, scene.desc, cam, w, h, (name, "camera beyond 1e15"))
    # which instantiation: the one that reads the scene image the way the frames do — in place for the 484-triangle image,
    # staged in LDS for the small presets
    assert len(frame_lds) == 1
    lds = frame_lds.pop()
    if name == "in_place_484":
        assert not lds
    if name in ("default", "cornell", "mixed"):
        assert lds
    assert r.launched_kernels() & ptss.feature_kernels() == {("features", lds)}, name
    r.close()


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_features_of_a_two_shard_context(name):
    scene = SCENE_MAKERS[name]()
    w, h = 40, 36
    cam = moved_camera()
    seen = []
    for rank in range(2):
        r = ptss.Renderer(scene, w, h, max_iterations=2, tile_rank=rank, tile_world=2, band_rows=8)
        r.set_camera(cam)
        rows = r.rows()
        seen += rows.tolist()
        check_features(r, scene.desc, cam, w, h, (name, "shard", rank), rows=rows)
        with pytest.raises(ptss.PtssError, match="shard"):   # a band of rows has no neighbours to filter with
            r.denoise(levels=1)
        r.close()
    assert sorted(seen) == list(range(h))


# ---- device = host --------------------------------------------------------------------------------------------------------------
def inverse_ticks(S, frames):
    return np.float32(1.0) / np.float32(S * frames)


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("w,h", [(64, 64), (250, 130), (1280, 720)])
def test_device_equals_the_host_build(w, h, S):
    scene = ptss.Scene("mixed")
    r = ptss.Renderer(scene, w, h, max_iterations=5, samples_per_pass=S)
    frames = 3
    for _ in range(frames):
        r.generate_frame()
    shown = r.pixels().copy()
    features = r.features()
    accum = r.accumulator()
    for levels in range(1, 6):
        p = ptss.default_denoise_params(levels=levels)
        want, want_float = ptss.probe_denoise(accum, inverse_ticks(S, frames), features, w, h, p)
        separate = r.denoise(levels=levels)
        assert np.array_equal(separate, want), (w, h, S, levels, "separate buffer")
        # the floats behind those bytes: one more level leaves the result of pass `levels` in a colour plane (levels + 1 <= 6)
        r.denoise(levels=levels + 1)
        got_float, level = r.denoise_plane()
        assert level == levels - 1
        assert got_float.tobytes() == want_float.tobytes(), (w, h, S, levels, "floats", float(np.abs(got_float - want_float).max()))
        assert np.array_equal(r.pixels(), shown)   # the frame's own pixels were not touched
        aliased = r.denoise(levels=levels, dev_out=r.pixels_devptr())
        assert np.array_equal(aliased, want), (w, h, S, levels, "dev_out = dev_pixels")
        r.denoise(levels=0, dev_out=r.pixels_devptr())   # levels = 0 puts the display pixels back
        assert np.array_equal(r.pixels(), shown)
    assert np.array_equal(r.accumulator(), accum)
    assert ("denoise",) in r.launched_kernels()
    r.close()


@pytest.mark.parametrize("S", [1, 4])
def test_levels_zero_is_the_frames_display(S):
    """S = 1: the pixels finishPath wrote; S = 4: displayKernel's."""
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, 61, 47, max_iterations=4, samples_per_pass=S)
    for frames in (1, 2, 7):
        while r.ticks <= frames:
            r.generate_frame()
        assert np.array_equal(r.denoise(levels=0), r.pixels()), (S, frames)
    r.close()


# ---- no trace in frame state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_frames_are_untouched_by_denoising(S):
    torch = pytest.importorskip("torch")
    scene = ptss.Scene("cornell")
    w, h, bounces = 40, 24, 4
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, samples_per_pass=S)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    assert r.denoise(levels=3).shape == (w * h, 4)   # before the first frame: PTSS_OK
    side = torch.cuda.Stream()
    for tick in range(20):
        r.generate_frame()
        o.generate_frame()
        r.features()
        r.denoise(levels=1 + tick % 5)
        torch.cuda.synchronize()
        r.denoise(levels=5, stream=side.cuda_stream)   # and on a second stream
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, ("twenty frames with a denoise after each", S), w, h, S)
    r.request_reset()
    r.denoise(levels=2)   # after a reset request
    r.set_mode(False)
    o.set_mode(False)
    r.denoise(levels=2)   # in ray-tracing mode, before and after its first frame
    r.generate_frame()
    o.generate_frame()
    r.denoise(levels=2)
    compare(r, o, ("ray-tracing mode", S), w, h, S)
    r.close()
    o.close()


# ---- quality ------------------------------------------------------------------------------------------------------------------
def mse(a, b):
    return float(((a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)) ** 2).mean())


def quality(name):
    scene = ptss.Scene(name)
    r = ptss.Renderer(scene, 256, 256, max_iterations=8)
    for _ in range(4):
        r.generate_frame()
    raw = r.pixels().copy()
    denoised = r.denoise()   # default parameters
    for _ in range(4096 - 4):
        r.generate_frame()
    truth = r.pixels().copy()
    r.close()
    a, b = mse(raw, truth), mse(denoised, truth)
    print(f"quality {name}: MSE raw 4 spp {a:.2f}, denoised {b:.2f}, ratio {b / a:.3f} (256x256, 8 bounces, truth 4,096 spp)")
    return a, b


@pytest.mark.parametrize("name", ["cornell", "lambert"])
def test_denoised_is_closer_to_the_converged_image(name):
    a, b = quality(name)
    assert b < a


def test_mixed_ratio_is_recorded_not_asserted():
    """mixed has a mirror and a glass sphere: first-hit features do not describe what is seen in them, so reflections are blurred
    within the material. The ratio is printed for the record."""
    a, b = quality("mixed")
    assert a > 0 and b >= 0


# ---- the host mirror ----------------------------------------------------------------------------------------------------------
def test_main_denoise_writes_both_files(tmp_path):
    w, h = 96, 64
    base = [MAIN, "--preset", "cornell", "--size", f"{w}x{h}", "--ticks", "4", "--bounces", "5", "--quiet"]
    plain, both = str(tmp_path / "plain.tga"), str(tmp_path / "both.tga")
    for args in (base + ["--out", plain], base + ["--out", both, "--denoise"], base + ["--out", str(tmp_path / "two.tga"), "--denoise", "2"]):
        p = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
    assert not os.path.exists(str(tmp_path / "plain_denoised.tga"))
    with open(plain, "rb") as f, open(both, "rb") as g:
        shown = f.read()
        assert shown == g.read()   # without the flag: byte-identical
    for name in ("both_denoised.tga", "two_denoised.tga"):
        with open(str(tmp_path / name), "rb") as f:
            data = f.read()
        assert len(data) == len(shown) == 18 + 3 * w * h and data[:18] == shown[:18]
        assert data != shown
    # the same image through the Python binding
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, w, h, max_iterations=5)
    for _ in range(4):
        r.generate_frame()
    want = r.denoise()
    r.close()
    with open(str(tmp_path / "both_denoised.tga"), "rb") as f:
        bgr = np.frombuffer(f.read()[18:], dtype=np.uint8).reshape(-1, 3)
    assert np.array_equal(bgr[:, ::-1], want[:, :3])


def test_denoise_plane_needs_two_levels():
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, 32, 24, max_iterations=2)
    r.generate_frame()
    for levels in (0, 1):
        r.denoise(levels=levels)
        with pytest.raises(ptss.PtssError, match="fewer than two levels"):
            r.denoise_plane()
    r.denoise(levels=4)
    flt, level = r.denoise_plane()
    assert level == 2 and flt.shape == (32 * 24, 3) and np.isfinite(flt).all()
    r.close()


def test_set_camera_invalidates_the_kept_features():
    """Renderer.denoise(features=None) filters with the features of the CURRENT camera."""
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, 48, 32, max_iterations=3)
    cam = moved_camera()
    for _ in range(3):
        ptss.move_camera(cam, "d")
    r.features()   # of the default camera
    r.set_camera(cam)
    for _ in range(2):
        r.generate_frame()
    got = r.denoise(levels=3)
    want, _ = ptss.probe_denoise(r.accumulator(), inverse_ticks(1, 2), r.features(), 48, 32, ptss.default_denoise_params(levels=3))
    assert np.array_equal(got, want)
    r.close()


def test_both_feature_kernels_are_reached():
    """(Across the module, like tests/test_gpu_kernel_coverage.py's test_every_instantiation_is_reached: run the file as a whole.)"""
    assert _REACHED == ptss.feature_kernels(), _REACHED
