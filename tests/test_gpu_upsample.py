"""Rendering below display size on the GPU (ptss_render_features_scaled / ptss_upsample).

Scaled features: byte for byte ptss_render_features of a second context created at f W x f H with the same scene and camera, and
ptss_intersect of that frame's pixel-centre rays; lo 33x17 and 64x64, f = 2, 3, 4; a scene staged in LDS, a mesh image and a
many-sphere image, cfg.everySphereLoop both ways, the default and a moved camera; both feature-kernel instantiations reached; a
two-shard context gets exactly its rows. Upsampling: the device against the host build of csrc/ptupsample.h (ptss_probe_upsample),
array_equal on bytes, floats and weights; frames untouched by both calls; the refusals and the launch counter; ptss_main --upscale;
and the quality figures quoted in DESIGN.md §3.22 (printed; only guided <= replicated is asserted, on cornell and lambert).

Quality, 128x128 -> 256x256, 8 bounces, MSE of the display bytes against 4,096 spp at 256x256, as measured on an MI355X (the table
of DESIGN.md §3.22): (a) replicated 16 spp / (b) guided / (c) guided of the denoised image / (d) 256x256 at 4 spp denoised —
cornell 134.91 / 56.66 / 21.20 / 135.22, lambert 232.99 / 95.55 / 20.69 / 361.31, mixed 264.68 / 114.25 / 45.93 / 493.99."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import ptss
from test_gpu_denoise import MAIN, SCENE_MAKERS, expected_features, moved_camera, mse
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu

FACTORS = (2, 3, 4)
SHAPES = ((33, 17), (64, 64))   # 33x17: ragged workgroups on both axes, all four borders within one workgroup's reach
SCENES = ("mixed", "mesh", "stress")   # staged in LDS; a mesh image; a many-sphere image (chunked unless everySphereLoop)


def same_fields(got, want, what):
    assert got.shape == want.shape, what
    for field in ("normal", "depth", "albedo", "materialIdx"):
        assert got[field].tobytes() == want[field].tobytes(), (what, field, int((got[field] != want[field]).sum()))


# ---- scaled features ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every_sphere_loop", [False, True])
@pytest.mark.parametrize("name", SCENES)
def test_scaled_features_equal_a_larger_context(name, every_sphere_loop):
    scene = ptss.Scene(name)
    scene.desc.defaultColor.x, scene.desc.defaultColor.y, scene.desc.defaultColor.z = 0.25, 0.5, 0.125
    cameras = {"default": ptss.default_camera(), "moved": moved_camera()}
    for w, h in SHAPES:
        lo = ptss.Renderer(scene, w, h, max_iterations=2, every_sphere_loop=every_sphere_loop)
        same_fields(lo.features_scaled(1), lo.features(), (name, w, h, "factor 1"))
        for f in FACTORS:
            hi = ptss.Renderer(scene, w * f, h * f, max_iterations=2, every_sphere_loop=every_sphere_loop)
            for label, cam in cameras.items():
                lo.set_camera(cam)
                hi.set_camera(cam)
                got = lo.features_scaled(f)
                same_fields(got, hi.features(), (name, w, h, f, label, "larger context"))
                _, want = expected_features(lo, scene.desc, cam, w * f, h * f)   # ... and the queries of that frame's pixel-centre rays
                same_fields(got, want, (name, w, h, f, label, "ptss_intersect"))
            hi.close()
        assert len({k for k in lo.launched_kernels() if k[0] == "features"}) == 1   # the instantiation ptss_render_features uses for this image
        lo.close()


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_scaled_features_of_a_two_shard_context(name):
    scene = ptss.Scene(name)
    w, h, band = 40, 36, 8   # 36 rows: bands of 8, 8, 8, 8, 4 — the last band is a partial one
    cam = moved_camera()
    whole = ptss.Renderer(scene, w, h, max_iterations=2)
    whole.set_camera(cam)
    for f in FACTORS:
        full = whole.features_scaled(f).reshape(h * f, w * f)
        seen = []
        for rank in range(2):
            r = ptss.Renderer(scene, w, h, max_iterations=2, tile_rank=rank, tile_world=2, band_rows=band)
            r.set_camera(cam)
            rows = r.rows()
            hi_rows = (rows[:, None] * f + np.arange(f)[None, :]).reshape(-1)   # f hi rows per lo row, in local row order
            seen += hi_rows.tolist()
            same_fields(r.features_scaled(f), full[hi_rows].reshape(-1), (name, f, "shard", rank))
            with pytest.raises(ptss.PtssError, match="shard"):   # a band of rows has no neighbours
                r.upsample(factor=f)
            assert r.upsample_launches() == 0
            r.close()
        assert sorted(seen) == list(range(h * f))
    whole.close()


def test_both_feature_kernels_are_reached():
    """The scaled call alone, on a scene image staged in LDS and on one read in place: it reports the instantiation it launched."""
    reached = set()
    for name in ("mixed", "stress", "in_place_484"):   # the last two are too large for LDS: 1,024 spheres; 484 triangles
        r = ptss.Renderer(SCENE_MAKERS[name](), 33, 17, max_iterations=2)
        assert not r.launched_kernels()
        r.features_scaled(2)
        mine = r.launched_kernels()
        assert len(mine) == 1 and mine <= ptss.feature_kernels(), (name, mine)
        reached |= mine
        r.close()
    assert reached == ptss.feature_kernels(), reached


# ---- device = host ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["frame", "denoised"])
@pytest.mark.parametrize("w,h", [(33, 17), (64, 64), (250, 130)])
def test_device_equals_the_host_build(w, h, source):
    """frame: the frame's pixels after 4 ticks at S = 1; denoised: ptss_denoise output at S = 4."""
    scene = ptss.Scene("mixed")
    S = 1 if source == "frame" else 4
    r = ptss.Renderer(scene, w, h, max_iterations=5, samples_per_pass=S)
    for _ in range(4):
        r.generate_frame()
    shown = r.pixels().copy()
    lo = shown if source == "frame" else r.denoise()
    f_lo = r.features()
    launches = 0
    for f in FACTORS + (1,):
        f_hi = r.features_scaled(f)
        want, want_float = ptss.probe_upsample(lo, f_lo, w, h, f_hi, ptss.default_upsample_params(factor=f))
        got, got_float = r.upsample(lo=None if source == "frame" else lo, factor=f, floats=True)
        launches += 1
        assert np.array_equal(got, want), (w, h, source, f, int((got != want).any(axis=1).sum()))
        assert got_float.tobytes() == want_float.tobytes(), (w, h, source, f, "floats and weights")
        assert np.array_equal(r.upsample(lo=None if source == "frame" else lo, factor=f), want), (w, h, source, f, "without the floats")
        launches += 1
        if f == 1:
            assert np.array_equal(got[:, :3], lo[:, :3]) and (got[:, 3] == 255).all()
    other = ptss.default_upsample_params(factor=2, sigmaNormal=0.5, sigmaDepth=0.25)
    want, want_float = ptss.probe_upsample(lo, f_lo, w, h, r.features_scaled(2), other)
    got, got_float = r.upsample(lo=lo, factor=2, sigma_normal=0.5, sigma_depth=0.25, floats=True)
    assert np.array_equal(got, want) and got_float.tobytes() == want_float.tobytes()
    assert r.upsample_launches() == launches + 1
    assert np.array_equal(r.pixels(), shown)   # the frame's own pixels were not touched
    r.close()


# ---- no trace in frame state --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_frames_are_untouched(S):
    torch = pytest.importorskip("torch")
    scene = ptss.Scene("cornell")
    w, h, bounces = 40, 24, 4
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, samples_per_pass=S)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    assert r.upsample(factor=2).shape == (4 * w * h, 4)   # before the first frame: PTSS_OK
    side = torch.cuda.Stream()
    for tick in range(20):
        r.generate_frame()
        o.generate_frame()
        f = 2 + tick % 3
        r.features_scaled(f)
        r.upsample(factor=f)
        torch.cuda.synchronize()
        r.features_scaled(f, stream=side.cuda_stream)   # and on a second stream
        r.upsample(factor=f, stream=side.cuda_stream)
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, ("twenty frames with scaled features and an upsample after each", S), w, h, S)
    r.close()
    o.close()


# ---- refusals and the counter ---------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter():
    scene = ptss.Scene("cornell")
    w, h = 32, 24
    r = ptss.Renderer(scene, w, h, max_iterations=2)
    r.generate_frame()
    r.features()
    r.features_scaled(2)
    L = ptss.device_lib()
    ctx, lo, fl, fh = r._ctx, r.pixels_devptr(), r.features_devptr(), r.features_scaled_devptr(2)
    out = r._device_buffer("refusal_out", 16 * w * h * 4)
    flt = r._device_buffer("refusal_float", 16 * w * h * 16)
    mask = C.c_ulonglong()
    L.ptss_launched_kernels(ctx, C.byref(mask))
    before, launches = mask.value, r.upsample_launches()
    good = ptss.default_upsample_params()
    off = lambda p, n: C.c_void_p(p.value + n)
    call = lambda c=ctx, a=lo, b=fl, d=fh, p=C.byref(good), o=out, of=flt: L.ptss_upsample(c, a, b, d, p, o, of, None)
    bad = [dict(c=None), dict(a=None), dict(b=None), dict(d=None), dict(p=None), dict(o=None), dict(a=off(lo, 2)), dict(o=off(out, 1)),
           dict(b=off(fl, 4)), dict(d=off(fh, 8)), dict(of=off(flt, 4)), dict(o=lo)]
    for factor in (0, -1, 5):
        bad.append(dict(p=C.byref(ptss.default_upsample_params(factor=factor))))
    for name in ("sigmaNormal", "sigmaDepth"):
        for v in (0.0, -1.0, float("inf"), float("nan")):
            bad.append(dict(p=C.byref(ptss.default_upsample_params(**{name: v}))))
    wrong = ptss.default_upsample_params()
    wrong.structSize -= 4
    bad.append(dict(p=C.byref(wrong)))
    for kw in bad:
        assert call(**kw) == -1, kw
    for args in ((None, 2, fh), (ctx, 2, None), (ctx, 0, fh), (ctx, 5, fh), (ctx, 2, off(fh, 4))):
        assert L.ptss_render_features_scaled(args[0], args[1], args[2], None) == -1, args
    for factor in (0, 5, 1 << 20):   # the binding refuses the factor before it sizes a buffer from it
        with pytest.raises(ValueError, match="factor"):
            r.features_scaled(factor)
        with pytest.raises(ValueError, match="factor"):
            r.upsample(factor=factor)
    L.ptss_launched_kernels(ctx, C.byref(mask))
    assert mask.value == before and r.upsample_launches() == launches
    for k in range(3):   # one per accepted call, with and without the floats; ptss_launched_kernels stays as it is
        assert call(of=None if k == 1 else flt) == 0
        assert r.upsample_launches() == launches + k + 1
    r.synchronize()
    L.ptss_launched_kernels(ctx, C.byref(mask))
    assert mask.value == before
    r.close()


# ---- the host mirror ----------------------------------------------------------------------------------------------------------
def read_tga(path, w, h):
    with open(path, "rb") as f:
        data = f.read()
    assert len(data) == 18 + 3 * w * h and data[12] | data[13] << 8 == w and data[14] | data[15] << 8 == h
    return np.frombuffer(data[18:], dtype=np.uint8).reshape(-1, 3)[:, ::-1]


def test_main_upscale_writes_the_python_composition(tmp_path):
    w, h = 96, 64
    base = [MAIN, "--preset", "cornell", "--size", f"{w}x{h}", "--ticks", "4", "--bounces", "5", "--quiet"]
    plain, up, both = str(tmp_path / "plain.tga"), str(tmp_path / "up.tga"), str(tmp_path / "both.tga")
    for args in (base + ["--out", plain], base + ["--out", up, "--upscale", "2"], base + ["--out", both, "--denoise", "--upscale", "2"]):
        p = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
    assert subprocess.run(base + ["--out", plain, "--upscale", "5"], capture_output=True).returncode == 2
    assert not os.path.exists(str(tmp_path / "plain_upscaled.tga"))
    with open(plain, "rb") as f, open(up, "rb") as g:
        assert f.read() == g.read()   # the normal file is the run's without the flag
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, w, h, max_iterations=5)
    for _ in range(4):
        r.generate_frame()
    want = r.upsample(factor=2)
    want_denoised = r.upsample(lo=r.denoise(), factor=2)
    r.close()
    assert np.array_equal(read_tga(str(tmp_path / "up_upscaled.tga"), 2 * w, 2 * h), want[:, :3])
    assert np.array_equal(read_tga(str(tmp_path / "both_upscaled.tga"), 2 * w, 2 * h), want_denoised[:, :3])
    assert not np.array_equal(want, want_denoised)


def test_main_upscale_combines_with_temporal(tmp_path):
    """--temporal --upscale 2: the filtered history --out receives, upsampled with the features of the final pose."""
    w, h, ticks, keys = 96, 64, 4, "df"
    out = str(tmp_path / "temporal.tga")
    p = subprocess.run([MAIN, "--preset", "cornell", "--size", f"{w}x{h}", "--ticks", str(ticks), "--bounces", "5", "--quiet", "--keys", keys,
                        "--out", out, "--temporal", "--upscale", "2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    # the loop of INTEGRATION.md through the binding (tests/test_gpu_reproject.py test_main_temporal), then the upsample
    r = ptss.Renderer(ptss.Scene("cornell"), w, h, max_iterations=5)
    cam = ptss.default_camera()

    def step():
        r.set_camera(cam)
        for _ in range(ticks):
            r.generate_frame()
        return r.features()

    f = step()
    hist = r.reproject()
    for k in keys:
        prev = (type(cam).from_buffer_copy(cam), f, hist)
        ptss.move_camera(cam, k)
        f = step()
        hist = r.reproject(prev_camera=prev[0], prev_features=prev[1], prev_history=prev[2])
    shown = r.denoise_history()
    want = r.upsample(lo=shown, factor=2)
    r.close()
    assert np.array_equal(read_tga(out, w, h), shown[:, :3])
    assert np.array_equal(read_tga(str(tmp_path / "temporal_upscaled.tga"), 2 * w, 2 * h), want[:, :3])


# ---- quality ------------------------------------------------------------------------------------------------------------------
def quality(name):
    """(a) nearest-neighbour replication of the 16-spp 128x128 image, (b) its guided upsample, (c) the guided upsample of its
    ptss_denoise output, (d) the 256x256 context at 4 spp (the same ray budget) denoised: MSE against 4,096 spp at 256x256."""
    w = h = 128
    scene = ptss.Scene(name)
    big = ptss.Renderer(scene, 2 * w, 2 * h, max_iterations=8)
    for _ in range(4):
        big.generate_frame()
    same_budget = big.denoise()
    for _ in range(4096 - 4):
        big.generate_frame()
    truth = big.pixels().copy()
    big.close()
    r = ptss.Renderer(scene, w, h, max_iterations=8)
    for _ in range(16):
        r.generate_frame()
    lo = r.pixels().copy()
    replicated = np.repeat(np.repeat(lo.reshape(h, w, 4), 2, axis=0), 2, axis=1).reshape(-1, 4)   # numpy: owes nothing to the code under test
    guided = r.upsample(factor=2)
    guided_denoised = r.upsample(lo=r.denoise(), factor=2)
    r.close()
    a, b, c, d = (mse(x, truth) for x in (replicated, guided, guided_denoised, same_budget))
    print(f"upsample quality {name}: MSE (a) replicated 16 spp {a:.2f}, (b) guided {b:.2f}, (c) guided of denoised {c:.2f}, "
          f"(d) 256x256 at 4 spp denoised {d:.2f}; b/a {b / a:.3f}, c/d {c / d:.3f}")
    return a, b, c, d


@pytest.mark.parametrize("name", ["cornell", "lambert"])
def test_guided_does_not_lose_to_replication(name):
    a, b, _, _ = quality(name)
    assert b <= a


def test_mixed_figures_are_recorded_not_asserted():
    """mixed has a mirror and a glass sphere: first-hit features do not describe what is seen in them."""
    a, b, c, d = quality("mixed")
    assert min(a, b, c, d) >= 0
