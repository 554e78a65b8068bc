"""Features behind mirrors and glass on the GPU (ptss_render_features_specular).

The kernel's rows and step counts against a Python loop of Renderer.intersect and ptss_probe_specular_step (the host build of
csrc/ptspecular.h), byte for byte, for maxSteps 0, 1, 2 and 8, three cameras and six scenes, with and without cfg.everySphereLoop;
maxSteps = 0 and a Lambert-only scene against ptss_render_features; a two-shard context; frames untouched by the call, which also
leaves ptss_launched_kernels as it is and counts in ptss_specular_feature_launches instead; the refusals; ptss_main
--specular-features; and the question the feature exists for, printed for DESIGN.md §3.21: is a 4-spp image filtered with these
features closer to the converged image than one filtered with first-hit features?"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import oracle
import ptss
from test_gpu_denoise import MAIN, SCENE_MAKERS, far_camera, moved_camera, mse
from test_gpu_edge_scenes import CREAM, EMIT, GLASS, GREEN, MIRROR, RED, build, quad
from test_gpu_kernel_coverage import compare

pytestmark = pytest.mark.gpu

W, H = 37, 23   # W != H, neither a multiple of anything; 851 pixels = 14 waves, the last one partly filled
STEPS = (0, 1, 2, 8)
_LAUNCHES = [0, 0]   # ptss_specular_feature_launches added up over the module: [in place, in LDS]


def same_bits(a, b):
    return a.tobytes() == b.tobytes()


def tir_scene():
    """The camera (at the origin) inside two overlapping glass spheres. The one centred at +x, whose surface is the nearer one for
    rays towards -x, has lost its specular lobe: total internal reflection ends the chain there. The one centred at -x keeps it and
    reflects. Ahead a mirror triangle pair, around them diffuse walls on which the chains end."""
    s = build(spheres=[((0.7, 0.0, 0.0), 1.0, GLASS), ((-0.7, 0.0, 0.0), 1.0, GLASS + 1), ((0.0, -0.4, -3.0), 0.5, RED)],
              triangles=quad((-4, -1.5, 1), (4, -1.5, 1), (4, -1.5, -9), (-4, -1.5, -9), CREAM) +
              quad((-2.5, -1.5, -6), (2.5, -1.5, -6), (2.5, 2.5, -6.5), (-2.5, 2.5, -6.5), MIRROR) +
              quad((-4, -1.5, 2), (4, -1.5, 2), (4, 4, 2), (-4, 4, 2), GREEN) + quad((-1, 3, -3), (1, 3, -3), (1, 3, -5), (-1, 3, -5), EMIT),
              area=[((50, 50, 50), 6)])
    s.desc.materials[GLASS].specAvg = 0.0   # spec-less glass
    return s


def mirror_mesh():
    """The mesh preset with the icosphere's material turned into a flagged mirror: chains leave a mesh image from its triangles."""
    s = ptss.Scene("mesh")
    m = s.desc.materials[s.desc.numMaterials - 1]
    m.diffAvg, m.specAvg, m.flags = 0.0, 0.9, b"\x01"
    assert ptss.specular_class(s.desc.materials[s.desc.numMaterials - 1]) == "mirror"
    return s


SCENES = {
    "default": SCENE_MAKERS["default"],
    "cornell": SCENE_MAKERS["cornell"],
    "mixed": SCENE_MAKERS["mixed"],
    "tir": tir_scene,
    "mirror_mesh": mirror_mesh,
    "in_place_484": SCENE_MAKERS["in_place_484"],
}


def expected_chain(r, desc, cam, w, h, max_steps, rows=None):
    """The chain as a composition: ptss_intersect of the live rays, ptss_probe_specular_step of their hits, max_steps + 1 times.
    Returns (features, steps, what happened: a dict of counts)."""
    rays = ptss.camera_rays(cam, w, h)
    if rows is not None:
        rays = rays.reshape(h, w, 8)[rows].reshape(-1, 8)
    n = len(rays)
    colours = np.array([[m.diffuseColor.x, m.diffuseColor.y, m.diffuseColor.z] for m in (desc.materials[k] for k in range(desc.numMaterials))],
                       dtype=np.float32)
    classes = np.array([ptss.SPECULAR_CLASSES.index(ptss.specular_class(desc.materials[k])) for k in range(desc.numMaterials)])
    feat = np.zeros(n, dtype=ptss.FEATURE_DTYPE)
    steps = np.zeros(n, dtype=np.uint32)
    depth = np.zeros(n, dtype=np.float32)
    live = np.ones(n, dtype=bool)
    cur = rays.copy()
    iors = np.array([desc.materials[k].indexOfRefraction for k in range(desc.numMaterials)], dtype=np.float64)
    seen = dict(tir_stopped=0, tir_reflected=0, refracted=0, mirrored=0, missed_after_steps=0)
    for k in range(max_steps + 1):
        idx = np.nonzero(live)[0]
        if not len(idx):
            break
        hits = r.intersect(cur[idx])
        hit = hits["kind"] != 0
        miss = idx[~hit]
        feat["normal"][miss], feat["depth"][miss], feat["materialIdx"][miss] = 0, np.inf, -1
        feat["albedo"][miss] = [desc.defaultColor.x, desc.defaultColor.y, desc.defaultColor.z]
        seen["missed_after_steps"] += int((steps[miss] > 0).sum())
        at, hh = idx[hit], hits[hit]
        depth[at] = hh["distance"] if k == 0 else depth[at] + hh["distance"]   # float32, in chain order
        feat["normal"][at], feat["depth"][at], feat["materialIdx"][at] = hh["normal"], depth[at], hh["materialIdx"]
        feat["albedo"][at] = colours[hh["materialIdx"]]
        live[:] = False
        if k < max_steps and len(at):
            nxt, follows = ptss.probe_specular_step(cur[at], hh, desc)
            # what happened, from a float64 look at the hits (counts only: they show that a case reaches its branches)
            cls, ior = classes[hh["materialIdx"]], iors[hh["materialIdx"]]
            cos = -(cur[at, 4:7].astype(np.float64) * hh["normal"]).sum(1)
            eta = np.where(cos > 0, 1.0 / ior, ior)
            tir = (cls == 1) & (eta * eta * (1 - cos * cos) > 1.001)
            seen["tir_stopped"] += int((tir & ~follows).sum())
            seen["tir_reflected"] += int((tir & follows).sum())
            seen["refracted"] += int(((cls == 1) & ~tir & follows).sum())
            seen["mirrored"] += int(((cls == 2) & follows).sum())
            go = at[follows]
            cur[go] = nxt[follows]
            steps[go] += 1
            live[go] = True
    return feat, steps, seen


def check(r, desc, cam, w, h, max_steps, what, rows=None):
    got, got_steps = r.features_specular(max_steps, steps=True)
    want, want_steps, seen = expected_chain(r, desc, cam, w, h, max_steps, rows)
    assert got.shape == want.shape
    for field in ("normal", "depth", "albedo", "materialIdx"):
        assert same_bits(got[field], want[field]), (what, max_steps, field, int((got[field] != want[field]).sum()))
    assert np.array_equal(got_steps, want_steps), (what, max_steps)
    assert got_steps.max(initial=0) <= max_steps
    assert same_bits(r.features_specular(max_steps), got), (what, "without dev_steps")
    miss = got["materialIdx"] < 0
    assert np.isposinf(got["depth"][miss]).all() and not got["normal"][miss].any()
    return got, got_steps, seen


# ---- the kernel equals the composition --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every_sphere_loop", [False, True])
@pytest.mark.parametrize("name", list(SCENES))
def test_rows_and_steps_equal_the_composition(name, every_sphere_loop):
    scene = SCENES[name]()
    scene.desc.defaultColor.x, scene.desc.defaultColor.y, scene.desc.defaultColor.z = 0.25, 0.5, 0.125
    r = ptss.Renderer(scene, W, H, max_iterations=2, every_sphere_loop=every_sphere_loop)
    total = dict()
    deepest = 0
    for cam_name, cam in (("default", ptss.default_camera()), ("moved", moved_camera()), ("far", far_camera())):
        r.set_camera(cam)
        first_hit = r.features()
        for max_steps in STEPS:
            got, steps, seen = check(r, scene.desc, cam, W, H, max_steps, (name, cam_name))
            if max_steps == 0:   # what ptss_render_features writes, bit for bit
                assert same_bits(got, first_hit) and not steps.any(), (name, cam_name)
            if cam_name != "far":
                for k, v in seen.items():
                    total[k] = total.get(k, 0) + v
                deepest = max(deepest, int(steps.max()))
    print(f"{name}: {total}, deepest chain {deepest}")
    # the cases are there for a reason: each reaches the branches it was chosen for
    if name in ("default", "mixed"):
        assert total["refracted"] > 0 and total["mirrored"] > 0 and deepest >= 3
    if name == "cornell":
        assert total["refracted"] > 0 and total["mirrored"] > 0   # the Phong-glass sphere, the Fresnel-weighted mirror panel
    if name == "tir":
        assert total["tir_stopped"] > 0 and total["tir_reflected"] > 0 and total["refracted"] > 0 and total["mirrored"] > 0
    if name == "mirror_mesh":
        assert total["mirrored"] > 0
    inplace, lds = r.specular_feature_launches()
    assert (inplace == 0) != (lds == 0)
    if name == "in_place_484":
        assert lds == 0
    if name in ("default", "cornell", "mixed", "tir"):
        assert inplace == 0
    _LAUNCHES[0] += inplace
    _LAUNCHES[1] += lds
    r.close()


def test_a_lambert_scene_has_no_chain():
    scene = ptss.Scene("lambert")
    r = ptss.Renderer(scene, W, H, max_iterations=2)
    cam = moved_camera()
    r.set_camera(cam)
    first_hit = r.features()
    for max_steps in (1, 8):
        got, steps = r.features_specular(max_steps, steps=True)
        assert same_bits(got, first_hit) and not steps.any(), max_steps
    r.close()


# ---- sharding -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mirror_mesh"])
def test_a_two_shard_context_gets_its_own_rows(name):
    scene = SCENES[name]()
    w, h = 40, 36
    cam = moved_camera()
    seen_rows = []
    for rank in range(2):
        r = ptss.Renderer(scene, w, h, max_iterations=2, tile_rank=rank, tile_world=2, band_rows=8)
        r.set_camera(cam)
        rows = r.rows()
        seen_rows += rows.tolist()
        _, steps, _ = check(r, scene.desc, cam, w, h, 4, (name, "shard", rank), rows=rows)
        assert steps.any()
        r.close()
    assert sorted(seen_rows) == list(range(h))


# ---- no trace in frame state ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_frames_are_untouched(S):
    torch = pytest.importorskip("torch")
    scene = ptss.Scene("mixed")
    w, h, bounces = 40, 24, 4
    r = ptss.Renderer(scene, w, h, max_iterations=bounces, float_accumulator=True, samples_per_pass=S)
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    r.features_specular(3)   # before the first frame
    side = torch.cuda.Stream()
    for tick in range(12):
        r.generate_frame()
        o.generate_frame()
        before = r.launched_kernels()
        r.features_specular(tick % 9, steps=bool(tick & 1))
        torch.cuda.synchronize()
        r.features_specular(8, steps=True, stream=side.cuda_stream)   # and on a second stream
        assert r.launched_kernels() == before, tick
        assert np.array_equal(r.live_counts(), o.live_counts()), tick
    compare(r, o, ("twelve frames with the specular features after each", S), w, h, S)
    r.request_reset()
    r.features_specular(2)
    r.set_mode(False)
    o.set_mode(False)
    r.generate_frame()
    o.generate_frame()
    r.features_specular(2)
    compare(r, o, ("ray-tracing mode", S), w, h, S)
    inplace, lds = r.specular_feature_launches()
    assert inplace == 0 and lds == 1 + 2 * 12 + 2
    r.close()
    o.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_move_no_counter():
    L = ptss.device_lib()
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, W, H, max_iterations=2)
    r.features_specular(1, steps=True)
    d_feat, d_steps = r.features_specular_devptr(), r._device_buffer("specular_steps", W * H * 4)
    counters, kernels = r.specular_feature_launches(), r.launched_kernels()
    assert counters == (0, 1)
    off = lambda p, k: C.c_void_p(p.value + k)
    assert L.ptss_render_features_specular(None, 1, d_feat, d_steps, None) == -1
    assert L.ptss_render_features_specular(r._ctx, 1, None, d_steps, None) == -1
    for bad in (-1, 9, 2 ** 31 - 1, -2 ** 31):
        assert L.ptss_render_features_specular(r._ctx, bad, d_feat, d_steps, None) == -1, bad
    for k in (4, 8, 12):
        assert L.ptss_render_features_specular(r._ctx, 1, off(d_feat, k), d_steps, None) == -1, k
    for k in (1, 2, 3):
        assert L.ptss_render_features_specular(r._ctx, 1, d_feat, off(d_steps, k), None) == -1, k
    out = (C.c_ulonglong * 2)()
    assert L.ptss_specular_feature_launches(None, out) == -1 and L.ptss_specular_feature_launches(r._ctx, None) == -1
    assert r.specular_feature_launches() == counters and r.launched_kernels() == kernels
    assert L.ptss_render_features_specular(r._ctx, 8, d_feat, None, None) == 0   # dev_steps may be NULL; 8 is allowed
    r.synchronize()
    assert r.specular_feature_launches() == (0, 2) and r.launched_kernels() == kernels
    r.close()


def test_both_instantiations_were_launched():
    """(Across the module, like tests/test_gpu_denoise.py's test_both_feature_kernels_are_reached: run the file as a whole.)"""
    assert _LAUNCHES[0] > 0 and _LAUNCHES[1] > 0, _LAUNCHES


# ---- quality --------------------------------------------------------------------------------------------------------------------
def quality(name, max_steps=4):
    scene = ptss.Scene(name)
    r = ptss.Renderer(scene, 256, 256, max_iterations=8)
    for _ in range(4):
        r.generate_frame()
    raw = r.pixels().copy()
    first_hit = r.denoise()   # default parameters, ptss_render_features
    feats, steps = r.features_specular(max_steps, steps=True)
    specular = r.denoise(features=feats)
    for _ in range(4096 - 4):
        r.generate_frame()
    truth = r.pixels().copy()
    r.close()
    behind = steps > 0
    out = {}
    for where, mask in (("whole image", np.ones(len(steps), dtype=bool)), ("steps > 0", behind)):
        a, b, c = (mse(x[mask], truth[mask]) if mask.any() else float("nan") for x in (raw, first_hit, specular))
        out[where] = (a, b, c)
        print(f"quality {name}, {where} ({int(mask.sum())} px): MSE raw 4 spp {a:.2f}, denoised with first-hit features {b:.2f} "
              f"(ratio {b / a:.3f}), with specular features {c:.2f} (ratio {c / a:.3f}; {c / b:.3f} of first-hit) "
              f"(256x256, 8 bounces, maxSteps {max_steps}, truth 4,096 spp)")
    print(f"quality {name}: mean steps per pixel {steps.mean():.3f}, pixels with steps > 0: {behind.mean():.3f}")
    return out


@pytest.mark.parametrize("name", ["cornell", "mixed", "default"])
def test_quality_is_recorded(name):
    """Asserted: on cornell the image filtered with the specular features beats the raw one over the whole image. Everything else
    is printed for the record of DESIGN.md §3.21, whichever way it falls."""
    out = quality(name)
    raw, _, specular = out["whole image"]
    assert raw > 0 and specular >= 0
    if name == "cornell":
        assert specular < raw


# ---- the host mirror ------------------------------------------------------------------------------------------------------------
def test_main_specular_features(tmp_path):
    w, h = 96, 64
    base = [MAIN, "--preset", "cornell", "--size", f"{w}x{h}", "--ticks", "4", "--bounces", "5", "--quiet"]
    files = {k: str(tmp_path / f"{k}.tga") for k in ("plain", "zero", "four")}
    for args in (base + ["--out", files["plain"], "--denoise"], base + ["--out", files["zero"], "--denoise", "--specular-features", "0"],
                 base + ["--out", files["four"], "--denoise", "--specular-features", "4"]):
        p = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
    data = {}
    for k, path in files.items():
        with open(path, "rb") as f, open(path[:-4] + "_denoised.tga", "rb") as g:
            data[k] = (f.read(), g.read())
    assert data["plain"][0] == data["zero"][0] == data["four"][0]
    assert data["zero"][1] == data["plain"][1]    # maxSteps = 0: the bytes of plain --denoise
    assert data["four"][1] != data["plain"][1] and len(data["four"][1]) == 18 + 3 * w * h
    for bad in (["--specular-features", "4"], ["--denoise", "--specular-features", "9"]):   # without --denoise; out of range
        p = subprocess.run(base + ["--out", str(tmp_path / "bad.tga")] + bad, capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "--specular-features" in p.stderr
    # the same image through the Python binding
    scene = ptss.Scene("cornell")
    r = ptss.Renderer(scene, w, h, max_iterations=5)
    for _ in range(4):
        r.generate_frame()
    want = r.denoise(features=r.features_specular(4))
    r.close()
    bgr = np.frombuffer(data["four"][1][18:], dtype=np.uint8).reshape(-1, 3)
    assert np.array_equal(bgr[:, ::-1], want[:, :3])
