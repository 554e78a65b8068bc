"""ptss_main --film KIND --linear [exposure] --tone clamp|reinhard[,white]|filmic [--srgb] [--tone-luminance]: after the
last round the table is built and the toned resolve makes the screenshot and the PFM, at the meter's exposure and with the glare pyramid
where --auto-exposure and --glare keep them. The files are the ones the Python face computes from the same calls; --tone clamp writes the
bytes of the run without the flag."""
import subprocess

import numpy as np
import pytest

import ptss
from path_query_common import H, W
from test_gpu_glare_main import python_face, run_main
from test_gpu_linear_main import ARGS, MAIN, read_pfm, read_tga

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("extra, compensation, key_rate, glare_arg, glare_kw, tone_args, tone_kw", [
    ([], None, None, None, None, ["filmic", "--srgb"], dict(curve="filmic", transfer="srgb")),
    (["--filter", "tent"], 0.5, (0.18, 0.5), "0.5,0.25,4", dict(strength=0.5, threshold=0.25, levels=4), ["filmic", "--srgb"], dict(curve="filmic", transfer="srgb")),
    (["--refill"], 2.0, (0.3, 0.25), None, None, ["reinhard,2.5", "--tone-luminance"], dict(curve="reinhard", transfer="gamma22", white=2.5, luminance=True)),
    ([], None, None, "0.3", dict(strength=0.3), ["reinhard"], dict(curve="reinhard", transfer="gamma22"))])
def test_tone_writes_the_python_faces_files(tmp_path, extra, compensation, key_rate, glare_arg, glare_kw, tone_args, tone_kw):
    args = ["--film", "pinhole", "--linear"] + ([str(compensation)] if compensation is not None else []) + extra
    args += ["--auto-exposure", "%g,%g" % key_rate] if key_rate else []
    args += (["--glare", glare_arg] if glare_arg else [])
    args += ["--tone"] + tone_args
    run_main(args, tmp_path / "shot.tga")
    splat = "--filter" in extra
    r, film, state, _ = python_face(splat, "--refill" in extra, compensation, key_rate, None)
    params = ptss.linear_params(exposure=1.0 if compensation is None else compensation)
    tone = ptss.tone_params(bits=8, **tone_kw)
    table = r.tone_build(tone)
    glare = None
    if glare_kw is not None:
        g = ptss.glare_params(**glare_kw)
        glare = (W, H, g, r.glare_build(film, W, H, params, g))
    linear, pixels, _ = (r.resolve_splat if splat else r.resolve_linear)(film, params=params, metered=state, glare=glare, tone=(tone, table))
    assert r.tone_launches() == (1, 1) and (state is None) == (key_rate is None)
    assert np.array_equal(read_tga(tmp_path / "shot.tga"), pixels[:, :3]) and 0 < int(pixels[:, :3].max()) and (pixels[:, 3] == 255).all()
    means = np.stack([linear["r"], linear["g"], linear["b"]], axis=1)
    assert read_pfm(tmp_path / "shot.pfm").tobytes() == means.tobytes() and means.max() > 0
    r.close()


def test_tone_clamp_writes_the_bytes_of_the_run_without_the_flag(tmp_path):
    same = lambda a, b: open(tmp_path / (a + ".pfm"), "rb").read() == open(tmp_path / (b + ".pfm"), "rb").read()
    args = ["--film", "pinhole", "--linear", "0.5"]
    plain, _ = run_main(args, tmp_path / "plain.tga")
    clamp, _ = run_main(args + ["--tone", "clamp"], tmp_path / "clamp.tga")
    assert clamp == plain and same("clamp", "plain")
    filmic, _ = run_main(args + ["--tone", "filmic", "--srgb"], tmp_path / "filmic.tga")
    assert len(filmic) == len(plain) and filmic != plain and same("filmic", "plain")   # another curve is another image of the same means
    args = ["--film", "pinhole", "--linear", "--filter", "tent", "--auto-exposure", "--glare", "0.4"]   # the splat film, a state, a pyramid
    plain, _ = run_main(args, tmp_path / "plain2.tga")
    clamp, _ = run_main(args + ["--tone", "clamp"], tmp_path / "clamp2.tga")
    assert clamp == plain and same("clamp2", "plain2")


def test_tone_arguments_are_checked(tmp_path):
    base = ["--film", "pinhole", "--linear"]
    for args in (["--film", "pinhole", "--tone", "filmic"], base + ["--tone", "aces"], base + ["--tone", "reinhard,0"], base + ["--tone", "reinhard,70000"],
                 base + ["--tone", "reinhard,4x"], base + ["--srgb"]):
        r = subprocess.run([MAIN] + ARGS + args + ["--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--tone" in r.stderr, args
