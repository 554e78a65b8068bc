"""Bounce 0 visits only the primitives its strip's word names (csrc/ptstrip.h): the frames must stay the oracle's, bit
for bit, and the words must be the ones of the CURRENT camera and scene.

  * `mixed` and `lambert` at 33 x 17, 130 x 9 and 256 x 64, one and five sample lanes, one and two frame lanes, and as shards of two
    and three ranks: accumulator, display pixels, float sums and ray counts equal the oracle's;
  * the scenes a frustum cull gets wrong (tests/strip_mask_common.py: tiny far primitives, tangent spheres, the camera inside and
    1e-4 off a sphere, walls edge-on and around the grazing threshold, vertices behind the camera) at those sizes, the same;
  * in every case the context reports that bounce 0 read the words, and the words it read are the ones the host build of the same
    header computes for that camera, scene and frame shape (so a test that passes has culled, and with fresh words);
  * recompute on a live context, each against a fresh context: a camera move that changes every strip's word, ptss_set_scene to a
    scene with other primitive counts, ptss_update_triangles. An image small enough for the words stores its triangles grouped by
    edge class, and ptss_update_triangles refuses such images (ptss_set_scene replaces them): the test pins the refusal, with the
    words and frames untouched by it, and moves the wall of a mesh image — where bounce 0 visits everything, before and after."""
import numpy as np
import pytest

import oracle
import ptss
import tiles
from scene_update_common import deform, m530
from strip_mask_common import adversarial_cases, camera, tiny_scene

pytestmark = pytest.mark.gpu

SIZES = [(33, 17), (130, 9), (256, 64)]
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
SEED = 0x5EED


def words_are_current(r, scene, cam, w, h, band=8, rank=0, world=1):
    words, on = r.strip_words()
    want, want_on, _ = ptss.probe_strip_masks(scene, cam, w, h, band, rank, world)
    assert on and want_on
    assert np.array_equal(words, want)
    return words


def against_oracle(scene, w, h, cam=None, S=1, lanes=1, world=1, band=8, bounces=3, frames=2):
    cam = cam or ptss.default_camera()
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    o.set_camera(cam)
    rs = [ptss.Renderer(scene, w, h, max_iterations=bounces, tile_rank=k, tile_world=world, band_rows=band, float_accumulator=True,
                        samples_per_pass=S, frame_lanes=lanes) for k in range(world)]
    for r in rs:
        r.set_camera(cam)
    for _ in range(frames):
        o.generate_frame()
        for r in rs:
            r.generate_frame()
    culled = 0
    for k, r in enumerate(rs):
        if r.local_pixels:
            words = words_are_current(r, scene, cam, w, h, band, k, world)
            culled += int((words != ALL).sum())
    acc = tiles.untile([r.accumulator() for r in rs], w, h, band)
    pix = tiles.untile([r.pixels() for r in rs], w, h, band)
    fsum = tiles.untile([r.float_accumulator() for r in rs], w, h, band)
    assert np.array_equal(acc, o.accumulator())
    assert np.array_equal(pix, o.pixels())
    assert np.array_equal(fsum, o.float_sum(), equal_nan=True)
    if world == 1:
        assert np.array_equal(rs[0].live_counts(), o.live_counts())
        assert rs[0].total_ray_bounces() == o.total_ray_bounces()
    for r in rs:
        r.close()
    return culled


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("preset", ["mixed", "lambert"])
def test_presets_match_the_oracle(preset, w, h, S, lanes):
    culled = against_oracle(ptss.Scene(preset), w, h, S=S, lanes=lanes)
    assert culled > 0 or w < 64   # (33 wide: most strips cover two rows and still lose bits; none is required to)


@pytest.mark.parametrize("world,band", [(2, 8), (3, 4)])
@pytest.mark.parametrize("w,h", [(130, 9), (256, 64)])
def test_shards_match_the_oracle(w, h, world, band):
    assert against_oracle(ptss.Scene("mixed"), w, h, world=world, band=band, cam=camera(keys="hq")) > 0


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("case", range(6))
def test_adversarial_scenes_match_the_oracle(case, w, h):
    name, scene, cam = adversarial_cases(w, h)[case]
    against_oracle(scene, w, h, cam=cam, S=1 + 4 * (case % 2), bounces=2)


def frames_of(r, n=2):
    for _ in range(n):
        r.generate_frame()
    return r.accumulator(), r.pixels(), r.float_accumulator()


def same_frames(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_camera_move_recomputes_the_words():
    w, h = 256, 64
    scene, cam2 = ptss.Scene("mixed"), camera((0.4, -0.2, -0.5), keys="hhg")
    r = ptss.Renderer(scene, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    frames_of(r)
    before = words_are_current(r, scene, ptss.default_camera(), w, h)
    r.set_camera(cam2)
    assert not r.strip_words()[1]   # no frame yet under the new camera: nothing to read
    r.reseed(SEED)
    got = frames_of(r)
    after = words_are_current(r, scene, cam2, w, h)
    real = w * h // 64
    assert (before[:real] != after[:real]).all()   # the pose changes every strip's word
    fresh = ptss.Renderer(scene, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    fresh.set_camera(cam2)
    assert same_frames(got, frames_of(fresh))
    r.close()
    fresh.close()


def test_set_scene_recomputes_the_words():
    w, h = 130, 9
    first, second = ptss.Scene("mixed"), tiny_scene(w, h)   # 22 + 16 primitives, then 9 + 6
    r = ptss.Renderer(first, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    frames_of(r)
    words_are_current(r, first, ptss.default_camera(), w, h)
    r.set_scene(second)
    r.reseed(SEED)
    got = frames_of(r)
    words_are_current(r, second, ptss.default_camera(), w, h)
    fresh = ptss.Renderer(second, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    assert same_frames(got, frames_of(fresh))
    # ... and to a scene outside the cull's domain (a mesh image): bounce 0 visits everything again
    r.set_scene(m530())
    frames_of(r, 1)
    words, on = r.strip_words()
    assert not on and (words == ALL).all()
    r.close()
    fresh.close()


def test_update_triangles_on_live_contexts():
    w, h = 130, 9
    # an image with words: the update is refused (edge-classed storage), words and frames stay what they were
    scene = ptss.Scene("mixed")
    r = ptss.Renderer(scene, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    frames_of(r)
    table = np.zeros(2, dtype=ptss.TRIANGLE_DTYPE)
    with pytest.raises(ptss.PtssError):
        r.update_triangles(table, first=8)
    words_are_current(r, scene, ptss.default_camera(), w, h)
    r.reseed(SEED)
    fresh = ptss.Renderer(scene, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    assert same_frames(frames_of(r), frames_of(fresh))
    r.close()
    fresh.close()
    # a mesh image: the wall (and everything else) moves, bounce 0 visits everything before and after
    mesh = m530()
    moved = deform(mesh.triangles)
    r = ptss.Renderer(mesh, w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    frames_of(r)
    assert not r.strip_words()[1]
    r.update_triangles(moved)
    r.reseed(SEED)
    got = frames_of(r)
    assert not r.strip_words()[1]
    fresh = ptss.Renderer(mesh.with_triangles(moved), w, h, max_iterations=3, float_accumulator=True, seed=SEED)
    assert same_frames(got, frames_of(fresh))
    r.close()
    fresh.close()


def test_read_strip_words_argument_checks():
    import ctypes as C
    L = ptss.device_lib()
    n, on = C.c_size_t(), C.c_int()
    buf = (C.c_ulonglong * 4)()
    assert L.ptss_read_strip_words(None, buf, 4, C.byref(n), C.byref(on)) == -1
    r = ptss.Renderer(ptss.Scene("mixed"), 130, 9, max_iterations=2)
    assert L.ptss_read_strip_words(r._ctx, buf, 4, C.byref(n), C.byref(on)) == -1 and n.value == 20   # 1,170 pixels: a plane of 1,280
    words, enabled = r.strip_words()
    assert not enabled and len(words) == 20 and (words == ALL).all()   # no frame yet
    r.close()
