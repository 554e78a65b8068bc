"""Cases and expected values shared by tests/test_film_cpu.py and tests/test_gpu_film.py (ptss_generate_rays / ptss_accumulate_paths /
ptss_ray_features).

The main pin is an identity in the style of tests/path_query_common.py: a pinhole film of the frame's size, fed the context's seed
(ptss_seed_path_rng(seed, 0, skip = 0)) and run generate -> trace -> accumulate once per frame, reproduces the frame loop's integer
accumulator, display pixels and stream states bit for bit, frame after frame — as long as the loop guard (`numRays > 128`,
CudaTracer.cu:622) fires in none of the frames used, because a path query has no such guard. The cases are path_query_common's; the
oracle's consecutive frames are computed here once per process. test_film_cpu.py checks the condition over FRAMES frames without a GPU;
a case that violated it would be replaced in path_query_common's style, never skipped."""
import ctypes as C

import numpy as np

import oracle
import ptss
from path_query_common import CASES, H, N, SCENES, W, camera_of, make_scene, satisfies_identity_condition

FRAMES = 4    # consecutive frames the condition is checked over
ROUNDS = 3    # of which the GPU identity uses the first three


class Frames:
    """FRAMES consecutive frames of the oracle: per frame the accumulator, the display pixels, every stream's state and the live counts."""

    def __init__(self, desc, cam, iterations, seed, frames=FRAMES, width=W, height=H):
        o = oracle.Oracle(desc, width, height, max_iterations=iterations, seed=seed)
        o.set_camera(cam)
        self.accum, self.pixels, self.states, self.live_counts = [], [], [], []
        for _ in range(frames):
            o.generate_frame()
            self.accum.append(o.accumulator())
            self.pixels.append(o.pixels())
            self.states.append(np.array([o.rng_state(p) for p in range(width * height)], dtype=np.uint32))
            self.live_counts.append(o.live_counts())
        o.close()


_FRAMES = {}


def frames_of(name, iterations):
    if (name, iterations) not in _FRAMES:
        _FRAMES[(name, iterations)] = Frames(make_scene(name).desc, camera_of(name), iterations, SCENES[name][3])
    return _FRAMES[(name, iterations)]


def words(a):
    """The 32-bit words of a record or float array, one row per entry."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def seeded_states(seed, n, first=0):
    """(n, 6) uint32: curand_init(seed, first + i, 0) on the oracle."""
    return np.array([oracle.probe_rng(seed, first + i, 0)[0] for i in range(n)], dtype=np.uint32)


def oracle_state_after(seed, sequence, draws):
    """(the state of the oracle's stream curand_init(seed, sequence, 0) after `draws` draws, their uniforms). The oracle reports the
    seeded state and the raw draws; XORWOW shifts v by one word per draw and appends raw - d, d growing by 362437."""
    state, raw, uni = oracle.probe_rng(seed, sequence, draws)
    d = (int(state[5]) + 362437 * np.arange(1, draws + 1)) % 2 ** 32
    v = np.concatenate([state[:5].astype(np.int64), (raw.astype(np.int64) - d) % 2 ** 32])[draws:draws + 5]
    return np.concatenate([v, [(int(state[5]) + 362437 * draws) % 2 ** 32]]).astype(np.uint32), uni


def advance(state6, draws):
    """`draws` draws of the host XORWOW (ptss_probe_rng_draw; pinned against the oracle by test_film_cpu) -> (state afterwards, uniforms)."""
    s = np.array(state6, dtype=np.uint32)
    raw, uni = np.zeros(max(draws, 1), np.uint32), np.zeros(max(draws, 1), np.float32)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    assert ptss.host_lib().ptss_probe_rng_draw(s.ctypes.data_as(u32p), raw.ctypes.data_as(u32p), uni.ctypes.data_as(f32p), draws) == 0
    return s, uni[:draws]


def turned_camera():
    """A camera away from the origin, turned about two axes (a unit quaternion), the reference's zNear and field of view."""
    cam = ptss.default_camera()
    for key in "fftg":
        ptss.move_camera(cam, key)
    cam.position.x, cam.position.y, cam.position.z = 0.3, -0.4, 1.25
    return cam


# the films of the device-equals-probe tests: (width, height); the batch sizes; and the three models
FILM_SIZES = ((1, 1), (5, 3), (64, 48), (3, 64))
BATCHES = (1, 63, 64, 65, 257)
LENS = dict(lens_radius=0.2, focus_distance=4.0)


def films(width, height, cam=None):
    """Every model with both jitter settings on a width x height film."""
    cam = cam if cam is not None else turned_camera()
    out = []
    for jitter in (1, 0):
        out.append(ptss.film_camera("pinhole", width, height, cam, jitter=jitter))
        out.append(ptss.film_camera("thinlens", width, height, cam, jitter=jitter, **LENS))
        out.append(ptss.film_camera("equirect", width, height, cam, jitter=jitter))
    return out


def quant_thresholds():
    T = np.empty(257, dtype=np.float32)
    assert ptss.host_lib().ptss_probe_quant_table(T.ctypes.data_as(C.POINTER(C.c_float))) == 0
    return T


def adversarial_radiance():
    """(M, 3) float32 radiance rows for the tone map: NaN, +-inf, negatives, zeros, denormals, every threshold of the table with its two
    float neighbours, 1 and beyond."""
    T = quant_thresholds()[1:256]
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 1e-45, 1e-38, -1e-30, 1.0, np.nextafter(np.float32(1), np.float32(0)),
                        np.nextafter(np.float32(1), np.float32(2)), 2.0, 255.0, 3e38, 0.5, 0.18], dtype=np.float32)
    v = np.concatenate([special, T, np.nextafter(T, np.float32(-1)), np.nextafter(T, np.float32(2))]).astype(np.float32)
    v = np.concatenate([v, np.zeros((-len(v)) % 3, dtype=np.float32)])
    g = np.random.default_rng(11)
    return np.concatenate([v.reshape(-1, 3), g.permutation(v).reshape(-1, 3), g.permutation(v).reshape(-1, 3)])


def results_of(radiance):
    r = np.zeros(len(radiance), dtype=ptss.PATH_RESULT_DTYPE)
    r["radiance"] = radiance
    r["bounces"] = 1
    return r
