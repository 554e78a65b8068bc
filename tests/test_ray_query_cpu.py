"""Batched ray queries without a GPU: the new C-ABI symbols, the ctypes / numpy mirrors of ptss_ray_query and ptss_ray_hit
against what a C compiler makes of the headers, ptss_camera_ray against the oracle's eye ray, and the argument checks of
ptss_intersect / ptss_occluded that must not touch a device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
import ptss
from ptss_types import RayHit, RayQuery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

FIELDS = {
    "ptss_ray_query": (RayQuery, ptss.RAY_DTYPE, ["origin", "tmax", "direction", "pad"]),
    "ptss_ray_hit": (RayHit, ptss.HIT_DTYPE, ["point", "distance", "normal", "materialIdx", "kind", "primitive", "w1", "w2"]),
}


def test_new_symbols_are_exported():
    dev = C.CDLL(ptss.DEVICE_LIB)
    host = C.CDLL(ptss.HOST_LIB)
    for name in ("ptss_intersect", "ptss_occluded"):
        assert hasattr(dev, name), name
    assert hasattr(host, "ptss_camera_ray")


@pytest.mark.parametrize("struct", sorted(FIELDS))
def test_mirrors_match_the_c_layout(struct, tmp_path):
    cls, dtype, names = FIELDS[struct]
    prints = "".join(f'printf(" %zu", offsetof({struct}, {n}));' for n in names)
    src = (f'#include <stdio.h>\n#include <stddef.h>\n#include "ptss.h"\n'
           f'int main(void){{printf("%zu", sizeof({struct})); {prints} return 0;}}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe], input=src.encode(), check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(cls) == dtype.itemsize
    assert got[1:] == [getattr(cls, n).offset for n in names] == [dtype.fields[n][1] for n in names]


def cameras():
    a = ptss.default_camera()
    b = ptss.default_camera()
    for k in "wwdft":
        ptss.move_camera(b, k)
    c = ptss.default_camera()
    c.position.x, c.position.y, c.position.z = 0.3, -0.7, 2.5
    c.fieldOfView = 1.1
    c.zNear = 0.37
    for k in "hhgq":
        ptss.move_camera(c, k)
    return [a, b, c]


@pytest.mark.parametrize("w,h", [(64, 64), (37, 23), (16, 90)])
def test_camera_ray_is_the_frames_eye_ray(w, h):
    seed = 0x5EED
    pixels = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 3), (w // 3, h - 2)}
    for cam in cameras():
        for x, y in sorted(pixels):
            _, _, uni = oracle.probe_rng(seed, y * w + x, 2)
            ray = ptss.camera_ray(cam, w, h, x, y, (float(uni[0]), float(uni[1])))
            want = oracle.probe_eye_ray(x, y, w, h, cam, seed)
            assert ray[:3].tobytes() == want[:3].tobytes(), (x, y)
            assert ray[4:7].tobytes() == want[3:6].tobytes(), (x, y)
            assert math.isinf(ray[3]) and ray[3] > 0 and ray[7] == 0


def test_camera_rays_are_row_major_pixel_centres():
    cam = cameras()[1]
    rays = ptss.camera_rays(cam, 7, 5)
    assert rays.shape == (35, 8) and rays.dtype == np.float32
    for x, y in ((0, 0), (6, 0), (3, 4)):
        assert rays[y * 7 + x].tobytes() == ptss.camera_ray(cam, 7, 5, x, y).tobytes()


def test_camera_ray_argument_checks():
    cam = ptss.default_camera()
    L = ptss.host_lib()
    q = RayQuery()
    assert L.ptss_camera_ray(None, 4, 4, 0, 0, 0.5, 0.5, C.byref(q)) < 0
    assert L.ptss_camera_ray(C.byref(cam), 4, 4, 0, 0, 0.5, 0.5, None) < 0
    assert L.ptss_camera_ray(C.byref(cam), 0, 4, 0, 0, 0.5, 0.5, C.byref(q)) < 0


def test_make_rays():
    r = ptss.make_rays([[1, 2, 3], [4, 5, 6]], [[0, 0, -1], [1, 0, 0]], tmax=[2.0, 7.0])
    assert r.shape == (2, 8)
    assert r.view(ptss.RAY_DTYPE).reshape(-1)["tmax"].tolist() == [2.0, 7.0]
    assert r[1, 4:7].tolist() == [1, 0, 0] and r[0, 7] == 0
    assert np.isinf(ptss.make_rays([0, 0, 0], [0, 0, 1])[0, 3])


def test_query_argument_checks_without_a_device():
    """A null context, null buffers with n > 0 and n = 0 are answered on the host (no GPU is needed to get here)."""
    L = ptss.device_lib()
    buf = (C.c_float * 16)()
    for fn in (L.ptss_intersect, L.ptss_occluded):
        assert fn(None, buf, buf, 1, None) == -1           # PTSS_EINVAL: null context
        assert fn(None, None, None, 0, None) == -1         # ... even with n = 0
        assert fn(C.c_void_p(1), None, buf, 0, None) == 0  # n = 0: nothing to do, nothing touched
        assert fn(C.c_void_p(1), None, buf, 5, None) == -1
        assert fn(C.c_void_p(1), buf, None, 5, None) == -1
        assert fn(C.c_void_p(1), buf, buf, 1 << 31, None) == -5   # PTSS_ERANGE
