"""The small bodies the C-ABI files share (csrc/ptss_context.h): every ptss_*_launches getter copies exactly the words its header
parameter names, every ptss_debug_*_form setter accepts exactly its set and leaves the form alone when it refuses, and the rejected
read-backs work before any call of their family. Widths, sets and texts are literals here, taken from include/ptss.h and from the
library's source before the getters and setters were folded into helpers.

Nothing is rendered: a 64 x 4 context of the default scene, one sample per pass, and the smallest calls that launch."""
import ctypes as C

import numpy as np
import pytest

import ptss

pytestmark = pytest.mark.gpu

EINVAL = -1   # PTSS_EINVAL
SENTINEL = 0xA5A5A5A5A5A5A5A5
NULL_ARGUMENT = "null argument"
# name -> outK of include/ptss.h
LAUNCH_GETTERS = {
    "ptss_specular_feature_launches": 2, "ptss_chain_launches": 2, "ptss_path_launches": 2, "ptss_film_launches": 3, "ptss_adaptive_launches": 2,
    "ptss_linear_launches": 2, "ptss_linear_stats_launches": 2, "ptss_meter_launches": 3, "ptss_glare_launches": 3, "ptss_denoise_linear_launches": 2,
    "ptss_reproject_linear_launches": 1, "ptss_upsample_linear_launches": 1, "ptss_tone_launches": 2, "ptss_surface_launches": 2,
    "ptss_lightmap_launches": 1, "ptss_lightmap_chain_launches": 1, "ptss_upsample_launches": 1, "ptss_resort_launches": 1,
}
STATS = {"ptss_splat_stats": 5, "ptss_path_refill_stats": 5}
REJECTED = {"ptss_film_rejected": 1, "ptss_surface_rejected": 1, "ptss_update_rejected": 1}
GETTERS = dict(LAUNCH_GETTERS, **STATS, ptss_launched_kernels=1)

W, H, FACTOR = 4, 4, 2
P = W * H


@pytest.fixture
def ctx():
    r = ptss.Renderer(ptss.Scene("cornell"), 64, 4, max_iterations=2)
    yield r, ptss.device_lib()
    r.close()


def read(L, r, name, k):
    """The k + 1 words around a getter's call: k documented ones and the one behind them."""
    out = (C.c_ulonglong * (k + 1))(*([SENTINEL] * (k + 1)))
    assert getattr(L, name)(r._ctx, out) == 0, name
    assert out[k] == SENTINEL, f"{name} wrote more than {k} words"
    return [int(v) for v in out[:k]]


def detail(L):
    return L.ptss_last_error_detail().decode()


def film_rows():
    film = np.zeros(P, dtype=ptss.LINEAR_DTYPE)
    film["r"], film["g"], film["b"] = np.arange(P) << 18, 1 << 19, (P - np.arange(P)) << 17
    film["samples"] = 2
    return film


def test_getters_on_a_fresh_context_write_their_documented_words(ctx):
    r, L = ctx
    assert len(LAUNCH_GETTERS) == 18
    for name, k in dict(GETTERS, **REJECTED).items():
        assert read(L, r, name, k) == [0] * k, name


def test_getters_after_one_launch_of_each_width(ctx):
    r, L = ctx
    r.lookup_lightmap(np.zeros(2, dtype=ptss.HIT_DTYPE), np.zeros(4, dtype=ptss.LINEAR_DTYPE), ptss.lightmap_params(2, 2))   # misses: no block
    r.dilate_linear(film_rows(), W, H)
    rays = np.zeros(1, dtype=ptss.RAY_DTYPE)
    rays["direction"], rays["tmax"] = (0, 0, -1), np.inf
    r.ray_features(rays)
    assert read(L, r, "ptss_lightmap_launches", 1) == [1]
    assert read(L, r, "ptss_surface_launches", 2) == [0, 1]
    assert read(L, r, "ptss_film_launches", 3) == [0, 0, 1]
    moved = {"ptss_lightmap_launches", "ptss_surface_launches", "ptss_film_launches"}
    for name, k in GETTERS.items():
        if name not in moved:
            assert read(L, r, name, k) == [0] * k, name


def test_getters_refuse_null_arguments(ctx):
    r, L = ctx
    for name, k in dict(GETTERS, **REJECTED).items():
        out = (C.c_ulonglong * (k + 1))(*([SENTINEL] * (k + 1)))
        assert getattr(L, name)(None, out) == EINVAL and detail(L) == NULL_ARGUMENT, name
        assert list(out) == [SENTINEL] * (k + 1), name
        assert getattr(L, name)(r._ctx, None) == EINVAL and detail(L) == NULL_ARGUMENT, name


def dilate(r):
    return r.dilate_linear(film_rows(), W, H).tobytes()


def toned(r):
    tone = ptss.tone_params(bits=8)
    return b"".join(a.tobytes() for a in r.resolve_linear(film_rows(), tone=(tone, r.tone_build(tone))))


def lightmap(r):
    got, info = r.lookup_lightmap(np.zeros(2, dtype=ptss.HIT_DTYPE), film_rows()[:4], ptss.lightmap_params(2, 2))
    return got.tobytes() + info.tobytes()


def features(n):
    f = np.zeros(n, dtype=ptss.FEATURE_DTYPE)
    f["normal"], f["depth"], f["albedo"] = (0, 0, 1), 1.0, 0.5
    return f


def denoised(r):
    moments = np.zeros(P, dtype=ptss.MOMENT_DTYPE)
    moments["samples"] = 2
    return r.denoise_linear(film_rows(), W, H, moments, features(P)).tobytes()


def upsampled(r):
    got, info = r.upsample_linear(film_rows(), W, H, features(P), features(FACTOR * FACTOR * P), upsample=ptss.upsample_linear_params(factor=FACTOR))
    return got.tobytes() + info.tobytes()


THREE = "form must be 0, 1 or 2"
FORMS = {
    "ptss_debug_tone_form": ((0, 1, 2), (-1, 3), THREE, toned),
    "ptss_debug_dilate_linear_form": ((0, 1, 2), (-1, 3), THREE, dilate),
    "ptss_debug_lightmap_form": ((0, 1, 2), (-1, 3), THREE, lightmap),
    "ptss_debug_upsample_linear_form": ((0, 1, 2), (-1, 3), THREE, upsampled),
    "ptss_debug_denoise_linear_form": ((0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11), (-1, 3, 12), "form must be 0, 1, 2 or 4 .. 11", denoised),
}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_form_setters_accept_their_set_and_keep_the_form_when_they_refuse(ctx, name):
    r, L = ctx
    accepted, outside, text, feature = FORMS[name]
    setter = getattr(L, name)
    for form in accepted:
        assert setter(r._ctx, form) == 0, (name, form)
    assert setter(r._ctx, 1) == 0
    before = feature(r)
    for form in outside:
        assert setter(r._ctx, form) == EINVAL and detail(L) == text, (name, form)
        assert feature(r) == before, (name, form)
    assert setter(None, 0) == EINVAL and detail(L) == "ctx is null"


def test_rejected_read_backs_before_any_call_of_their_family(ctx):
    r, L = ctx
    for name in REJECTED:
        assert read(L, r, name, 1) == [0], name
