"""The binding's own refusals (ptss.py): the ValueErrors a Renderer wrapper raises before the library is reached, on the tensor path and
on the array path, each with its literal text; no refusal moves a counter or touches a buffer. And what every wrapper does with a
zero-size call: it reaches the library with null pointers, or it returns early.

Nothing here launches more than the sentinel fills: every input is refused on the host."""
import numpy as np
import pytest

import ptss
from ptss_types import FILM_DTYPE, LINEAR_DTYPE, METER_BINS, METER_STATE_DTYPE, MOMENT_DTYPE, PATH_RESULT_DTYPE, PATH_RNG_DTYPE, POSITION_DTYPE, SPLAT_DTYPE

pytestmark = pytest.mark.gpu

N, W, H, FACTOR = 16, 4, 4, 2   # rays; the film; upsample_linear's factor
P = W * H
FILM = ptss.film_camera("pinhole", W, H)
GLARE = ptss.glare_params(levels=2)
TONE = ptss.tone_params(bits=8)
UPSAMPLE = ptss.upsample_linear_params(factor=FACTOR)
PYRAMID = ptss.glare_layout(W, H, GLARE.levels)[1]
WORKSPACE = ptss.denoise_linear_workspace(W, H)
COUNTERS = ("film_launches", "film_rejected", "adaptive_launches", "linear_launches", "linear_stats_launches", "splat_stats", "meter_launches",
            "glare_launches", "tone_launches", "denoise_linear_launches", "reproject_linear_launches", "upsample_linear_launches", "path_launches",
            "path_refill_stats", "upsample_launches", "specular_feature_launches", "resort_launches", "update_rejected", "launched_kernels")


def counters(r):
    return [getattr(r, name)() for name in COUNTERS]


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    r = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    gone = ptss.Renderer(ptss.Scene("cornell"), 16, 16, max_iterations=2)
    gone.close()   # a context the library refuses: whoever reaches the library hears of it
    yield torch, r, gone
    r.close()


def test_the_sizes_the_messages_below_spell_out():
    assert (METER_BINS, PYRAMID, WORKSPACE, ptss.tone_table_floats(TONE.bits)) == (329, 5, 832, 260)
    assert (ptss.plan_cdf_entries(P), ptss.plan_cdf_entries(P + 1)) == (CDF, CDF_17)


CDF, CDF_17 = 19, 20   # plan_cdf_entries(16), plan_cdf_entries(17)

# ---- 1. the tensor path ----------------------------------------------------------------------------------------------------------------
CASES = ("dtype", "columns", "rows", "strided", "cpu", "numpy")
OTHER_DTYPE = {"float32": "float64", "int32": "int64", "int64": "int32", "uint8": "int8"}
QUERY_RAYS = "rays: a contiguous (N, 8) float32 device tensor"
TRACE_RNG = "rng: a contiguous (N, 6) int32 tensor on the rays' device"
RESULTS = "results: a contiguous float32 device tensor of shape (N, 4)"
INDEX, INDEX_17 = "index: a contiguous int32 device tensor of shape (16)", "index: a contiguous int32 device tensor of shape (17)"
FILM_N32, FILM_N64 = "film: a contiguous int32 device tensor of shape (N, 4)", "film: a contiguous int64 device tensor of shape (N, 4)"
FILM_16 = "film: a contiguous int64 device tensor of shape (16, 4)"
PIXELS, HISTORY = "pixels: a contiguous uint8 device tensor of shape (16, 4)", "history: a contiguous float32 device tensor of shape (16, 4)"
LINEAR = "linear: a contiguous float32 device tensor of shape (16, 4)"
MOMENTS_1 = "moments: a contiguous int64 device tensor of shape (16)"
MOMENTS_N4, MOMENTS_4 = "moments: a contiguous int64 device tensor of shape (N, 4)", "moments: a contiguous int64 device tensor of shape (16, 4)"
CDF_TEXT, PLAN_INDEX = "cdf: a contiguous int64 device tensor of shape (19)", "index: a contiguous int32 device tensor of shape (16)"
PLAN_INFO = "info: a contiguous int64 device tensor of shape (4)"
HISTOGRAM, STATE = "histogram: a contiguous int32 device tensor of shape (329)", "state: a contiguous int64 device tensor of shape (6)"
METERED, PYRAMID_TEXT = "metered: a contiguous int64 device tensor of shape (6)", "pyramid: a contiguous int64 device tensor of shape (5, 4)"
TABLE = "table: a contiguous float32 device tensor of shape (260)"
POSITIONS = "positions: a contiguous float32 device tensor of shape (16, 2)"
OUT_16, OUT_64 = "out: a contiguous int64 device tensor of shape (16, 4)", "out: a contiguous int64 device tensor of shape (64, 4)"
FEATURES_NOW = "features_now: a contiguous float32 device tensor of shape (16, 8)"


def primary(text, rows=None, **more):
    """The expectations of a wrapper's primary argument: `text` for every case but "numpy" (the array path) and "rows" (who refuses then)."""
    return dict({"*": text, "rows": rows, "numpy": None}, **more)


RESOLVE_ARGS = dict(film=("int64", (P, 4)), linear=("float32", (P, 4)), pixels=("uint8", (P, 4)), history=("float32", (P, 4)))
TONED_ARGS = dict(RESOLVE_ARGS, metered=("int64", (6,)), pyramid=("int64", (PYRAMID, 4)), table=("float32", (260,)))
RESOLVE_TEXTS = dict(film=primary(FILM_N64, rows="linear: a contiguous float32 device tensor of shape (17, 4)"), linear=LINEAR, pixels=PIXELS,
                     history=HISTORY)
TONED_TEXTS = dict(RESOLVE_TEXTS, film=primary(FILM_N64, rows="film: width * height entries"), metered=METERED, pyramid=PYRAMID_TEXT, table=TABLE)
ACCUMULATE_ARGS = dict(results=("float32", (N, 4)), film=("int32", (P, 4)), index=("int32", (N,)), pixels=("uint8", (P, 4)),
                       history=("float32", (P, 4)))
PLAN_ARGS = dict(cdf=("int64", (CDF,)), index=("int32", (N,)), info=("int64", (4,)))
PLAN_TEXTS = dict(cdf=CDF_TEXT, index=PLAN_INDEX, info=PLAN_INFO)


def toned(resolve):
    return lambda r, a: getattr(r, resolve)(a["film"], linear=a["linear"], pixels=a["pixels"], history=a["history"], metered=a["metered"],
                                            glare=(W, H, GLARE, a["pyramid"]), tone=(TONE, a["table"]))


# wrapper -> (the call over its good arguments, argument -> (dtype, shape), argument -> the refusal's text: one for every case, or per case
# with "*" for the rest; None: the binding does not refuse that case)
TENSOR_CALLS = {
    "intersect": (lambda r, a: r.intersect(a["rays"]), dict(rays=("float32", (N, 8))), dict(rays=primary(QUERY_RAYS))),
    "occluded": (lambda r, a: r.occluded(a["rays"]), dict(rays=("float32", (N, 8))), dict(rays=primary(QUERY_RAYS))),
    "trace_paths": (lambda r, a: r.trace_paths(a["rays"], a["rng"], 2), dict(rays=("float32", (N, 8)), rng=("int32", (N, 6))),
                    dict(rays=primary(QUERY_RAYS, rows=TRACE_RNG), rng=TRACE_RNG)),
    "trace_paths_refill": (lambda r, a: r.trace_paths(a["rays"], a["rng"], 2, schedule="refill"), dict(rays=("float32", (N, 8)), rng=("int32", (N, 6))),
                           dict(rays=primary(QUERY_RAYS, rows=TRACE_RNG), rng=TRACE_RNG)),
    "generate_rays": (lambda r, a: r.generate_rays(FILM, a["rng"], 0, a["index"], a["rays"]),
                      dict(rng=("int32", (N, 6)), rays=("float32", (N, 8)), index=("int32", (N,))),
                      dict(rng=primary("rng: a contiguous int32 device tensor of shape (N, 6)", rows="rays: a contiguous float32 device tensor of shape (17, 8)"),
                           rays="rays: a contiguous float32 device tensor of shape (16, 8)", index=INDEX)),
    "generate_rays_positions": (lambda r, a: r.generate_rays(FILM, a["rng"], 0, None, None, a["positions"]),
                                dict(rng=("int32", (N, 6)), positions=("float32", (N, 2))),
                                dict(rng=primary("rng: a contiguous int32 device tensor of shape (N, 6)",
                                                 rows="positions: a contiguous float32 device tensor of shape (17, 2)"), positions=POSITIONS)),
    "accumulate_paths": (lambda r, a: r.accumulate_paths(a["results"], a["film"], 0, a["index"], a["pixels"], a["history"]), ACCUMULATE_ARGS,
                         dict(results=primary(RESULTS, rows=INDEX_17), film={"*": FILM_N32, "rows": "pixels: a contiguous uint8 device tensor of shape (17, 4)"},
                              index=INDEX, pixels=PIXELS, history=HISTORY)),
    "accumulate_paths_stats": (lambda r, a: r.accumulate_paths_stats(a["results"], a["film"], a["moments"], 0, a["index"], a["pixels"], a["history"]),
                               dict(ACCUMULATE_ARGS, moments=("int64", (P,))),
                               dict(results=primary(RESULTS, rows=INDEX_17), film={"*": FILM_N32, "rows": "moments: a contiguous int64 device tensor of shape (17)"},
                                    moments=MOMENTS_1, index=INDEX, pixels=PIXELS, history=HISTORY)),
    "accumulate_paths_linear": (lambda r, a: r.accumulate_paths_linear(a["results"], a["film"], 0, a["index"]),
                                dict(results=("float32", (N, 4)), film=("int64", (P, 4)), index=("int32", (N,))),
                                dict(results=primary(RESULTS, rows=INDEX_17), film={"*": FILM_N64, "rows": None}, index=INDEX)),
    "accumulate_paths_linear_stats": (lambda r, a: r.accumulate_paths_linear_stats(a["results"], a["film"], a["moments"], 0, a["index"]),
                                      dict(results=("float32", (N, 4)), moments=("int64", (P, 4)), film=("int64", (P, 4)), index=("int32", (N,))),
                                      dict(results=primary(RESULTS, rows=INDEX_17), moments={"*": MOMENTS_N4, "rows": "film: a contiguous int64 device tensor of shape (17, 4)"},
                                           film=FILM_16, index=INDEX)),
    "ray_features": (lambda r, a: r.ray_features(a["rays"]), dict(rays=("float32", (N, 8))),
                     dict(rays=primary("rays: a contiguous float32 device tensor of shape (N, 8)"))),
    "plan_samples": (lambda r, a: r.plan_samples(a["film"], a["moments"], N, None, a["cdf"], a["index"], a["info"]),
                     dict(PLAN_ARGS, film=("int32", (P, 4)), moments=("int64", (P,))),
                     dict(PLAN_TEXTS, film=primary(FILM_N32, rows="moments: a contiguous int64 device tensor of shape (17)"), moments=MOMENTS_1)),
    "plan_samples_linear": (lambda r, a: r.plan_samples_linear(a["moments"], N, None, None, a["cdf"], a["index"], a["info"]),
                            dict(PLAN_ARGS, moments=("int64", (P, 4))),
                            dict(PLAN_TEXTS, moments=primary(MOMENTS_N4, rows="cdf: a contiguous int64 device tensor of shape (20)"))),
    "resolve_linear": (lambda r, a: r.resolve_linear(a["film"], linear=a["linear"], pixels=a["pixels"], history=a["history"]), RESOLVE_ARGS, RESOLVE_TEXTS),
    "resolve_splat": (lambda r, a: r.resolve_splat(a["film"], linear=a["linear"], pixels=a["pixels"], history=a["history"]), RESOLVE_ARGS, RESOLVE_TEXTS),
    "resolve_linear_metered": (lambda r, a: r.resolve_linear(a["film"], linear=a["linear"], pixels=None, history=None, metered=a["metered"]),
                               dict(film=("int64", (P, 4)), linear=("float32", (P, 4)), metered=("int64", (6,))),
                               dict(film=primary(FILM_N64, rows="linear: a contiguous float32 device tensor of shape (17, 4)"), linear=LINEAR, metered=METERED)),
    "resolve_splat_glare": (lambda r, a: r.resolve_splat(a["film"], linear=None, pixels=a["pixels"], history=None, glare=(W, H, GLARE, a["pyramid"])),
                            dict(film=("int64", (P, 4)), pixels=("uint8", (P, 4)), pyramid=("int64", (PYRAMID, 4))),
                            dict(film=primary(FILM_N64, rows="film: width * height entries"), pixels=PIXELS, pyramid=PYRAMID_TEXT)),
    "resolve_linear_toned": (toned("resolve_linear"), TONED_ARGS, TONED_TEXTS),
    "resolve_splat_toned": (toned("resolve_splat"), TONED_ARGS, TONED_TEXTS),
    "splat_paths": (lambda r, a: r.splat_paths(a["results"], a["positions"], a["film"], W, H),
                    dict(results=("float32", (N, 4)), positions=("float32", (N, 2)), film=("int64", (P, 4))),
                    dict(results=primary(RESULTS, rows="positions: a contiguous float32 device tensor of shape (17, 2)"), positions=POSITIONS, film=FILM_16)),
    "splat_paths_homed": (lambda r, a: r.splat_paths(a["results"], a["positions"], a["film"], W, H, homed_first_pixel=0),
                          dict(results=("float32", (N, 4)), positions=("float32", (N, 2)), film=("int64", (P, 4))),
                          dict(results=primary(RESULTS, rows="positions: a contiguous float32 device tensor of shape (17, 2)"), positions=POSITIONS, film=FILM_16)),
    "tone_build": (lambda r, a: r.tone_build(TONE, a["table"]), dict(table=("float32", (260,))), dict(table=TABLE)),   # a table at all: tensors
    "glare_build": (lambda r, a: r.glare_build(a["film"], W, H, glare=GLARE, pyramid=a["pyramid"]),
                    dict(film=("int64", (P, 4)), pyramid=("int64", (PYRAMID, 4))), dict(film=primary(FILM_16, rows=FILM_16), pyramid=PYRAMID_TEXT)),
    "denoise_linear": (lambda r, a: r.denoise_linear(a["film"], W, H, a["moments"], a["features"], out=a["out"], workspace=a["workspace"]),
                       dict(film=("int64", (P, 4)), moments=("int64", (P, 4)), features=("float32", (P, 8)), out=("int64", (P, 4)),
                            workspace=("uint8", (WORKSPACE,))),
                       dict(film=primary(FILM_16, rows=FILM_16), moments=MOMENTS_4, features="features: a contiguous float32 device tensor of shape (16, 8)",
                            out=OUT_16, workspace={"*": "workspace: a contiguous uint8 device tensor of shape (N)",
                                                   "rows": "workspace: denoise_linear_workspace(width, height) bytes"})),
    "reproject_linear": (lambda r, a: r.reproject_linear(FILM, a["features_now"], FILM, a["features_prev"], a["film_prev"], a["moments_prev"],
                                                         motion_now=a["motion_now"], out=a["out"], moments_out=a["moments_out"], info=a["info"]),
                         dict(features_now=("float32", (P, 8)), features_prev=("float32", (P, 8)), film_prev=("int64", (P, 4)),
                              moments_prev=("int64", (P, 4)), motion_now=("float32", (P, 4)), out=("int64", (P, 4)), moments_out=("int64", (P, 4)),
                              info=("int64", (4,))),
                         dict(features_now=FEATURES_NOW, features_prev="features_prev: a contiguous float32 device tensor of shape (16, 8)",
                              # the device is film_prev's, and features_now is the first to be held against it
                              film_prev=primary("film_prev: a contiguous int64 device tensor of shape (16, 4)",
                                                rows="film_prev: a contiguous int64 device tensor of shape (16, 4)", cpu=FEATURES_NOW),
                              moments_prev="moments_prev: a contiguous int64 device tensor of shape (16, 4)",
                              motion_now="motion_now: a contiguous float32 device tensor of shape (16, 4)", out=OUT_16,
                              moments_out="moments_out: a contiguous int64 device tensor of shape (16, 4)", info=PLAN_INFO)),
    "upsample_linear": (lambda r, a: r.upsample_linear(a["film_lo"], W, H, a["features_lo"], a["features_hi"], upsample=UPSAMPLE, out=a["out"], info=a["info"]),
                        dict(film_lo=("int64", (P, 4)), features_lo=("float32", (P, 8)), features_hi=("float32", (P * FACTOR ** 2, 8)),
                             out=("int64", (P * FACTOR ** 2, 4)), info=("int64", (3,))),
                        dict(film_lo=primary("film_lo: a contiguous int64 device tensor of shape (16, 4)",
                                             rows="film_lo: a contiguous int64 device tensor of shape (16, 4)"),
                             features_lo="features_lo: a contiguous float32 device tensor of shape (16, 8)",
                             features_hi="features_hi: a contiguous float32 device tensor of shape (64, 8)", out=OUT_64,
                             info="info: a contiguous int64 device tensor of shape (3)")),
    "meter_linear": (lambda r, a: r.meter_linear(a["film"], histogram=a["histogram"]), dict(film=("int64", (P, 4)), histogram=("int32", (METER_BINS,))),
                     dict(film=primary(FILM_N64), histogram=HISTOGRAM)),
    "meter_splat": (lambda r, a: r.meter_splat(a["film"], histogram=a["histogram"]), dict(film=("int64", (P, 4)), histogram=("int32", (METER_BINS,))),
                    dict(film=primary(FILM_N64), histogram=HISTOGRAM)),
    "meter_exposure": (lambda r, a: r.meter_exposure(a["histogram"], a["state"]), dict(histogram=("int32", (METER_BINS,)), state=("int64", (6,))),
                       dict(histogram=primary(HISTOGRAM, rows=HISTOGRAM), state=STATE)),
}


def sentinel(torch, dtype, shape):
    t = torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")
    t.view(torch.uint8).fill_(0x5A)
    return t


def wrong(torch, good, dtype, case, argument):
    """`good` made wrong in one respect."""
    rows, columns = good.shape[0], tuple(good.shape[1:])
    kind = getattr(torch, dtype)
    if case == "dtype":
        return torch.zeros(tuple(good.shape), dtype=getattr(torch, OTHER_DTYPE[dtype]), device="cuda")
    if case == "columns":
        return torch.zeros((rows, columns[0] + 1 if columns else 1), dtype=kind, device="cuda")
    if case == "rows":   # one more; a workspace may be larger, so one less
        return torch.zeros((rows - 1 if argument == "workspace" else rows + 1,) + columns, dtype=kind, device="cuda")
    if case == "strided":
        return torch.zeros((2 * rows,) + columns, dtype=kind, device="cuda")[::2]
    return good.cpu() if case == "cpu" else good.cpu().numpy()


@pytest.mark.parametrize("wrapper", sorted(TENSOR_CALLS))
def test_tensor_refusals_keep_their_text_and_touch_nothing(gpu, wrapper):
    torch, r, _ = gpu
    call, arguments, texts = TENSOR_CALLS[wrapper]
    good = {name: sentinel(torch, dtype, shape) for name, (dtype, shape) in arguments.items()}
    torch.cuda.synchronize()
    before, refused = counters(r), 0
    for name, (dtype, _) in arguments.items():
        for case in CASES:
            text = texts[name]
            if isinstance(text, dict):
                text = text.get(case, text.get("*"))
            if text is None:
                continue
            bad = dict(good, **{name: wrong(torch, good[name], dtype, case, name)})
            with pytest.raises(ValueError) as e:
                call(r, bad)
            assert str(e.value) == text, (wrapper, name, case)
            refused += 1
    assert refused >= 4 * len(arguments)
    assert counters(r) == before
    torch.cuda.synchronize()
    for name, t in good.items():
        assert bool((t.view(torch.uint8) == 0x5A).all()), (wrapper, name)


def test_a_range_outside_the_film_is_refused_on_tensors_too(gpu):
    torch, r, _ = gpu
    film, histogram = sentinel(torch, "int64", (P, 4)), sentinel(torch, "int32", (METER_BINS,))
    before = counters(r)
    for first, count in ((1, P), (0, P + 1), (-1, 1), (0, -1), (P + 1, None)):
        for call in (lambda: r.resolve_linear(film, first, count, linear=None, pixels=None, history=None),
                     lambda: r.resolve_splat(film, first, count, linear=None, pixels=None, history=None),
                     lambda: r.meter_linear(film, first, count, histogram), lambda: r.meter_splat(film, first, count, histogram)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == "first_pixel + count leaves the film", (first, count)
    assert counters(r) == before
    torch.cuda.synchronize()
    assert bool((film.view(torch.uint8) == 0x5A).all()) and bool((histogram.view(torch.uint8) == 0x5A).all())


# ---- 2. the array path: the normalising helpers' refusals, as reached through the wrappers -------------------------------------------------
def Z(shape, dtype):
    return np.zeros(shape, dtype=dtype)


RES, RAYS, RNG = Z((N, 4), "f4"), Z((N, 8), "f4"), Z((N, 6), "u4")
FILM32, FILM64, MOM1, MOM4, FEAT = Z((P, 4), "u4"), Z((P, 4), "u8"), Z(P, "u8"), Z((P, 4), "u8"), Z((P, 8), "f4")
FEAT_HI = Z((P * FACTOR ** 2, 8), "f4")
ROWS_F32, ROWS_U32, ROWS_U64 = "(N,) records or (N, 4) float32", "(N,) records or (N, 4) uint32", "(N,) records or (N, 4) uint64"
LEAVES, WH = "first_pixel + count leaves the film", "film: width * height entries"
PER_PIXEL = " one FEATURE_DTYPE row (or 8 float32) per pixel of its film"
ARRAY_REFUSALS = [
    ("intersect", lambda r: r.intersect(Z((N, 7), "f4")), "rays: (N, 8) float32 or (N,) RAY_DTYPE"),
    ("occluded", lambda r: r.occluded(Z(N, "f4")), "rays: (N, 8) float32 or (N,) RAY_DTYPE"),
    ("trace_paths rays", lambda r: r.trace_paths(Z((N, 7), "f4"), RNG, 2), "rays: (N, 8) float32 or (N,) RAY_DTYPE"),
    ("trace_paths rng", lambda r: r.trace_paths(RAYS, Z((N - 1, 6), "u4"), 2), "rng: (N,) PATH_RNG_DTYPE or (N, 6) uint32, one state per ray"),
    ("generate_rays rng", lambda r: r.generate_rays(FILM, Z((N, 5), "u4")), "rng: (N,) PATH_RNG_DTYPE or (N, 6) uint32"),
    ("generate_rays index", lambda r: r.generate_rays(FILM, RNG, index=Z(N - 1, "u4")), "index: one film pixel per ray"),
    ("generate_rays rays", lambda r: r.generate_rays(FILM, RNG, rays=Z((N - 1, 8), "f4")), "rays: one row per stream"),
    ("generate_rays rays columns", lambda r: r.generate_rays(FILM, RNG, rays=Z((N, 7), "f4")), "rays: (N,) records or (N, 8) float32"),
    ("generate_rays positions index", lambda r: r.generate_rays(FILM, RNG, index=Z(N + 1, "u4"), positions=True), "index: one film pixel per ray"),
    ("accumulate_paths results", lambda r: r.accumulate_paths(Z((N, 3), "f4"), FILM32), "results: " + ROWS_F32),
    ("accumulate_paths index", lambda r: r.accumulate_paths(RES, FILM32, index=Z(N + 1, "u4")), "index: one film pixel per ray"),
    ("accumulate_paths film", lambda r: r.accumulate_paths(RES, Z((P, 3), "u4")), "film: " + ROWS_U32),
    ("accumulate_paths pixels", lambda r: r.accumulate_paths(RES, FILM32, pixels=Z((P - 1, 4), "u1")), "pixels and history: one entry per film pixel"),
    ("accumulate_paths history", lambda r: r.accumulate_paths(RES, FILM32, history=Z((P, 3), "f4")), "history: " + ROWS_F32),
    ("accumulate_paths_stats moments", lambda r: r.accumulate_paths_stats(RES, FILM32, Z(P - 1, "u8")), "moments: one uint64 per film pixel"),
    ("accumulate_paths_stats history", lambda r: r.accumulate_paths_stats(RES, FILM32, MOM1, history=Z((P + 1, 4), "f4")),
     "pixels and history: one entry per film pixel"),
    ("accumulate_paths_linear results", lambda r: r.accumulate_paths_linear(Z((N, 5), "f4"), FILM64), "results: " + ROWS_F32),
    ("accumulate_paths_linear film", lambda r: r.accumulate_paths_linear(RES, Z((P, 3), "u8")), "film: " + ROWS_U64),
    ("accumulate_paths_linear index", lambda r: r.accumulate_paths_linear(RES, FILM64, index=Z(1, "u4")), "index: one film pixel per ray"),
    ("accumulate_paths_linear_stats film", lambda r: r.accumulate_paths_linear_stats(RES, Z((P - 1, 4), "u8"), MOM4), "moments: one row per film pixel"),
    ("accumulate_paths_linear_stats moments", lambda r: r.accumulate_paths_linear_stats(RES, FILM64, Z((P, 3), "u8")), "moments: " + ROWS_U64),
    ("accumulate_paths_linear_stats index", lambda r: r.accumulate_paths_linear_stats(RES, None, MOM4, index=Z(N - 1, "u4")), "index: one film pixel per ray"),
    ("ray_features", lambda r: r.ray_features(Z((N, 7), "f4")), "rays: (N,) records or (N, 8) float32"),
    ("plan_samples film", lambda r: r.plan_samples(Z((P, 5), "u4"), MOM1, N), "film: " + ROWS_U32),
    ("plan_samples moments", lambda r: r.plan_samples(FILM32, Z(P + 1, "u8"), N), "moments: one uint64 per film pixel"),
    ("plan_samples_linear moments", lambda r: r.plan_samples_linear(Z((P, 3), "u8"), N), "moments: " + ROWS_U64),
    ("resolve_linear first", lambda r: r.resolve_linear(FILM64, 1, P), LEAVES),
    ("resolve_linear count", lambda r: r.resolve_linear(FILM64, 0, -1), LEAVES),
    ("resolve_splat first", lambda r: r.resolve_splat(FILM64, P + 1), LEAVES),
    ("resolve_linear film", lambda r: r.resolve_linear(Z((P, 3), "u8")), "film: " + ROWS_U64),
    ("resolve_linear linear", lambda r: r.resolve_linear(FILM64, linear=Z((P - 1, 4), "f4")), "linear, pixels and history: one entry per film pixel"),
    ("resolve_splat pixels", lambda r: r.resolve_splat(FILM64, pixels=Z((P + 1, 4), "u1")), "linear, pixels and history: one entry per film pixel"),
    ("resolve_linear metered", lambda r: r.resolve_linear(FILM64, metered=Z(2, METER_STATE_DTYPE)), "state: one METER_STATE_DTYPE record"),
    ("resolve_linear glare film", lambda r: r.resolve_linear(FILM64, glare=(W + 1, H, GLARE, Z((64, 4), "u8"))), WH),
    ("resolve_linear glare pyramid", lambda r: r.resolve_linear(FILM64, glare=(W, H, GLARE, Z((PYRAMID - 1, 4), "u8"))),
     "pyramid: the entries glare_layout counts"),
    ("resolve_splat tone table", lambda r: r.resolve_splat(FILM64, tone=(TONE, Z(259, "f4"))), "table: tone_table_floats(bits) float32"),
    ("splat_paths positions", lambda r: r.splat_paths(RES, Z((N - 1, 2), "f4"), FILM64, W, H),
     "positions: one (x, y) per result, (N,) POSITION_DTYPE or (N, 2) float32"),
    ("splat_paths film", lambda r: r.splat_paths(RES, Z((N, 2), "f4"), FILM64, W + 1, H), WH),
    ("splat_paths_homed film", lambda r: r.splat_paths(RES, Z((N, 2), "f4"), Z((P - 1, 4), "u8"), W, H, homed_first_pixel=0), WH),
    ("glare_build film", lambda r: r.glare_build(Z((P - 1, 4), "u8"), W, H, glare=GLARE), WH),
    ("denoise_linear film", lambda r: r.denoise_linear(Z((P + 1, 4), "u8"), W, H, MOM4, FEAT), WH),
    ("denoise_linear features", lambda r: r.denoise_linear(FILM64, W, H, MOM4, Z((P, 7), "f4")), "features: (N,) FEATURE_DTYPE or (N, 8) float32"),
    ("denoise_linear moments", lambda r: r.denoise_linear(FILM64, W, H, Z((P - 1, 4), "u8"), FEAT), "moments, features: one row per film pixel"),
    ("denoise_linear features rows", lambda r: r.denoise_linear(FILM64, W, H, MOM4, Z((P + 1, 8), "f4")), "moments, features: one row per film pixel"),
    ("reproject_linear size", lambda r: r.reproject_linear(ptss.film_camera("pinhole", 0, H), FEAT, FILM, FEAT, FILM64),
     "the films' width and height must be positive"),
    ("reproject_linear film_prev", lambda r: r.reproject_linear(FILM, FEAT, FILM, FEAT, Z((P - 1, 4), "u8")), WH),
    ("reproject_linear features_now", lambda r: r.reproject_linear(FILM, Z((P - 1, 8), "f4"), FILM, FEAT, FILM64), "features_now:" + PER_PIXEL),
    ("reproject_linear features_prev", lambda r: r.reproject_linear(FILM, FEAT, FILM, Z((P, 7), "f4"), FILM64), "features_prev:" + PER_PIXEL),
    ("reproject_linear motion_now", lambda r: r.reproject_linear(FILM, FEAT, FILM, FEAT, FILM64, motion_now=Z(P - 1, ptss.MOTION_DTYPE)),
     "motion_now: one row per pixel of the new film"),
    ("reproject_linear moments_prev", lambda r: r.reproject_linear(FILM, FEAT, FILM, FEAT, FILM64, Z((P + 1, 4), "u8")),
     "moments_prev: one row per pixel of the previous film"),
    ("upsample_linear size", lambda r: r.upsample_linear(FILM64, 0, H, FEAT, FEAT_HI, upsample=UPSAMPLE), "width and height must be positive"),
    ("upsample_linear film_lo", lambda r: r.upsample_linear(Z((P - 1, 4), "u8"), W, H, FEAT, FEAT_HI, upsample=UPSAMPLE), WH),
    ("upsample_linear features_lo", lambda r: r.upsample_linear(FILM64, W, H, Z((P + 1, 8), "f4"), FEAT_HI, upsample=UPSAMPLE), "features_lo:" + PER_PIXEL),
    ("upsample_linear features_hi", lambda r: r.upsample_linear(FILM64, W, H, FEAT, FEAT, upsample=UPSAMPLE), "features_hi:" + PER_PIXEL),
    ("meter_linear first", lambda r: r.meter_linear(FILM64, 1, P), LEAVES),
    ("meter_splat count", lambda r: r.meter_splat(FILM64, 0, P + 1), LEAVES),
    ("meter_linear film", lambda r: r.meter_linear(Z((P, 5), "u8")), "film: " + ROWS_U64),
    ("meter_linear histogram", lambda r: r.meter_linear(FILM64, histogram=Z(METER_BINS - 1, "u4")), "histogram: METER_BINS uint32 counts"),
    ("meter_exposure histogram", lambda r: r.meter_exposure(Z(METER_BINS + 1, "u4")), "histogram: METER_BINS uint32 counts"),
    ("meter_exposure state", lambda r: r.meter_exposure(Z(METER_BINS, "u4"), Z(2, METER_STATE_DTYPE)), "state: one METER_STATE_DTYPE record"),
]


def test_array_refusals_keep_their_text_and_move_no_counter(gpu):
    _, r, _ = gpu
    before = counters(r)
    for what, call, text in ARRAY_REFUSALS:
        with pytest.raises(ValueError) as e:
            call(r)
        assert str(e.value) == text, what
    assert counters(r) == before
    for a in (RES, RAYS, RNG, FILM32, FILM64, MOM1, MOM4, FEAT, FEAT_HI):
        assert not a.any()


# ---- 3. zero-size calls --------------------------------------------------------------------------------------------------------------------
NO_RES, NO_RAYS, NO_RNG = Z((0, 4), "f4"), Z((0, 8), "f4"), Z((0, 6), "u4")
HISTORY_ROWS = (ptss.HISTORY_DTYPE, (P,))
# wrapper -> (the call, the (dtype, shape) of every array it returns; None for None)
ZERO_CALLS = {
    "intersect": (lambda r: r.intersect(NO_RAYS), [(ptss.HIT_DTYPE, (0,))]),
    "occluded": (lambda r: r.occluded(NO_RAYS), [(np.uint32, (0,))]),
    "seed_path_rng": (lambda r: r.seed_path_rng(0, 7), [(PATH_RNG_DTYPE, (0,))]),
    "trace_paths": (lambda r: r.trace_paths(NO_RAYS, NO_RNG, 2), [(PATH_RESULT_DTYPE, (0,)), (PATH_RNG_DTYPE, (0,))]),
    "trace_paths_refill": (lambda r: r.trace_paths(NO_RAYS, NO_RNG, 2, schedule="refill"), [(PATH_RESULT_DTYPE, (0,)), (PATH_RNG_DTYPE, (0,))]),
    "generate_rays": (lambda r: r.generate_rays(FILM, NO_RNG), [(ptss.RAY_DTYPE, (0,)), (PATH_RNG_DTYPE, (0,))]),
    "generate_rays_positions": (lambda r: r.generate_rays(FILM, NO_RNG, positions=True),
                                [(ptss.RAY_DTYPE, (0,)), (PATH_RNG_DTYPE, (0,)), (POSITION_DTYPE, (0,))]),
    "accumulate_paths": (lambda r: r.accumulate_paths(NO_RES, FILM32, pixels=True), [(FILM_DTYPE, (P,)), (np.uint8, (P, 4)), None]),
    "accumulate_paths_stats": (lambda r: r.accumulate_paths_stats(NO_RES, FILM32, MOM1, history=True),
                               [(FILM_DTYPE, (P,)), (np.uint64, (P,)), None, HISTORY_ROWS]),
    "accumulate_paths_linear": (lambda r: r.accumulate_paths_linear(NO_RES, FILM64), [(LINEAR_DTYPE, (P,))]),
    "accumulate_paths_linear_stats": (lambda r: r.accumulate_paths_linear_stats(NO_RES, FILM64, MOM4), [(LINEAR_DTYPE, (P,)), (MOMENT_DTYPE, (P,))]),
    "ray_features": (lambda r: r.ray_features(NO_RAYS), [(ptss.FEATURE_DTYPE, (0,))]),
    "plan_samples": (lambda r: r.plan_samples(FILM32, MOM1, 0)[:2], [(np.uint64, (P,)), (np.uint32, (0,))]),
    "plan_samples_linear": (lambda r: r.plan_samples_linear(MOM4, 0)[:2], [(np.uint64, (P,)), (np.uint32, (0,))]),
    "resolve_linear": (lambda r: r.resolve_linear(FILM64, 3, 0), [HISTORY_ROWS, (np.uint8, (P, 4)), HISTORY_ROWS]),
    "resolve_splat": (lambda r: r.resolve_splat(FILM64, P, None, history=None), [HISTORY_ROWS, (np.uint8, (P, 4)), None]),
    "splat_paths": (lambda r: r.splat_paths(NO_RES, Z((0, 2), "f4"), FILM64, W, H), [(SPLAT_DTYPE, (P,))]),
    "splat_paths_homed": (lambda r: r.splat_paths(NO_RES, Z((0, 2), "f4"), FILM64, W, H, homed_first_pixel=2), [(SPLAT_DTYPE, (P,))]),
    "meter_linear": (lambda r: r.meter_linear(FILM64, 0, 0), [(np.uint32, (METER_BINS,))]),
    "meter_splat": (lambda r: r.meter_splat(FILM64, P, 0), [(np.uint32, (METER_BINS,))]),
}
RETURNS_EARLY = ("intersect", "occluded")   # every other wrapper reaches the library with null pointers and n == 0


def layout_of(result):
    results = result if isinstance(result, tuple) else (result,)
    return [None if a is None else (a.dtype, a.shape) for a in results]


@pytest.mark.parametrize("wrapper", sorted(ZERO_CALLS))
def test_a_zero_size_call_does_what_it_did(gpu, wrapper):
    _, r, gone = gpu
    call, want = ZERO_CALLS[wrapper]
    before = counters(r)
    assert layout_of(call(r)) == [None if w is None else (np.dtype(w[0]), w[1]) for w in want]
    assert counters(r) == before
    if wrapper in RETURNS_EARLY:
        assert layout_of(call(gone)) == layout_of(call(r))
    else:
        with pytest.raises(ptss.PtssError, match="ptss error -1"):
            call(gone)
