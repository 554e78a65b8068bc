"""ptss.py — thin ctypes binding of the two product libraries for the Python harness
(tests/, bench.py, __graft_entry__.py).

  libptss_host.so  include/ptss_host.h  host mirror (Scene presets, camera, TGA, tile rows, probes)
  libptss.so       include/ptss.h       the HIP hot path (no CPU fallback: create() raises without a GPU)

PyTorch is used by callers only for device memory / streams / torch.distributed; nothing here
imports torch.
"""
import ctypes as C
import os
import sys

import numpy as np

from ptss_types import (FILM_DTYPE, FILM_EQUIRECT, FILM_PINHOLE, FILM_THIN_LENS, KERNEL_BITS, LINEAR_DTYPE, LinearEntry, LinearParams, PATH_RESULT_DTYPE, PATH_RNG_DTYPE, PATHS_LANE_PER_RAY, PATHS_REFILL,
                        PathOptions, PlanInfo, PlanParams, SCENE_LAYOUT_FIELDS,
                        SCENE_LAYOUT_MESH_FIELDS, AreaLight, Camera, DenoiseParams, FilmCamera, FilmEntry, HistoryEntry, Material, PixelFeature, PixelMotion, PointLight, RayHit, RayQuery, ReprojectParams, SceneDesc, Sphere, Triangle,
                        UChar4, UpsampleParams, Vec3, struct_to_dict)
from ptss_types import POSITION_DTYPE, SPLAT_BOX, SPLAT_DTYPE, SPLAT_GAUSSIAN, SPLAT_TENT, FilmPosition, SplatEntry, SplatFilter
from ptss_types import METER_BINS, METER_BLOCK, METER_GRID_CAP, METER_STATE_DTYPE, MeterParams, MeterState
from ptss_types import MOMENT_DTYPE, LinearMoment, LinearPlanParams
from ptss_types import (GLARE_ADD, GLARE_DTYPE, GLARE_FILM_LINEAR, GLARE_FILM_SPLAT, GLARE_MAX_LEVELS, GLARE_MIX, GLARE_TAIL_ENTRIES, GLARE_TILE, GlareLevel,
                        GlareParams)
from ptss_types import DENOISE_LINEAR_EMPTY, DENOISE_LINEAR_WORKSPACE_BYTES, DENOISE_MAX_LEVELS, FILM_LINEAR, FILM_SPLAT, DenoiseLinearParams
from ptss_types import REPROJECT_LINEAR_INFO_DTYPE, REPROJECT_LINEAR_MAX_HISTORY, ReprojectLinearParams
from ptss_types import UPSAMPLE_LINEAR_INFO_DTYPE, UPSAMPLE_LINEAR_WRAP_X, UpsampleLinearParams
from ptss_types import SPHERE_DTYPE, SURFACE_BACK, SURFACE_COSINE, SURFACE_NORMAL, SURFACE_POINT_DTYPE, SURFACE_TRIANGLE, SurfaceParams
from ptss_types import (LIGHTMAP_BILINEAR, LIGHTMAP_EMISSION, LIGHTMAP_MODULATE, LIGHTMAP_NEAREST, MATERIAL_DTYPE, SURFACE_BLOCK_DTYPE,
                        LightmapParams)
from ptss_types import CHAIN_DTYPE, CHAIN_LANE_PER_RAY, CHAIN_REFILL, ChainOptions
from ptss_types import TONE_CLAMP, TONE_FILMIC, TONE_LUMINANCE, TONE_REINHARD, TRANSFER_GAMMA22, TRANSFER_SRGB, ToneParams

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(_HERE, "lib")
HOST_LIB = os.path.join(LIBDIR, "libptss_host.so")
DEVICE_LIB = os.path.join(LIBDIR, os.environ.get("PTSS_LIBNAME", "libptss.so"))  # PTSS_LIBNAME: A/B variants

_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)


class PtssError(RuntimeError):
    pass


class RenderConfig(C.Structure):
    _fields_ = [("structSize", C.c_uint), ("width", C.c_int), ("height", C.c_int), ("seed", C.c_ulonglong), ("maxIterations", C.c_uint),
                ("device", C.c_int), ("tileRank", C.c_int), ("tileWorld", C.c_int), ("bandRows", C.c_int),
                ("syncEachFrame", C.c_int), ("floatAccumulator", C.c_int), ("timeKernels", C.c_int),
                ("samplesPerPass", C.c_int), ("everySphereLoop", C.c_int), ("frameLanes", C.c_int),
                ("lanesFreeRun", C.c_int), ("oneLaunchFrames", C.c_int)]


# scene variants of the bounce / frame kernels, in the order of their bit in ptss_launched_kernels (include/ptss_types.h)
KERNEL_VARIANTS = ("accel", "bounded+pairs", "bounded", "plain")


def _bounce(variant, j):   # a bounce kernel's place in its variant's eight: last * 4 + inLds * 2 + first
    return ("bounce", variant, bool(j & 4), bool(j & 2), bool(j & 1))


# the instantiation behind offset j of each range of ptss_types.KERNEL_BITS
_KERNEL_NAMES = {
    "BOUNCE": lambda j: _bounce(KERNEL_VARIANTS[j // 8], j % 8),
    "FRAME": lambda j: ("frame", KERNEL_VARIANTS[j]),
    "BOUNCE_MESH": lambda j: _bounce("mesh", j),
    "QUERY": lambda j: ("query", "any" if j & 2 else "closest", bool(j & 1)),
    "FEATURES": lambda j: ("features", bool(j)),
    "DENOISE": lambda j: ("denoise",),
    "UPDATE": lambda j: ("update",),
    "REFIT": lambda j: ("refit",),
    "REPROJECT": lambda j: ("reproject",),
    "FEATURES_MOTION": lambda j: ("features_motion", bool(j)),
    "REPROJECT_MOTION": lambda j: ("reproject_motion",),
}
# bit of ptss_launched_kernels -> the name launched_kernels() reports for it
KERNEL_OF_BIT = {base + j: _KERNEL_NAMES[rng](j) for rng, (base, width) in KERNEL_BITS.items() for j in range(width)}


def _kernels_of(*ranges):
    return {KERNEL_OF_BIT[KERNEL_BITS[r][0] + j] for r in ranges for j in range(KERNEL_BITS[r][1])}


def decode_launched_kernels(mask):
    """The names of the bits set in a ptss_launched_kernels mask; a bit no kernel owns names nothing."""
    return {name for bit, name in KERNEL_OF_BIT.items() if mask >> bit & 1}


def all_kernels():
    """Every instantiation ptss_launched_kernels can report: ("bounce", variant, last, inLds, first) and ("frame", variant)."""
    return _kernels_of("BOUNCE", "FRAME")


def mesh_kernels():
    """The bounce-kernel instantiations of the mesh image (no frame kernel): ("bounce", "mesh", last, inLds, first)."""
    return _kernels_of("BOUNCE_MESH")


def query_kernels():
    """The query-kernel instantiations (ptss_intersect / ptss_occluded): ("query", "closest" | "any", inLds)."""
    return _kernels_of("QUERY")


def feature_kernels():
    """The feature-kernel instantiations (ptss_render_features): ("features", inLds)."""
    return _kernels_of("FEATURES")


def reproject_kernels():
    """The reprojection kernel (ptss_reproject): ("reproject",)."""
    return _kernels_of("REPROJECT")


def motion_kernels():
    """The kernels of the motion path (ptss_render_features_motion / ptss_reproject_motion): ("features_motion", inLds) and
    ("reproject_motion",)."""
    return _kernels_of("FEATURES_MOTION", "REPROJECT_MOTION")


_host = None
_dev = None
_hip = None


def _hip_lib():
    """The HIP runtime libptss.so links (device buffers of the numpy query path)."""
    global _hip
    if _hip is None:
        device_lib()
        L = C.CDLL("libamdhip64.so.7", mode=C.RTLD_GLOBAL)   # by soname: the runtime already loaded for libptss.so
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipSetDevice.argtypes = [C.c_int]
        L.hipDeviceSynchronize.argtypes = []
        _hip = L
    return _hip


def _hip_check(rc, what):
    if rc != 0:
        raise PtssError(f"{what} failed (hipError {rc})")


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise PtssError(f"{HOST_LIB} missing: run `python __graft_entry__.py build` first")
        L = C.CDLL(HOST_LIB)
        L.ptss_scene_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.ptss_scene_destroy.argtypes = [C.c_void_p]
        L.ptss_scene_destroy.restype = None
        L.ptss_scene_describe.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
        L.ptss_camera_default.argtypes = [C.POINTER(Camera)]
        L.ptss_camera_move.argtypes = [C.POINTER(Camera), C.c_ubyte, C.POINTER(C.c_int)]
        L.ptss_write_tga.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
        L.ptss_tile_rows.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.ptss_probe_math.argtypes = [C.c_int, _f32p, _f32p, _f32p, C.c_size_t]
        L.ptss_probe_vector.argtypes = [C.c_int, _f32p, _f32p, C.c_size_t]
        L.ptss_probe_quantize.argtypes = [_f32p, C.POINTER(C.c_uint), C.c_size_t]
        L.ptss_probe_guard.argtypes = [C.c_int, _f32p, C.POINTER(C.c_uint), C.c_size_t]
        L.ptss_probe_guard_constants.argtypes = [_f32p]
        L.ptss_probe_scene_guard_flags.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_uint)]
        L.ptss_probe_triangle_forms.argtypes = [_f32p, _f32p, _f32p, _f32p, C.c_int, C.c_size_t, C.POINTER(C.c_int), _f32p, _f32p]
        L.ptss_probe_quant_table.argtypes = [_f32p]
        L.ptss_probe_wave_locate.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int)]
        L.ptss_probe_rng_init.argtypes = [C.c_ulonglong, C.c_uint, _u32p]
        L.ptss_scene_add_obj.argtypes = [C.c_void_p, C.c_char_p, _f32p, C.c_int, C.POINTER(C.c_size_t)]
        L.ptss_probe_mesh_bound.argtypes = [_f32p, C.c_size_t, _f32p, _f32p, C.c_size_t, C.c_float, C.POINTER(C.c_int), _f32p]
        L.ptss_probe_rng_draw.argtypes = [_u32p, _u32p, _f32p, C.c_size_t]
        L.ptss_probe_rng_jump_table.argtypes = [_u32p, C.c_size_t]
        L.ptss_camera_ray.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(RayQuery)]
        L.ptss_probe_mesh_refit.argtypes = [_f32p, C.c_size_t, _f32p]
        L.ptss_probe_mesh_touch.argtypes = [_f32p, _f32p, _f32p, C.c_size_t, C.c_float, C.POINTER(C.c_int)]
        L.ptss_probe_kd_order.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.ptss_probe_kd_order_signed_zero.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.ptss_probe_pack_scene.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p,
                                            C.c_size_t, _f32p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.ptss_probe_denoise.argtypes = [_u32p, C.c_float, C.c_void_p, C.c_int, C.c_int, C.POINTER(DenoiseParams), C.c_void_p, _f32p]
        L.ptss_probe_denoise_history.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(DenoiseParams), C.c_void_p, _f32p]
        L.ptss_probe_reproject.argtypes = [_u32p, C.c_float, C.c_int, C.POINTER(Camera), C.POINTER(Camera), C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.POINTER(ReprojectParams), C.c_void_p]
        L.ptss_probe_reproject_motion.argtypes = [_u32p, C.c_float, C.c_int, C.POINTER(Camera), C.POINTER(Camera), C.c_int, C.c_int, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ReprojectParams), C.c_void_p]
        L.ptss_probe_upsample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(UpsampleParams), C.c_void_p, _f32p]
        L.ptss_probe_upsample_axis.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _f32p]
        L.ptss_probe_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]
        L.ptss_probe_specular_step.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int)]
        L.ptss_probe_specular_class.argtypes = [C.c_void_p]
        L.ptss_probe_specular_link.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]
        L.ptss_probe_lookup_lightmap_chain.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(LightmapParams), C.POINTER(LinearParams), C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ptss_probe_strip_masks.argtypes = [C.POINTER(SceneDesc), C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                             C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_void_p]
        L.ptss_probe_film_rays.argtypes = [C.POINTER(FilmCamera), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.ptss_probe_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_ulonglong)]
        L.ptss_probe_accumulate_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                  C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.ptss_probe_plan_samples.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(PlanParams), C.c_size_t, C.c_void_p, C.c_void_p,
                                              C.POINTER(PlanInfo)]
        L.ptss_probe_plan_weight.argtypes = [C.POINTER(FilmEntry), C.c_ulonglong, C.POINTER(PlanParams)]
        L.ptss_probe_plan_weight.restype = C.c_uint32
        L.ptss_probe_plan_target.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_ulonglong]
        L.ptss_probe_plan_target.restype = C.c_ulonglong
        L.ptss_probe_accumulate_linear.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(LinearParams),
                                                   C.POINTER(C.c_ulonglong)]
        L.ptss_probe_accumulate_linear_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                                         C.POINTER(LinearParams), C.POINTER(C.c_ulonglong)]
        L.ptss_probe_plan_samples_linear.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(LinearParams), C.POINTER(LinearPlanParams), C.c_size_t,
                                                     C.c_void_p, C.c_void_p, C.POINTER(PlanInfo)]
        L.ptss_probe_linear_plan_weight.argtypes = [C.POINTER(LinearMoment), C.POINTER(LinearParams), C.POINTER(LinearPlanParams)]
        L.ptss_probe_linear_plan_weight.restype = C.c_uint32
        L.ptss_probe_resolve_linear.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptss_probe_film_positions.argtypes = [C.POINTER(FilmCamera), C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_ulonglong)]
        L.ptss_probe_splat_paths.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_size_t, C.c_void_p, C.c_int, C.c_int,
                                             C.POINTER(SplatFilter), C.POINTER(LinearParams), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        L.ptss_probe_resolve_splat.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptss_probe_meter_bin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
        L.ptss_probe_meter_linear.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        L.ptss_probe_meter_splat.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
        L.ptss_probe_meter_exposure.argtypes = [C.c_void_p, C.POINTER(LinearParams), C.POINTER(MeterParams), C.c_void_p]
        L.ptss_glare_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(GlareLevel), C.POINTER(C.c_size_t)]
        L.ptss_probe_glare_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(LinearParams), C.POINTER(GlareParams), C.c_void_p]
        L.ptss_probe_resolve_glare.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), C.c_int, C.c_int,
                                               C.POINTER(GlareParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptss_probe_tone_build.argtypes = [C.POINTER(ToneParams), C.c_void_p]
        L.ptss_probe_tone_value.argtypes = [C.POINTER(ToneParams), C.c_void_p, C.c_void_p, C.c_size_t]
        L.ptss_probe_tone_level.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.ptss_probe_resolve_toned.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), C.POINTER(ToneParams), C.c_void_p,
                                               C.c_void_p, C.c_int, C.c_int, C.POINTER(GlareParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ptss_probe_denoise_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(LinearParams),
                                                C.POINTER(DenoiseLinearParams), C.c_void_p, C.c_void_p]
        L.ptss_probe_denoise_linear_finish.argtypes = [C.POINTER(C.c_float), C.c_ulonglong, C.c_int, C.POINTER(LinearParams), C.POINTER(C.c_ulonglong)]
        L.ptss_probe_reproject_linear.argtypes = [C.POINTER(FilmCamera), C.c_void_p, C.c_void_p, C.POINTER(FilmCamera), C.c_void_p, C.c_void_p, C.c_int,
                                                  C.c_void_p, C.POINTER(LinearParams), C.POINTER(ReprojectLinearParams), C.c_void_p, C.c_void_p,
                                                  C.c_void_p]
        L.ptss_probe_reproject_linear_finish.argtypes = [C.POINTER(C.c_float), C.c_float, C.c_int, C.c_float, C.c_int, C.POINTER(LinearParams),
                                                         C.POINTER(ReprojectLinearParams), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        L.ptss_probe_upsample_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(LinearParams),
                                                 C.POINTER(UpsampleLinearParams), C.c_void_p, C.c_void_p]
        L.ptss_probe_surface_rays.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(SurfaceParams), C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_ulonglong)]
        L.ptss_probe_dilate_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.ptss_surface_atlas.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
        L.ptss_surface_atlas_blocks.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int),
                                                C.POINTER(C.c_size_t)]
        L.ptss_probe_lookup_lightmap.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(LightmapParams), C.POINTER(LinearParams), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        _host = L
    return _host


def _torch():
    """torch where the caller has imported it, None otherwise: the one place that looks for it (nothing here imports it)."""
    return sys.modules.get("torch")


def _is_torch(value):
    """Whether `value` is a torch object: what sends a Renderer call down its tensor path."""
    return type(value).__module__.split(".")[0] == "torch"


def _stream_of(torch, device):
    """The raw handle of torch's current stream on `device`."""
    return torch.cuda.current_stream(device).cuda_stream


def _torch_first():
    """PyTorch bundles its own HIP runtime and libptss.so links ROCm's; both may share a process, but torch's must initialise
    first or a later torch.cuda call can fail with "No HIP GPUs are available" (INTEGRATION.md §5). If torch is already
    imported, initialise it now — before libptss.so's runtime touches the device."""
    torch = _torch()
    if torch is None:
        return
    try:
        if torch.cuda.is_available() and not torch.cuda.is_initialized():
            torch.cuda.init()
    except Exception as e:  # pragma: no cover - depends on the box
        raise PtssError("torch is imported but torch.cuda could not be initialised before libptss.so's HIP runtime "
                        f"(INTEGRATION.md §5, two HIP runtimes in one process): {e}")


def device_lib():
    """Loads libptss.so. Loading needs no GPU; ptss_create does."""
    global _dev
    _torch_first()
    if _dev is None:
        if not os.path.exists(DEVICE_LIB):
            raise PtssError(f"{DEVICE_LIB} missing: the HIP extension was not built (no CPU fallback exists)")
        L = C.CDLL(DEVICE_LIB)
        vp = C.c_void_p
        L.ptss_default_config.argtypes = [C.POINTER(RenderConfig)]
        L.ptss_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(RenderConfig), C.POINTER(vp)]
        L.ptss_destroy.argtypes = [vp]
        L.ptss_generate_frame.argtypes = [vp, vp, C.c_int]
        L.ptss_set_camera.argtypes = [vp, C.POINTER(Camera)]
        L.ptss_get_camera.argtypes = [vp, C.POINTER(Camera)]
        L.ptss_request_reset.argtypes = [vp]
        L.ptss_set_mode.argtypes = [vp, C.c_int]
        L.ptss_set_max_iterations.argtypes = [vp, C.c_uint]
        L.ptss_set_stream.argtypes = [vp, vp]
        L.ptss_bind_accumulator.argtypes = [vp, vp]
        L.ptss_accumulator_devptr.argtypes = [vp, C.POINTER(vp)]
        L.ptss_float_accumulator_devptr.argtypes = [vp, C.POINTER(vp)]
        L.ptss_alloc_pixels.argtypes = [vp, C.POINTER(vp)]
        L.ptss_free_pixels.argtypes = [vp, vp]
        L.ptss_local_pixels.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.ptss_local_rows.argtypes = [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
        L.ptss_read_accumulator.argtypes = [vp, _u32p, C.c_size_t]
        L.ptss_read_float_accumulator.argtypes = [vp, _f32p, C.c_size_t]
        L.ptss_read_pixels.argtypes = [vp, vp, vp, C.c_size_t]
        L.ptss_read_rng_state.argtypes = [vp, C.c_size_t, _u32p]
        L.ptss_read_rng_state_lane.argtypes = [vp, C.c_size_t, C.c_uint, _u32p]
        L.ptss_synchronize.argtypes = [vp]
        L.ptss_last_pass_ms.argtypes = [vp, _f32p]
        L.ptss_samples_since_reset.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptss_live_counts.argtypes = [vp, _u32p, C.c_int, C.POINTER(C.c_int)]
        L.ptss_total_ray_bounces.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_frame_lanes.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptss_one_launch_frames.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptss_guard_timeouts.argtypes = [vp, C.POINTER(C.c_uint)]
        L.ptss_bounce_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)]
        L.ptss_launched_kernels.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_guard_flags.argtypes = [vp, C.POINTER(C.c_uint)]
        L.ptss_debug_counters.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_triangle_leaves.argtypes = [vp, C.POINTER(C.c_int)]
        L.ptss_intersect.argtypes = [vp, vp, vp, C.c_size_t, vp]
        L.ptss_occluded.argtypes = [vp, vp, vp, C.c_size_t, vp]
        L.ptss_render_features.argtypes = [vp, vp, vp]
        L.ptss_default_denoise_params.argtypes = [C.POINTER(DenoiseParams)]
        L.ptss_denoise.argtypes = [vp, vp, C.POINTER(DenoiseParams), vp, vp]
        L.ptss_read_denoise_plane.argtypes = [vp, _f32p, C.c_size_t, C.POINTER(C.c_int)]
        L.ptss_default_reproject_params.argtypes = [C.POINTER(ReprojectParams)]
        L.ptss_reproject.argtypes = [vp, vp, C.POINTER(Camera), vp, vp, C.POINTER(ReprojectParams), vp, vp]
        L.ptss_denoise_history.argtypes = [vp, vp, vp, C.POINTER(DenoiseParams), vp, vp]
        L.ptss_render_features_motion.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp, vp]
        L.ptss_reproject_motion.argtypes = [vp, vp, vp, C.POINTER(Camera), vp, vp, C.POINTER(ReprojectParams), vp, vp]
        L.ptss_render_features_specular.argtypes = [vp, C.c_int, vp, vp, vp]
        L.ptss_specular_feature_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_seed_path_rng.argtypes = [vp, vp, C.c_size_t, C.c_ulonglong, C.c_ulonglong, C.c_uint, vp]
        L.ptss_trace_paths.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint, vp]
        L.ptss_path_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_path_options.argtypes = [C.POINTER(PathOptions)]
        L.ptss_trace_paths_opt.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint, C.POINTER(PathOptions), vp]
        L.ptss_path_refill_stats.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_generate_rays.argtypes = [vp, C.POINTER(FilmCamera), C.c_size_t, vp, C.c_size_t, vp, vp, vp]
        L.ptss_accumulate_paths.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp, vp, vp]
        L.ptss_ray_features.argtypes = [vp, vp, vp, C.c_size_t, vp]
        L.ptss_film_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_film_rejected.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_accumulate_paths_stats.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t, vp, vp, vp]
        L.ptss_default_plan_params.argtypes = [C.POINTER(PlanParams)]
        L.ptss_plan_cdf_entries.argtypes = [C.c_size_t, C.POINTER(C.c_size_t)]
        L.ptss_plan_samples.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(PlanParams), C.c_size_t, vp, vp, vp, vp]
        L.ptss_adaptive_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_linear_params.argtypes = [C.POINTER(LinearParams)]
        L.ptss_accumulate_paths_linear.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.POINTER(LinearParams), vp]
        L.ptss_resolve_linear.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), vp, vp, vp, vp]
        L.ptss_linear_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_linear_plan_params.argtypes = [C.POINTER(LinearPlanParams)]
        L.ptss_accumulate_paths_linear_stats.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(LinearParams), vp]
        L.ptss_plan_samples_linear.argtypes = [vp, vp, C.c_size_t, C.POINTER(LinearParams), C.POINTER(LinearPlanParams), C.c_size_t, vp, vp, vp, vp]
        L.ptss_linear_stats_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_splat_filter.argtypes = [C.POINTER(SplatFilter)]
        L.ptss_generate_rays_positions.argtypes = [vp, C.POINTER(FilmCamera), C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp]
        L.ptss_splat_paths.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_int, C.c_int, C.POINTER(SplatFilter), C.POINTER(LinearParams), vp]
        L.ptss_splat_paths_homed.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp, C.c_int, C.c_int, C.POINTER(SplatFilter),
                                             C.POINTER(LinearParams), vp]
        L.ptss_resolve_splat.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), vp, vp, vp, vp]
        L.ptss_splat_stats.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_meter_params.argtypes = [C.POINTER(MeterParams)]
        L.ptss_meter_linear.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp]
        L.ptss_meter_splat.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp, vp]
        L.ptss_meter_exposure.argtypes = [vp, vp, C.POINTER(LinearParams), C.POINTER(MeterParams), vp, vp]
        L.ptss_resolve_linear_metered.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), vp, vp, vp, vp, vp]
        L.ptss_resolve_splat_metered.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), vp, vp, vp, vp, vp]
        L.ptss_meter_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_glare_params.argtypes = [C.POINTER(GlareParams)]
        L.ptss_glare_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(GlareLevel), C.POINTER(C.c_size_t)]
        L.ptss_glare_build.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(LinearParams), C.POINTER(GlareParams), vp, vp]
        L.ptss_resolve_linear_glare.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), C.c_int, C.c_int, C.POINTER(GlareParams), vp, vp,
                                                vp, vp, vp, vp]
        L.ptss_resolve_splat_glare.argtypes = L.ptss_resolve_linear_glare.argtypes
        L.ptss_glare_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_tone_params.argtypes = [C.POINTER(ToneParams)]
        L.ptss_tone_table_floats.argtypes = [C.c_int]
        L.ptss_tone_table_floats.restype = C.c_size_t
        L.ptss_tone_build.argtypes = [vp, C.POINTER(ToneParams), vp, vp]
        L.ptss_resolve_toned.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(LinearParams), C.POINTER(ToneParams), vp, vp, C.c_int, C.c_int,
                                         C.POINTER(GlareParams), vp, vp, vp, vp, vp]
        L.ptss_tone_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_debug_tone_form.argtypes = [vp, C.c_int]
        L.ptss_default_denoise_linear_params.argtypes = [C.POINTER(DenoiseLinearParams)]
        L.ptss_denoise_linear_workspace.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.ptss_denoise_linear.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(LinearParams), C.POINTER(DenoiseLinearParams), vp, vp, vp]
        L.ptss_denoise_linear_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_debug_denoise_linear_form.argtypes = [vp, C.c_int]
        L.ptss_default_reproject_linear_params.argtypes = [C.POINTER(ReprojectLinearParams)]
        L.ptss_reproject_linear.argtypes = [vp, C.POINTER(FilmCamera), vp, vp, C.POINTER(FilmCamera), vp, vp, C.c_int, vp, C.POINTER(LinearParams),
                                            C.POINTER(ReprojectLinearParams), vp, vp, vp, vp]
        L.ptss_reproject_linear_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_default_upsample_linear_params.argtypes = [C.POINTER(UpsampleLinearParams)]
        L.ptss_upsample_linear.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(LinearParams), C.POINTER(UpsampleLinearParams), vp, vp, vp]
        L.ptss_upsample_linear_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_debug_upsample_linear_form.argtypes = [vp, C.c_int]
        L.ptss_generate_rays_surface.argtypes = [vp, C.POINTER(SurfaceParams), vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp]
        L.ptss_dilate_linear.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp]
        L.ptss_surface_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_surface_rejected.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_debug_dilate_linear_form.argtypes = [vp, C.c_int]
        L.ptss_default_lightmap_params.argtypes = [C.POINTER(LightmapParams)]
        L.ptss_lookup_lightmap.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(LinearParams), vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
        L.ptss_lightmap_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_debug_lightmap_form.argtypes = [vp, C.c_int]
        L.ptss_default_chain_options.argtypes = [C.POINTER(ChainOptions)]
        L.ptss_intersect_chain.argtypes = [vp, vp, C.c_size_t, C.c_int, C.POINTER(ChainOptions), vp, vp, vp]
        L.ptss_chain_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_lookup_lightmap_chain.argtypes = [vp, C.POINTER(LightmapParams), C.POINTER(LinearParams), vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
        L.ptss_lightmap_chain_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_render_features_scaled.argtypes = [vp, C.c_int, vp, vp]
        L.ptss_default_upsample_params.argtypes = [C.POINTER(UpsampleParams)]
        L.ptss_upsample.argtypes = [vp, vp, vp, vp, C.POINTER(UpsampleParams), vp, vp, vp]
        L.ptss_upsample_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_set_scene.argtypes = [vp, C.POINTER(SceneDesc)]
        L.ptss_update_triangles.argtypes = [vp, vp, C.c_size_t, C.c_size_t, vp]
        L.ptss_update_rejected.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_resort_triangles.argtypes = [vp, vp]
        L.ptss_resort_launches.argtypes = [vp, C.POINTER(C.c_ulonglong)]
        L.ptss_reseed.argtypes = [vp, C.c_ulonglong]
        L.ptss_read_strip_words.argtypes = [vp, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.ptss_read_triangle_bounds.argtypes = [vp, _f32p, C.c_size_t]
        L.ptss_read_triangle_positions.argtypes = [vp, C.POINTER(C.c_int), C.c_size_t]
        L.ptss_error_string.argtypes = [C.c_int]
        L.ptss_error_string.restype = C.c_char_p
        L.ptss_last_error_detail.restype = C.c_char_p
        _dev = L
    return _dev


def _check(rc):
    if rc != 0:
        L = device_lib()
        raise PtssError(f"ptss error {rc} ({L.ptss_error_string(rc).decode()}): {L.ptss_last_error_detail().decode()}")


class Scene:
    """class Scene of the host mirror (reference: CudaTracer/Scene.h:5-27), built from a preset name."""

    def __init__(self, preset="default"):
        self._h = C.c_void_p()
        rc = host_lib().ptss_scene_create(preset.encode(), C.byref(self._h))
        if rc != 0:
            raise PtssError(f"unknown scene preset {preset!r}")
        self.preset = preset
        self.desc = SceneDesc()
        host_lib().ptss_scene_describe(self._h, C.byref(self.desc))
        self.desc._owner = self  # desc borrows the scene's arrays: `Scene(p).desc` must keep the scene alive

    def add_obj(self, path, transform=None, material=0):
        """Scene::addObjModel: appends the triangles of a Wavefront OBJ file, placed by `transform` (4x4, row-major, applied to
        column vectors; None = identity), all with material index `material`. Returns the number added. Raises PtssError on a
        file that cannot be read, a malformed line or an index out of range; the scene is then unchanged. The scene's tables are
        described again, so `desc` (and arrays taken from it before) must be re-read after this call."""
        m = None
        if transform is not None:
            t = np.ascontiguousarray(np.asarray(transform, dtype=np.float32).reshape(4, 4))
            m = t.ctypes.data_as(_f32p)
        added = C.c_size_t()
        rc = host_lib().ptss_scene_add_obj(self._h, os.fsencode(path), m, int(material), C.byref(added))
        if rc != 0:
            raise PtssError(f"add_obj({path!r}) failed: {'cannot read the file' if rc == -2 else 'malformed OBJ or bad argument'} ({rc})")
        owner = self
        self.desc = SceneDesc()
        host_lib().ptss_scene_describe(self._h, C.byref(self.desc))
        self.desc._owner = owner
        return added.value

    def __del__(self):
        if getattr(self, "_h", None) and self._h.value and host_lib is not None:
            host_lib().ptss_scene_destroy(self._h)
            self._h = C.c_void_p()

    def _arr(self, ptr, n):
        return [ptr[i] for i in range(n)]

    @property
    def spheres(self):
        return self._arr(self.desc.spheres, self.desc.numSpheres)

    @property
    def triangles(self):
        return self._arr(self.desc.triangles, self.desc.numTriangles)

    @property
    def materials(self):
        return self._arr(self.desc.materials, self.desc.numMaterials)

    @property
    def area_lights(self):
        return self._arr(self.desc.areaLights, self.desc.numAreaLights)

    @property
    def point_lights(self):
        return self._arr(self.desc.pointLights, self.desc.numPointLights)

    def table(self):
        """Plain-Python dump of every record (the committed scene fixtures)."""
        return {
            "spheres": [struct_to_dict(s) for s in self.spheres],
            "triangles": [struct_to_dict(s) for s in self.triangles],
            "materials": [struct_to_dict(s) for s in self.materials],
            "pointLights": [struct_to_dict(s) for s in self.point_lights],
            "areaLights": [struct_to_dict(s) for s in self.area_lights],
        }


def probe_mesh_bound(tris, origins, directions, margin=1.0):
    """csrc/ptmesh.h on the host: ONE bound built around `tris` ((n, 9) floats {v0, e1, e2}); per ray (origin, direction) 1 if
    the ray may be accepted by one of them, 0 if provably not. Returns (verdicts, the bound's 12 floats)."""
    t = np.ascontiguousarray(np.asarray(tris, dtype=np.float32).reshape(-1, 9))
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
    d = np.ascontiguousarray(np.asarray(directions, dtype=np.float32).reshape(-1, 3))
    out = np.zeros(len(o), dtype=np.int32)
    bound = np.zeros(12, dtype=np.float32)
    rc = host_lib().ptss_probe_mesh_bound(t.ctypes.data_as(_f32p), len(t), o.ctypes.data_as(_f32p), d.ctypes.data_as(_f32p), len(o),
                                          float(margin), out.ctypes.data_as(C.POINTER(C.c_int)), bound.ctypes.data_as(_f32p))
    if rc != 0:
        raise PtssError(f"ptss_probe_mesh_bound: {rc}")
    return out, bound


def probe_mesh_refit(tris):
    """csrc/ptmesh.h refitBound on the host: `tris` ((n, 9) floats {v0, e1, e2} in STORED order) -> (leaves + groups, 12) float32,
    the leaves' bounds first, then the groups' — what Renderer.triangle_bounds() returns after update_triangles, bit for bit."""
    t = np.ascontiguousarray(np.asarray(tris, dtype=np.float32).reshape(-1, 9))
    leaves = (len(t) + 15) // 16
    out = np.zeros((leaves + (leaves + 15) // 16, 12), dtype=np.float32)
    rc = host_lib().ptss_probe_mesh_refit(t.ctypes.data_as(_f32p), len(t), out.ctypes.data_as(_f32p))
    if rc != 0:
        raise PtssError(f"ptss_probe_mesh_refit: {rc}")
    return out


def probe_kd_order(triangles, signed_zero=False):
    """csrc/ptorder.h on the host: the stored position of each original index under the kd order Renderer.resort_triangles()
    rebuilds — an (n,) TRIANGLE_DTYPE array (only the vertices are read) -> (n,) int32. Every 16 consecutive positions hold what
    the packer puts into that leaf. signed_zero: float codes that keep -0.0 below +0.0 (not the packer's order; for tests)."""
    a = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    out = np.empty(len(a), dtype=np.int32)
    L = host_lib()
    fn = L.ptss_probe_kd_order_signed_zero if signed_zero else L.ptss_probe_kd_order
    rc = fn(a.ctypes.data, len(a), out.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise PtssError(f"ptss_probe_kd_order: {rc}")
    return out


def probe_mesh_touch(bound, origins, directions, margin=1.0):
    """ptmesh.h mayTouch of ONE given bound (12 floats) for each ray: 1 may be accepted by a triangle inside, 0 provably not."""
    b = np.ascontiguousarray(np.asarray(bound, dtype=np.float32).reshape(12))
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.float32).reshape(-1, 3))
    d = np.ascontiguousarray(np.asarray(directions, dtype=np.float32).reshape(-1, 3))
    out = np.zeros(len(o), dtype=np.int32)
    rc = host_lib().ptss_probe_mesh_touch(b.ctypes.data_as(_f32p), o.ctypes.data_as(_f32p), d.ctypes.data_as(_f32p), len(o), float(margin),
                                          out.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise PtssError(f"ptss_probe_mesh_touch: {rc}")
    return out


def probe_pack_scene_images(scene, every_sphere_loop=False):
    """How many images (1 or 2) ptss_create builds for `scene` (a ptss.Scene or anything with a .desc)."""
    n = C.c_int()
    rc = host_lib().ptss_probe_pack_scene(C.byref(scene.desc), 1 if every_sphere_loop else 0, 0, C.byref(n), None, None, 0, None, 0, None)
    if rc != 0:
        raise PtssError(f"ptss_probe_pack_scene: {rc}")
    return n.value


def probe_pack_scene(scene, every_sphere_loop=False, image=0):
    """csrc/ptpack.h on the host: the scene image ptss_create builds for `scene` (a ptss.Scene or anything with a .desc).
    Returns (layout: dict of SceneLayout field -> int, blob: (rows, 4) float32 — view it as int32 / uint32 for the integer tables —,
    in_lds). The union's words appear as triClassPack0..4 and as the mesh image's numLeaves .. reserved."""
    every = 1 if every_sphere_loop else 0
    raw = np.zeros(len(SCENE_LAYOUT_FIELDS), dtype=np.int32)
    in_lds, words = C.c_int(), C.c_size_t()
    blob = np.empty(1 << 16, dtype=np.float32)   # most images fit; a larger one is packed again into a buffer of its size
    for _ in range(2):
        rc = host_lib().ptss_probe_pack_scene(C.byref(scene.desc), every, int(image), None, C.byref(in_lds), raw.ctypes.data_as(C.c_void_p),
                                              raw.nbytes, blob.ctypes.data_as(_f32p), blob.size, C.byref(words))
        if rc == 0 or words.value <= blob.size:
            break
        blob = np.empty(words.value, dtype=np.float32)
    if rc != 0:
        raise PtssError(f"ptss_probe_pack_scene: {rc}")
    layout = {name: int(v) for name, v in zip(SCENE_LAYOUT_FIELDS, raw)}
    layout.update({f"triClassPack{k}": layout[f"triClassPack{k}"] & 0xFFFFFFFF for k in range(5)})   # unsigned words
    layout.update({name: layout[f"triClassPack{k}"] for k, name in enumerate(SCENE_LAYOUT_MESH_FIELDS)})
    return layout, blob[:words.value].reshape(-1, 4).copy(), bool(in_lds.value)


def default_camera():
    cam = Camera()
    host_lib().ptss_camera_default(C.byref(cam))
    return cam


def move_camera(cam, key):
    moved = C.c_int(0)
    host_lib().ptss_camera_move(C.byref(cam), ord(key), C.byref(moved))
    return bool(moved.value)


RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("tmax", np.float32), ("direction", np.float32, 3), ("pad", np.float32)])
HIT_DTYPE = np.dtype([("point", np.float32, 3), ("distance", np.float32), ("normal", np.float32, 3), ("materialIdx", np.int32),
                      ("kind", np.int32), ("primitive", np.int32), ("w1", np.float32), ("w2", np.float32)])
TRIANGLE_DTYPE = np.dtype([("vertex0", np.float32, 3), ("vertex1", np.float32, 3), ("vertex2", np.float32, 3), ("normal0", np.float32, 3),
                           ("normal1", np.float32, 3), ("normal2", np.float32, 3), ("materialIdx", np.int32)])
assert TRIANGLE_DTYPE.itemsize == C.sizeof(Triangle)
FEATURE_DTYPE = np.dtype([("normal", np.float32, 3), ("depth", np.float32), ("albedo", np.float32, 3), ("materialIdx", np.int32)])
assert RAY_DTYPE.itemsize == C.sizeof(RayQuery) and HIT_DTYPE.itemsize == C.sizeof(RayHit)
assert FEATURE_DTYPE.itemsize == C.sizeof(PixelFeature)
HISTORY_DTYPE = np.dtype([("r", np.float32), ("g", np.float32), ("b", np.float32), ("weight", np.float32)])
assert HISTORY_DTYPE.itemsize == C.sizeof(HistoryEntry)
MOTION_DTYPE = np.dtype([("prevPoint", np.float32, 3), ("surface", np.int32)])
assert MOTION_DTYPE.itemsize == C.sizeof(PixelMotion)


def _query_rays(rays):
    """The rays of a ray or a path query as (N, 8) float32 rows."""
    a = np.asarray(rays)
    if a.dtype == RAY_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32).reshape(-1, 8)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("rays: (N, 8) float32 or (N,) RAY_DTYPE")
    return a


# what the queries say of a tensor they refuse
_QUERY_TEXTS = {"rays": "rays: a contiguous (N, 8) float32 device tensor", "rng": "rng: a contiguous (N, 6) int32 tensor on the rays' device"}


def _records(rows, dtype):
    """Plain rows as (N,) records of `dtype`; None stays None."""
    return rows.view(dtype).reshape(-1) if rows is not None else None


# ---- the schedule of a path query (ptss_trace_paths_opt) ----
def path_options(schedule=PATHS_LANE_PER_RAY, max_workgroups=0):
    """A ptss_path_options. schedule: PATHS_LANE_PER_RAY, PATHS_REFILL or "lane_per_ray" / "refill"; max_workgroups: the refill grid's
    cap, 0 = the library's choice."""
    o = PathOptions()
    o.structSize = C.sizeof(PathOptions)
    o.schedule = {"lane_per_ray": PATHS_LANE_PER_RAY, "refill": PATHS_REFILL}.get(schedule, schedule)
    o.maxWorkgroups = int(max_workgroups)
    o.reserved = 0
    return o


# ---- the schedule of a chain query (ptss_intersect_chain) ----
def chain_options(schedule=CHAIN_LANE_PER_RAY, max_workgroups=0):
    """A ptss_chain_options. schedule: CHAIN_LANE_PER_RAY, CHAIN_REFILL or "lane" / "refill"; max_workgroups: the refill grid's cap,
    0 = the library's choice."""
    o = ChainOptions()
    o.structSize = C.sizeof(ChainOptions)
    o.schedule = {"lane": CHAIN_LANE_PER_RAY, "lane_per_ray": CHAIN_LANE_PER_RAY, "refill": CHAIN_REFILL}.get(schedule, schedule)
    o.maxWorkgroups = int(max_workgroups)
    o.reserved = 0
    return o


# ---- the film of a path query (ptss_generate_rays / ptss_accumulate_paths / ptss_ray_features) ----
def film_camera(kind, width, height, camera=None, lens_radius=0.0, focus_distance=1.0, jitter=1):
    """A ptss_film_camera. kind: FILM_PINHOLE, FILM_THIN_LENS, FILM_EQUIRECT or "pinhole" / "thinlens" / "equirect"; camera: a Camera
    (default_camera() otherwise); lens_radius, focus_distance: the thin lens only; jitter: 1 draws from the ray's stream, 0 draws nothing."""
    kinds = {"pinhole": FILM_PINHOLE, "thinlens": FILM_THIN_LENS, "thin_lens": FILM_THIN_LENS, "equirect": FILM_EQUIRECT}
    f = FilmCamera()
    f.structSize = C.sizeof(FilmCamera)
    f.kind = kinds[kind] if isinstance(kind, str) else int(kind)
    C.memmove(C.byref(f.camera), C.byref(camera if camera is not None else default_camera()), C.sizeof(Camera))
    f.width, f.height = int(width), int(height)
    f.lensRadius, f.focusDistance = float(lens_radius), float(focus_distance)
    f.jitter = int(jitter)
    return f


def film_draws(film):
    """The uniforms a film's model takes from a ray's stream: pinhole 2, thin lens 4, equirect 2; none with jitter = 0."""
    return 0 if not film.jitter else (4 if film.kind == FILM_THIN_LENS else 2)


def _rng_words(rng):
    s = np.asarray(rng)
    if s.dtype == PATH_RNG_DTYPE:
        s = np.ascontiguousarray(s).view(np.uint32).reshape(-1, 6)
    s = np.array(s, dtype=np.uint32, order="C")   # a copy: advanced in place
    if s.ndim != 2 or s.shape[1] != 6:
        raise ValueError("rng: (N,) PATH_RNG_DTYPE or (N, 6) uint32")
    return s


def _film_index(index, n):
    if index is None:
        return None
    i = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1)
    if len(i) != n:
        raise ValueError("index: one film pixel per ray")
    return i


def _rows(value, dtype, words, word_dtype, what, copy=False):
    """`value` as an (N, words) array of word_dtype: a record array of `dtype` or the plain rows."""
    a = np.asarray(value)
    if a.dtype == dtype:
        a = np.ascontiguousarray(a).view(word_dtype).reshape(-1, words)
    a = np.array(a, dtype=word_dtype, order="C") if copy else np.ascontiguousarray(a, dtype=word_dtype)
    if a.ndim != 2 or a.shape[1] != words:
        raise ValueError(f"{what}: (N,) records or (N, {words}) {np.dtype(word_dtype).name}")
    return a


def _output_rows(P, value, what):
    """An optional output of a film call as (P, 4) rows: None (NULL), True (zeros beforehand) or the buffer's content beforehand (a copy).
    "pixels" are bytes, every other output HISTORY_DTYPE."""
    if value is None:
        return None
    if what == "pixels":
        return np.zeros((P, 4), dtype=np.uint8) if value is True else np.array(value, dtype=np.uint8, order="C").reshape(-1, 4)
    return np.zeros((P, 4), dtype=np.float32) if value is True else _rows(value, HISTORY_DTYPE, 4, np.float32, what, copy=True)


def _film_outputs(P, **outputs):
    """_output_rows of each named output, in order, each of them one entry per film pixel."""
    rows = [_output_rows(P, value, what) for what, value in outputs.items()]
    if any(a is not None and len(a) != P for a in rows):
        names = list(outputs)
        raise ValueError(f"{', '.join(names[:-1])} and {names[-1]}: one entry per film pixel")
    return rows


def probe_film_rays(film, rng, first_pixel=0, index=None, rays=None):
    """ptss_generate_rays on the host (csrc/ptcamera.h; the specification of the device's rays) -> ((N,) RAY_DTYPE, (N,) PATH_RNG_DTYPE:
    the streams afterwards, number of index entries dropped). rays: the buffer's content beforehand (zeros otherwise): an entry whose
    index leaves the film keeps it."""
    s = _rng_words(rng)
    n = len(s)
    idx = _film_index(index, n)
    out = np.zeros((n, 8), dtype=np.float32) if rays is None else _rows(rays, RAY_DTYPE, 8, np.float32, "rays", copy=True)
    if len(out) != n:
        raise ValueError("rays: one row per stream")
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_film_rays(C.byref(film), int(first_pixel), idx.ctypes.data_as(C.c_void_p) if idx is not None else None, n,
                                         s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_film_rays: {rc}")
    return out.view(RAY_DTYPE).reshape(-1), s.view(PATH_RNG_DTYPE).reshape(-1), int(rejected.value)


def probe_accumulate(results, film, first_pixel=0, index=None, pixels=None, history=None):
    """ptss_accumulate_paths on the host, with the literal tone map -> (film afterwards (P,) FILM_DTYPE, pixels (P, 4) uint8 or None,
    history (P,) HISTORY_DTYPE or None, number of index entries dropped). film: (P,) FILM_DTYPE or (P, 4) uint32 (not modified);
    pixels / history: None (not written), True (zeros beforehand) or the buffer's content beforehand."""
    r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
    n = len(r)
    idx = _film_index(index, n)
    f = _rows(film, FILM_DTYPE, 4, np.uint32, "film", copy=True)
    px, hs = _output_rows(len(f), pixels, "pixels"), _output_rows(len(f), history, "history")
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_accumulate(r.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p) if idx is not None else None, int(first_pixel),
                                          n, f.ctypes.data_as(C.c_void_p), len(f), px.ctypes.data_as(C.c_void_p) if px is not None else None,
                                          hs.ctypes.data_as(C.c_void_p) if hs is not None else None, C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_accumulate: {rc}")
    return (f.view(FILM_DTYPE).reshape(-1), px, hs.view(HISTORY_DTYPE).reshape(-1) if hs is not None else None, int(rejected.value))


# ---- adaptive film sampling (ptss_accumulate_paths_stats / ptss_plan_samples) ----
def plan_params(min_samples=8, max_samples=1 << 23, threshold=0.5):
    """A ptss_plan_params; the defaults are ptss_default_plan_params' (design choices, not measurements)."""
    p = PlanParams()
    p.structSize = C.sizeof(PlanParams)
    p.minSamples, p.maxSamples, p.threshold = int(min_samples), int(max_samples), float(threshold)
    return p


def plan_info_dict(info):
    """A PlanInfo (or its four 64-bit words) as a dict."""
    if not isinstance(info, PlanInfo):
        info = PlanInfo.from_buffer_copy(np.ascontiguousarray(info).tobytes())
    return dict(totalWeight=int(info.totalWeight), activePixels=int(info.activePixels), unsampledPixels=int(info.unsampledPixels),
                cappedPixels=int(info.cappedPixels), uniform=int(info.uniform))


def _moments(moments, P):
    m = np.array(moments, dtype=np.uint64, order="C").reshape(-1)   # a copy
    if len(m) != P:
        raise ValueError("moments: one uint64 per film pixel")
    return m


def probe_accumulate_stats(results, film, moments, first_pixel=0, index=None, pixels=None, history=None):
    """ptss_accumulate_paths_stats on the host, with the literal tone map -> (film, moments (P,) uint64, pixels, history, dropped):
    probe_accumulate's arguments and results, with the moments beforehand (not modified) and afterwards."""
    r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
    n = len(r)
    idx = _film_index(index, n)
    f = _rows(film, FILM_DTYPE, 4, np.uint32, "film", copy=True)
    m = _moments(moments, len(f))
    px, hs = _output_rows(len(f), pixels, "pixels"), _output_rows(len(f), history, "history")
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_accumulate_stats(r.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p) if idx is not None else None,
                                                int(first_pixel), n, f.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), len(f),
                                                px.ctypes.data_as(C.c_void_p) if px is not None else None,
                                                hs.ctypes.data_as(C.c_void_p) if hs is not None else None, C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_accumulate_stats: {rc}")
    return (f.view(FILM_DTYPE).reshape(-1), m, px, hs.view(HISTORY_DTYPE).reshape(-1) if hs is not None else None, int(rejected.value))


def probe_plan_samples(film, moments, n, params=None):
    """ptss_plan_samples on the host (csrc/ptadaptive.h; the specification of the device's plan) -> (cdf (P,) uint64, index (n,) uint32,
    info: a dict). film: (P,) FILM_DTYPE or (P, 4) uint32; moments: (P,) uint64."""
    f = _rows(film, FILM_DTYPE, 4, np.uint32, "film")
    m = _moments(moments, len(f))
    params = params if params is not None else plan_params()
    return _probe_plan("ptss_probe_plan_samples", len(f), n, _ptr(f), _ptr(m), len(f), C.byref(params))


def _probe_plan(name, P, n, *front):
    """The body of probe_plan_samples and probe_plan_samples_linear: host call `name`, `front` its arguments in front of n."""
    cdf, index, info = np.zeros(P, dtype=np.uint64), np.zeros(int(n), dtype=np.uint32), PlanInfo()
    rc = getattr(host_lib(), name)(*front, int(n), _ptr(cdf), _ptr(index), C.byref(info))
    if rc != 0:
        raise PtssError(f"{name}: {rc}")
    return cdf, index, plan_info_dict(info)


def plan_cdf_entries(film_pixels):
    """ptss_plan_cdf_entries: the 64-bit entries dev_cdf must hold for a film of that many pixels."""
    out = C.c_size_t(0)
    _check(device_lib().ptss_plan_cdf_entries(int(film_pixels), C.byref(out)))
    return int(out.value)


# ---- the linear film (ptss_accumulate_paths_linear / ptss_resolve_linear) ----
def linear_params(scale_log2=20, clamp_max=65536.0, exposure=1.0):
    """A ptss_linear_params; the defaults are ptss_default_linear_params' (design choices, not measurements)."""
    p = LinearParams()
    p.structSize = C.sizeof(LinearParams)
    p.scaleLog2, p.clampMax, p.exposure, p.reserved = int(scale_log2), float(clamp_max), float(exposure), 0
    return p


def _linear_range(P, first_pixel, count):
    first_pixel = int(first_pixel)
    count = P - first_pixel if count is None else int(count)
    if first_pixel < 0 or count < 0 or first_pixel + count > P:
        raise ValueError("first_pixel + count leaves the film")
    return first_pixel, count


def probe_accumulate_linear(results, film, first_pixel=0, index=None, params=None):
    """ptss_accumulate_paths_linear on the host (csrc/ptlinear.h; the specification of the device's film) -> (film afterwards (P,)
    LINEAR_DTYPE, number of index entries dropped). film: (P,) LINEAR_DTYPE or (P, 4) uint64 (not modified)."""
    r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
    n = len(r)
    idx = _film_index(index, n)
    f = _rows(film, LINEAR_DTYPE, 4, np.uint64, "film", copy=True)
    params = params if params is not None else linear_params()
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_accumulate_linear(r.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p) if idx is not None else None,
                                                 int(first_pixel), n, f.ctypes.data_as(C.c_void_p), len(f), C.byref(params), C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_accumulate_linear: {rc}")
    return f.view(LINEAR_DTYPE).reshape(-1), int(rejected.value)


def probe_resolve_linear(film, first_pixel=0, count=None, params=None, linear=True, pixels=True, history=True):
    """ptss_resolve_linear on the host, with the literal tone map -> (linear (P,) HISTORY_DTYPE: the unexposed means and the sample
    count, pixels (P, 4) uint8, history (P,) HISTORY_DTYPE), each None when not asked for. film: (P,) LINEAR_DTYPE or (P, 4) uint64;
    count: None = to the film's end; linear / pixels / history: None (not written), True (zeros beforehand) or the content beforehand."""
    return _probe_resolve("ptss_probe_resolve_linear", LINEAR_DTYPE, film, first_pixel, count, params, linear, pixels, history)


def _probe_resolve(name, film_dtype, film, first_pixel, count, params, linear, pixels, history):
    """The body of probe_resolve_linear and probe_resolve_splat: one host call over a film of 32-byte entries."""
    f = _rows(film, film_dtype, 4, np.uint64, "film")
    P = len(f)
    first_pixel, count = _linear_range(P, first_pixel, count)
    ln, px, hs = _film_outputs(P, linear=linear, pixels=pixels, history=history)
    params = params if params is not None else linear_params()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = getattr(host_lib(), name)(ptr(f), first_pixel, count, C.byref(params), ptr(ln), ptr(px), ptr(hs))
    if rc != 0:
        raise PtssError(f"{name}: {rc}")
    return (ln.view(HISTORY_DTYPE).reshape(-1) if ln is not None else None, px, hs.view(HISTORY_DTYPE).reshape(-1) if hs is not None else None)


# ---- adaptive sampling on the linear film (ptss_accumulate_paths_linear_stats / ptss_plan_samples_linear) ----
def linear_plan_params(min_samples=8, max_samples=1 << 23, threshold=0.02, floor=1.0 / 64.0):
    """A ptss_linear_plan_params; the defaults are ptss_default_linear_plan_params' (design choices, not measurements)."""
    p = LinearPlanParams()
    p.structSize = C.sizeof(LinearPlanParams)
    p.minSamples, p.maxSamples, p.threshold, p.floor = int(min_samples), int(max_samples), float(threshold), float(floor)
    return p


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def probe_accumulate_linear_stats(results, film, moments, first_pixel=0, index=None, params=None):
    """ptss_accumulate_paths_linear_stats on the host (csrc/ptlinstats.h; the specification of the device's moments) -> (film afterwards
    (P,) LINEAR_DTYPE or None, moments afterwards (P,) MOMENT_DTYPE, number of index entries dropped). film: (P,) LINEAR_DTYPE or (P, 4)
    uint64, or None (moments only); moments: (P,) MOMENT_DTYPE or (P, 4) uint64. Neither is modified."""
    r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
    n = len(r)
    idx = _film_index(index, n)
    m = _rows(moments, MOMENT_DTYPE, 4, np.uint64, "moments", copy=True)
    f = _rows(film, LINEAR_DTYPE, 4, np.uint64, "film", copy=True) if film is not None else None
    if f is not None and len(f) != len(m):
        raise ValueError("moments: one row per film pixel")
    params = params if params is not None else linear_params()
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_accumulate_linear_stats(_ptr(r), _ptr(idx), int(first_pixel), n, _ptr(f), _ptr(m), len(m), C.byref(params),
                                                       C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_accumulate_linear_stats: {rc}")
    return (f.view(LINEAR_DTYPE).reshape(-1) if f is not None else None), m.view(MOMENT_DTYPE).reshape(-1), int(rejected.value)


def probe_plan_samples_linear(moments, n, params=None, plan=None):
    """ptss_plan_samples_linear on the host (csrc/ptlinstats.h; the specification of the device's plan) -> (cdf (P,) uint64, index (n,)
    uint32, info: a dict). moments: (P,) MOMENT_DTYPE or (P, 4) uint64; params: the film's linear_params; plan: a linear_plan_params."""
    m = _rows(moments, MOMENT_DTYPE, 4, np.uint64, "moments")
    params = params if params is not None else linear_params()
    plan = plan if plan is not None else linear_plan_params()
    return _probe_plan("ptss_probe_plan_samples_linear", len(m), n, _ptr(m), len(m), C.byref(params), C.byref(plan))


def probe_linear_plan_weight(moment, params=None, plan=None):
    """The weight ptss_plan_samples_linear gives one moment row (sumY, sqLo, sqHi, samples); PtssError for refused parameters."""
    m = LinearMoment(*[int(v) for v in moment])
    params = params if params is not None else linear_params()
    plan = plan if plan is not None else linear_plan_params()
    w = int(host_lib().ptss_probe_linear_plan_weight(C.byref(m), C.byref(params), C.byref(plan)))
    if w == 0xffffffff:
        raise PtssError("ptss_probe_linear_plan_weight: refused")
    return w


# ---- the filtered linear film (ptss_splat_paths / ptss_splat_paths_homed / ptss_resolve_splat) ----
_SPLAT_KINDS = {"box": SPLAT_BOX, "tent": SPLAT_TENT, "gaussian": SPLAT_GAUSSIAN}


def splat_filter(kind="tent", radius=1.0, alpha=2.0):
    """A ptss_splat_filter; kind: "box", "tent", "gaussian" or a PTSS_SPLAT_* value; the defaults are ptss_default_splat_filter's (design
    choices, not measurements)."""
    f = SplatFilter()
    f.structSize = C.sizeof(SplatFilter)
    f.kind, f.radius, f.alpha, f.reserved = int(_SPLAT_KINDS.get(kind, kind)), float(radius), float(alpha), 0
    return f


def _positions(positions, n):
    a = np.asarray(positions)
    if a.dtype == POSITION_DTYPE:
        a = np.ascontiguousarray(a).view(np.float32).reshape(-1, 2)
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape != (n, 2):
        raise ValueError("positions: one (x, y) per result, (N,) POSITION_DTYPE or (N, 2) float32")
    return a


def probe_film_positions(film, rng, first_pixel=0, index=None, rays=None):
    """ptss_generate_rays_positions on the host -> probe_film_rays' ((N,) RAY_DTYPE, (N,) PATH_RNG_DTYPE, ...) with the positions, (N,)
    POSITION_DTYPE, in front of the dropped count: (rays, streams, positions, dropped)."""
    s = _rng_words(rng)
    n = len(s)
    idx = _film_index(index, n)
    out = np.zeros((n, 8), dtype=np.float32) if rays is None else _rows(rays, RAY_DTYPE, 8, np.float32, "rays", copy=True)
    if len(out) != n:
        raise ValueError("rays: one row per stream")
    pos = np.zeros((n, 2), dtype=np.float32)
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_film_positions(C.byref(film), int(first_pixel), idx.ctypes.data_as(C.c_void_p) if idx is not None else None, n,
                                              s.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p),
                                              C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_film_positions: {rc}")
    return out.view(RAY_DTYPE).reshape(-1), s.view(PATH_RNG_DTYPE).reshape(-1), pos.view(POSITION_DTYPE).reshape(-1), int(rejected.value)


def probe_splat_paths(results, positions, film, width, height, filter=None, params=None, homed_first_pixel=None):
    """ptss_splat_paths (homed_first_pixel = None) or ptss_splat_paths_homed on the host (csrc/ptsplat.h; the specification of the
    device's film) -> (film afterwards (P,) SPLAT_DTYPE, samples dropped, samples clamped). film: (width * height,) SPLAT_DTYPE or
    (P, 4) uint64 (not modified)."""
    r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
    n = len(r)
    pos = _positions(positions, n)
    f = _rows(film, SPLAT_DTYPE, 4, np.uint64, "film", copy=True)
    if len(f) != int(width) * int(height):
        raise ValueError("film: width * height entries")
    filter = filter if filter is not None else splat_filter()
    params = params if params is not None else linear_params()
    first = C.byref(C.c_size_t(int(homed_first_pixel))) if homed_first_pixel is not None else None
    dropped, clamped = C.c_ulonglong(0), C.c_ulonglong(0)
    rc = host_lib().ptss_probe_splat_paths(r.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p), first, n, f.ctypes.data_as(C.c_void_p),
                                           int(width), int(height), C.byref(filter), C.byref(params), C.byref(dropped), C.byref(clamped))
    if rc != 0:
        raise PtssError(f"ptss_probe_splat_paths: {rc}")
    return f.view(SPLAT_DTYPE).reshape(-1), int(dropped.value), int(clamped.value)


def probe_resolve_splat(film, first_pixel=0, count=None, params=None, linear=True, pixels=True, history=True):
    """ptss_resolve_splat on the host, with the literal tone map: probe_resolve_linear's arguments and results over a (P,) SPLAT_DTYPE
    film; the weight of linear and history is the summed filter weight (1 per whole sample)."""
    return _probe_resolve("ptss_probe_resolve_splat", SPLAT_DTYPE, film, first_pixel, count, params, linear, pixels, history)


# ---- the meter of the two linear films (ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure) ----
def meter_params(key=0.18, low_permille=100, high_permille=20, rate=1.0, min_exposure=2.0 ** -16, max_exposure=2.0 ** 16):
    """A ptss_meter_params; the defaults are ptss_default_meter_params' (design choices, not measurements)."""
    p = MeterParams()
    p.structSize = C.sizeof(MeterParams)
    p.key, p.lowPermille, p.highPermille, p.rate = float(key), int(low_permille), int(high_permille), float(rate)
    p.minExposure, p.maxExposure, p.reserved = float(min_exposure), float(max_exposure), 0
    return p


def _histogram(histogram):
    """A meter's histogram as (METER_BINS,) uint32, a copy: None = zeros."""
    h = np.zeros(METER_BINS, dtype=np.uint32) if histogram is None else np.array(histogram, dtype=np.uint32, order="C").reshape(-1)
    if len(h) != METER_BINS:
        raise ValueError("histogram: METER_BINS uint32 counts")
    return h


def _meter_state(state):
    """A meter's state as (1,) METER_STATE_DTYPE, a copy: None = a new state."""
    if state is None:
        return np.zeros(1, dtype=METER_STATE_DTYPE)
    if isinstance(state, MeterState):
        return np.frombuffer(bytes(state), dtype=METER_STATE_DTYPE).copy()
    s = np.array(state, dtype=METER_STATE_DTYPE, order="C").reshape(-1)
    if len(s) != 1:
        raise ValueError("state: one METER_STATE_DTYPE record")
    return s


def probe_meter_bin(entry, splat=False):
    """The bin csrc/ptmeter.h gives one film entry -> (bin, or -1 for a pixel that is not metered; its fixed-point luminance Y). entry: a
    LINEAR_DTYPE record (splat: SPLAT_DTYPE) or its four uint64 words."""
    e = np.ascontiguousarray(entry).view(np.uint64).reshape(-1) if np.asarray(entry).dtype.fields else np.array(entry, dtype=np.uint64).reshape(-1)
    if len(e) != 4:
        raise ValueError("entry: one film entry, four 64-bit words")
    b, y = C.c_int(0), C.c_ulonglong(0)
    if host_lib().ptss_probe_meter_bin(e.ctypes.data_as(C.c_void_p), 1 if splat else 0, C.byref(b), C.byref(y)) != 0:
        raise PtssError("ptss_probe_meter_bin")
    return int(b.value), int(y.value)


def _probe_meter(name, film_dtype, film, first_pixel, count, histogram):
    f = _rows(film, film_dtype, 4, np.uint64, "film")
    first_pixel, count = _linear_range(len(f), first_pixel, count)
    h = _histogram(histogram)
    rc = getattr(host_lib(), name)(f.ctypes.data_as(C.c_void_p), first_pixel, count, h.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"{name}: {rc}")
    return h


def probe_meter_linear(film, first_pixel=0, count=None, histogram=None):
    """ptss_meter_linear on the host (csrc/ptmeter.h; the specification of the device's histogram) -> the histogram afterwards,
    (METER_BINS,) uint32. film: (P,) LINEAR_DTYPE or (P, 4) uint64; histogram: the counts beforehand (not modified; None = zeros)."""
    return _probe_meter("ptss_probe_meter_linear", LINEAR_DTYPE, film, first_pixel, count, histogram)


def probe_meter_splat(film, first_pixel=0, count=None, histogram=None):
    """ptss_meter_splat on the host: probe_meter_linear over a (P,) SPLAT_DTYPE film."""
    return _probe_meter("ptss_probe_meter_splat", SPLAT_DTYPE, film, first_pixel, count, histogram)


def probe_meter_exposure(histogram, state=None, params=None, meter=None):
    """ptss_meter_exposure on the host -> the state afterwards, (1,) METER_STATE_DTYPE. state: the state beforehand (not modified; None = a
    new one); params: the film's linear_params; meter: a meter_params."""
    h, s = _histogram(histogram), _meter_state(state)
    params = params if params is not None else linear_params()
    meter = meter if meter is not None else meter_params()
    rc = host_lib().ptss_probe_meter_exposure(h.ctypes.data_as(C.c_void_p), C.byref(params), C.byref(meter), s.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_meter_exposure: {rc}")
    return s


# ---- glare for the two linear films (ptss_glare_build and the glare resolves) ----
_GLARE_MODES = {"add": GLARE_ADD, "mix": GLARE_MIX}
_FILM_KINDS = {"linear": FILM_LINEAR, "splat": FILM_SPLAT}   # the names of the PTSS_FILM_* values (the glare calls' PTSS_GLARE_FILM_* are the same)


def _film_kind(film_kind, default=None):
    """A film_kind argument as its PTSS_FILM_* value: "linear", "splat" or a value; None: `default`."""
    film_kind = default if film_kind is None else film_kind
    return int(_FILM_KINDS.get(film_kind, film_kind))


def glare_params(levels=6, mode="mix", threshold=0.0, strength=0.1):
    """A ptss_glare_params; mode: "add", "mix" or a PTSS_GLARE_* value; the defaults are ptss_default_glare_params' (design choices, not
    measurements)."""
    p = GlareParams()
    p.structSize = C.sizeof(GlareParams)
    p.levels, p.mode, p.threshold, p.strength, p.reserved = int(levels), int(_GLARE_MODES.get(mode, mode)), float(threshold), float(strength), 0
    return p


def glare_layout(width, height, levels):
    """ptss_glare_layout (the host library's) -> ([(width, height, first entry) of level 1 .. levels], entries in all)."""
    out, n = (GlareLevel * GLARE_MAX_LEVELS)(), C.c_size_t(0)
    if host_lib().ptss_glare_layout(int(width), int(height), int(levels), out, C.byref(n)) != 0:
        raise PtssError("ptss_glare_layout")
    return [(out[k].width, out[k].height, int(out[k].first)) for k in range(int(levels))], int(n.value)


def _glare_film(film, film_kind, width, height):
    """A whole film as (width * height, 4) uint64 rows, and its PTSS_FILM_* value. film_kind: "linear", "splat", a value,
    or None: what the film's dtype says (plain rows count as linear)."""
    if film_kind is None:
        film_kind = FILM_SPLAT if np.asarray(film).dtype == SPLAT_DTYPE else FILM_LINEAR
    kind = _film_kind(film_kind)
    f = _rows(film, SPLAT_DTYPE if kind == FILM_SPLAT else LINEAR_DTYPE, 4, np.uint64, "film")
    if len(f) != int(width) * int(height):
        raise ValueError("film: width * height entries")
    return f, kind


def _glare_pyramid(pyramid, entries):
    """A pyramid as (entries, 4) uint64 rows."""
    a = _rows(pyramid, GLARE_DTYPE, 4, np.uint64, "pyramid")
    if len(a) < entries:
        raise ValueError("pyramid: the entries glare_layout counts")
    return a


def probe_glare_build(film, width, height, params=None, glare=None, film_kind=None):
    """ptss_glare_build on the host (csrc/ptglare.h; the specification of the device's pyramid) -> the pyramid, (entries,) GLARE_DTYPE:
    u_1 .. u_L as glare_layout places them. film: (width * height,) LINEAR_DTYPE or SPLAT_DTYPE, or (P, 4) uint64 with film_kind."""
    f, kind = _glare_film(film, film_kind, width, height)
    params = params if params is not None else linear_params()
    glare = glare if glare is not None else glare_params()
    out = np.zeros((max(glare_layout(width, height, glare.levels)[1], 1), 4), dtype=np.uint64)
    rc = host_lib().ptss_probe_glare_build(f.ctypes.data_as(C.c_void_p), kind, int(width), int(height), C.byref(params), C.byref(glare),
                                           out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_glare_build: {rc}")
    return out.view(GLARE_DTYPE).reshape(-1)


def probe_resolve_glare(film, width, height, pyramid, first_pixel=0, count=None, params=None, glare=None, state=None, linear=True, pixels=True,
                        history=True, film_kind=None):
    """ptss_resolve_linear_glare / ptss_resolve_splat_glare on the host, with the literal tone map -> probe_resolve_linear's results.
    pyramid: what probe_glare_build or Renderer.glare_build gave for this film and `glare`; state: a meter's state or None."""
    f, kind = _glare_film(film, film_kind, width, height)
    P = len(f)
    first_pixel, count = _linear_range(P, first_pixel, count)
    params = params if params is not None else linear_params()
    glare = glare if glare is not None else glare_params()
    pyr = _glare_pyramid(pyramid, glare_layout(width, height, glare.levels)[1])
    ln, px, hs = _film_outputs(P, linear=linear, pixels=pixels, history=history)
    st = _meter_state(state) if state is not None else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = host_lib().ptss_probe_resolve_glare(ptr(f), kind, first_pixel, count, C.byref(params), int(width), int(height), C.byref(glare), ptr(pyr),
                                             ptr(st), ptr(ln), ptr(px), ptr(hs))
    if rc != 0:
        raise PtssError(f"ptss_probe_resolve_glare: {rc}")
    return (ln.view(HISTORY_DTYPE).reshape(-1) if ln is not None else None, px, hs.view(HISTORY_DTYPE).reshape(-1) if hs is not None else None)


# ---- tone curves for the two linear films (ptss_tone_build, ptss_resolve_toned) ----
_TONE_CURVES = {"clamp": TONE_CLAMP, "reinhard": TONE_REINHARD, "filmic": TONE_FILMIC}
_TONE_TRANSFERS = {"gamma22": TRANSFER_GAMMA22, "srgb": TRANSFER_SRGB}
TONE_DEFAULT_FILMIC = (2.51, 0.03, 2.43, 0.59, 0.14)


def tone_params(curve="filmic", transfer="srgb", bits=8, luminance=False, white=4.0, filmic=TONE_DEFAULT_FILMIC):
    """A ptss_tone_params; curve: "clamp", "reinhard", "filmic" or a PTSS_TONE_* value; transfer: "gamma22", "srgb" or a PTSS_TRANSFER_*
    value; the defaults are ptss_default_tone_params' (design choices, not measurements)."""
    p = ToneParams()
    p.structSize = C.sizeof(ToneParams)
    p.curve, p.transfer, p.bits = int(_TONE_CURVES.get(curve, curve)), int(_TONE_TRANSFERS.get(transfer, transfer)), int(bits)
    p.flags, p.white, p.reserved = (TONE_LUMINANCE if luminance else 0), float(white), 0
    p.filmic[:] = [float(v) for v in filmic]
    return p


def tone_table_floats(bits):
    """ptss_tone_table_floats: the floats of a table, 2^bits + 4."""
    if bits not in (8, 10):
        raise ValueError("bits: 8 or 10")
    return (1 << bits) + 4


def tone_table_sorted(table):
    """Whether a table's builder found its thresholds in order: its flag T[K + 2] is 0."""
    t = np.asarray(table, dtype=np.float32).reshape(-1)
    return float(t[len(t) - 3]) == 0.0


def _tone_table(table, bits):
    t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1)
    if len(t) != tone_table_floats(bits):
        raise ValueError("table: tone_table_floats(bits) float32")
    return t


def probe_tone_build(tone=None):
    """ptss_tone_build on the host (csrc/pttone.h; the specification of the device's table) -> (tone_table_floats(bits),) float32: T[0] =
    -inf, T[1 .. K], NaN, the flag (0: in order), NaN, NaN. Raises where the thresholds came out of order."""
    tone = tone if tone is not None else tone_params()
    if tone.bits not in (8, 10):
        raise PtssError("ptss_probe_tone_build: -1")
    out = np.zeros(tone_table_floats(tone.bits), dtype=np.float32)
    rc = host_lib().ptss_probe_tone_build(C.byref(tone), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_tone_build: {rc}")
    return out


def probe_tone_value(tone, x):
    """The literal display value transfer(curve(x)) of `tone`, float32 in and out."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    v = np.zeros(x.shape, dtype=np.float32)
    rc = host_lib().ptss_probe_tone_value(C.byref(tone), x.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), x.size)
    if rc != 0:
        raise PtssError(f"ptss_probe_tone_value: {rc}")
    return v


def probe_tone_level(table, bits, x):
    """The level of x by the table: the number of k in 1 .. K with x >= table[k] -> uint32, x's shape."""
    t = _tone_table(table, bits)
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(x.shape, dtype=np.uint32)
    rc = host_lib().ptss_probe_tone_level(t.ctypes.data_as(C.c_void_p), int(bits), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size)
    if rc != 0:
        raise PtssError(f"ptss_probe_tone_level: {rc}")
    return out


def unpack_pixels10(pixels):
    """The words of a 10-bit toned resolve, (P, 4) uint8 or (P,) uint32 -> (P, 4) uint16: r, g, b in 0 .. 1023 and the two alpha bits."""
    w = np.ascontiguousarray(pixels)
    w = w.view(np.uint32).reshape(-1) if w.dtype == np.uint8 else w.astype(np.uint32).reshape(-1)
    return np.stack([w & 1023, (w >> 10) & 1023, (w >> 20) & 1023, w >> 30], axis=1).astype(np.uint16)


def pack_pixels10(rgba):
    """unpack_pixels10's inverse -> (P, 4) uint8, the words' bytes."""
    a = np.asarray(rgba, dtype=np.uint32).reshape(-1, 4)
    w = (a[:, 0] & 1023) | ((a[:, 1] & 1023) << 10) | ((a[:, 2] & 1023) << 20) | ((a[:, 3] & 3) << 30)
    return np.ascontiguousarray(w.astype(np.uint32)).view(np.uint8).reshape(-1, 4)


def probe_resolve_toned(film, tone, table, first_pixel=0, count=None, params=None, state=None, glare=None, linear=True, pixels=True, history=True,
                        film_kind=None):
    """ptss_resolve_toned on the host -> probe_resolve_linear's results, pixels as the (P, 4) bytes of the words (unpack_pixels10 for 10
    bits). film: (P,) LINEAR_DTYPE or SPLAT_DTYPE, or (P, 4) uint64 with film_kind; table: what probe_tone_build or Renderer.tone_build gave
    for `tone`; state: a meter's state or None; glare: None or (width, height, a glare_params, the film's pyramid)."""
    if film_kind is None:
        film_kind = FILM_SPLAT if np.asarray(film).dtype == SPLAT_DTYPE else FILM_LINEAR
    kind = _film_kind(film_kind)
    f = _rows(film, SPLAT_DTYPE if kind == FILM_SPLAT else LINEAR_DTYPE, 4, np.uint64, "film")
    P = len(f)
    first_pixel, count = _linear_range(P, first_pixel, count)
    params = params if params is not None else linear_params()
    t = _tone_table(table, tone.bits)
    width = height = 0
    g_params = pyr = None
    if glare is not None:
        width, height, g_params, g_pyramid = glare
        if P != int(width) * int(height):
            raise ValueError("film: width * height entries")
        pyr = _glare_pyramid(g_pyramid, glare_layout(width, height, g_params.levels)[1])
    ln, px, hs = _film_outputs(P, linear=linear, pixels=pixels, history=history)
    st = _meter_state(state) if state is not None else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = host_lib().ptss_probe_resolve_toned(ptr(f), kind, first_pixel, count, C.byref(params), C.byref(tone), ptr(t), ptr(st), int(width), int(height),
                                             C.byref(g_params) if g_params is not None else None, ptr(pyr), ptr(ln), ptr(px), ptr(hs))
    if rc != 0:
        raise PtssError(f"ptss_probe_resolve_toned: {rc}")
    return (ln.view(HISTORY_DTYPE).reshape(-1) if ln is not None else None, px, hs.view(HISTORY_DTYPE).reshape(-1) if hs is not None else None)


# ---- the denoiser of the two linear films (ptss_denoise_linear) ----
def denoise_linear_params(levels=5, sigma_luminance=3.0, sigma_normal=0.1, sigma_depth=4.0):
    """A ptss_denoise_linear_params; the defaults are ptss_default_denoise_linear_params' (design choices, not measurements)."""
    p = DenoiseLinearParams()
    p.structSize = C.sizeof(DenoiseLinearParams)
    p.levels, p.sigmaLuminance, p.sigmaNormal, p.sigmaDepth = int(levels), float(sigma_luminance), float(sigma_normal), float(sigma_depth)
    return p


def denoise_linear_workspace(width, height):
    """The bytes of workspace ptss_denoise_linear asks for over a width x height film (csrc/ptlindn.h workspaceLayout)."""
    return (int(width) * int(height) * DENOISE_LINEAR_WORKSPACE_BYTES + 15) & ~15


def _denoise_linear_inputs(film, film_kind, width, height, moments, features):
    """The film, its kind, the moments and the features of a denoise_linear call as plain rows."""
    f, kind = _glare_film(film, film_kind, width, height)
    m = _rows(moments, MOMENT_DTYPE, 4, np.uint64, "moments")
    ft = np.ascontiguousarray(np.asarray(features))
    ft = ft.view(np.float32).reshape(-1, 8) if ft.dtype == FEATURE_DTYPE else np.ascontiguousarray(ft, dtype=np.float32)
    if ft.ndim != 2 or ft.shape[1] != 8:
        raise ValueError("features: (N,) FEATURE_DTYPE or (N, 8) float32")
    if len(m) != len(f) or len(ft) != len(f):
        raise ValueError("moments, features: one row per film pixel")
    return f, kind, m, ft


def probe_denoise_linear(film, width, height, moments, features, params=None, denoise=None, film_kind=None, plane=False):
    """ptss_denoise_linear on the host (csrc/ptlindn.h; the specification of the device's film) -> the denoised film, (width * height,)
    LINEAR_DTYPE; with plane=True -> (film, the last plane the call computed as (width * height, 4) float32 rows {r, g, b, variance}; an
    empty pixel's variance is DENOISE_LINEAR_EMPTY). film: (P,) LINEAR_DTYPE or SPLAT_DTYPE, or (P, 4) uint64 with film_kind; moments: (P,)
    MOMENT_DTYPE; features: (P,) FEATURE_DTYPE."""
    f, kind, m, ft = _denoise_linear_inputs(film, film_kind, width, height, moments, features)
    params = params if params is not None else linear_params()
    denoise = denoise if denoise is not None else denoise_linear_params()
    out = np.zeros((len(f), 4), dtype=np.uint64)
    pl = np.zeros((len(f), 4), dtype=np.float32) if plane else None
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = host_lib().ptss_probe_denoise_linear(ptr(f), kind, int(width), int(height), ptr(m), ptr(ft), C.byref(params), C.byref(denoise), ptr(out),
                                              ptr(pl))
    if rc != 0:
        raise PtssError(f"ptss_probe_denoise_linear: {rc}")
    out = out.view(LINEAR_DTYPE).reshape(-1)
    return (out, pl) if plane else out


def probe_denoise_linear_finish(rgb, word3, film_kind="linear", params=None):
    """The finish of ptss_denoise_linear for one pixel on the host: the filtered colour rgb and the fourth word of the pixel's film entry ->
    the output row as four Python integers (r, g, b sums and samples | clamped << 32)."""
    params = params if params is not None else linear_params()
    c, out = (C.c_float * 3)(*[float(v) for v in rgb]), (C.c_ulonglong * 4)()
    rc = host_lib().ptss_probe_denoise_linear_finish(c, int(word3), _film_kind(film_kind), C.byref(params), out)
    if rc != 0:
        raise PtssError(f"ptss_probe_denoise_linear_finish: {rc}")
    return tuple(int(v) for v in out)


# ---- carrying the two linear films across a camera move (ptss_reproject_linear) ----
def reproject_linear_params(cos_normal=0.9, depth_tolerance=0.02, min_coverage=0.25, max_history=64):
    """A ptss_reproject_linear_params; the defaults are ptss_default_reproject_linear_params' (design choices, not measurements)."""
    p = ReprojectLinearParams()
    p.structSize = C.sizeof(ReprojectLinearParams)
    p.cosNormal, p.depthTolerance, p.minCoverage, p.maxHistory, p.reserved = float(cos_normal), float(depth_tolerance), float(min_coverage), int(max_history), 0
    return p


def _feature_rows(features, pixels, what):
    ft = np.ascontiguousarray(np.asarray(features))
    ft = ft.view(np.float32).reshape(-1, 8) if ft.dtype == FEATURE_DTYPE else np.ascontiguousarray(ft, dtype=np.float32)
    if ft.ndim != 2 or ft.shape[1] != 8 or len(ft) != pixels:
        raise ValueError(f"{what}: one FEATURE_DTYPE row (or 8 float32) per pixel of its film")
    return ft


def _reproject_linear_inputs(now, features_now, motion_now, prev, features_prev, film_prev, film_kind, moments_prev):
    """The buffers of a reproject_linear call as plain rows: (features_now, motion_now or None, features_prev, film_prev, kind, moments_prev
    or None)."""
    Pn, Pp = int(now.width) * int(now.height), int(prev.width) * int(prev.height)
    if Pn <= 0 or Pp <= 0:
        raise ValueError("the films' width and height must be positive")
    f, kind = _glare_film(film_prev, film_kind, prev.width, prev.height)
    fn, fp = _feature_rows(features_now, Pn, "features_now"), _feature_rows(features_prev, Pp, "features_prev")
    mo = None
    if motion_now is not None:
        mo = np.ascontiguousarray(motion_now, dtype=MOTION_DTYPE).reshape(-1)
        if len(mo) != Pn:
            raise ValueError("motion_now: one row per pixel of the new film")
    m = None
    if moments_prev is not None:
        m = _rows(moments_prev, MOMENT_DTYPE, 4, np.uint64, "moments_prev")
        if len(m) != Pp:
            raise ValueError("moments_prev: one row per pixel of the previous film")
    return fn, mo, fp, f, kind, m


def probe_reproject_linear(now, features_now, prev, features_prev, film_prev, moments_prev=None, params=None, reproject=None, film_kind=None,
                           motion_now=None):
    """ptss_reproject_linear on the host (csrc/ptlinrp.h; the specification of the device's rows) -> (the seeded film: (now.width *
    now.height,) LINEAR_DTYPE or SPLAT_DTYPE, the kind of film_prev; its moments, (P,) MOMENT_DTYPE, or None without moments_prev; the
    info, a REPROJECT_LINEAR_INFO_DTYPE record). now, prev: film_camera()s; features_*: FEATURE_DTYPE rows of each film's centre rays;
    film_prev: (P',) LINEAR_DTYPE or SPLAT_DTYPE, or (P', 4) uint64 with film_kind; params: the film's linear_params; reproject: a
    reproject_linear_params."""
    fn, mo, fp, f, kind, m = _reproject_linear_inputs(now, features_now, motion_now, prev, features_prev, film_prev, film_kind, moments_prev)
    params = params if params is not None else linear_params()
    reproject = reproject if reproject is not None else reproject_linear_params()
    out = np.zeros((len(fn), 4), dtype=np.uint64)
    mout = np.zeros((len(fn), 4), dtype=np.uint64) if m is not None else None
    info = np.zeros(1, dtype=REPROJECT_LINEAR_INFO_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = host_lib().ptss_probe_reproject_linear(C.byref(now), ptr(fn), ptr(mo), C.byref(prev), ptr(fp), ptr(f), kind, ptr(m), C.byref(params),
                                                C.byref(reproject), ptr(out), ptr(mout), ptr(info))
    if rc != 0:
        raise PtssError(f"ptss_probe_reproject_linear: {rc}")
    out = out.view(SPLAT_DTYPE if kind == FILM_SPLAT else LINEAR_DTYPE).reshape(-1)
    return out, (mout.view(MOMENT_DTYPE).reshape(-1) if mout is not None else None), info[0]


def probe_reproject_linear_finish(h, w, s2=None, film_kind="linear", params=None, reproject=None):
    """Steps 4's rounding to 6 of ptss_reproject_linear for one pixel on the host: the reprojected mean h (three floats), the
    interpolated count w and the interpolated per-sample variance s2 (None: no tap carried one) -> (the film row, the moment row), four
    Python integers each."""
    params = params if params is not None else linear_params()
    reproject = reproject if reproject is not None else reproject_linear_params()
    c, f4, m4 = (C.c_float * 3)(*[float(v) for v in h]), (C.c_ulonglong * 4)(), (C.c_ulonglong * 4)()
    rc = host_lib().ptss_probe_reproject_linear_finish(c, float(w), 0 if s2 is None else 1, 0.0 if s2 is None else float(s2),
                                                       _film_kind(film_kind), C.byref(params), C.byref(reproject), f4, m4)
    if rc != 0:
        raise PtssError(f"ptss_probe_reproject_linear_finish: {rc}")
    return tuple(int(v) for v in f4), tuple(int(v) for v in m4)


# ---- upsampling the two linear films (ptss_upsample_linear) ----
def upsample_linear_params(factor=2, sigma_normal=0.1, sigma_depth=4.0, wrap_x=False):
    """A ptss_upsample_linear_params; the defaults are ptss_default_upsample_linear_params'. wrap_x: the film is an equirect one."""
    p = UpsampleLinearParams()
    p.structSize = C.sizeof(UpsampleLinearParams)
    p.factor, p.sigmaNormal, p.sigmaDepth = int(factor), float(sigma_normal), float(sigma_depth)
    p.flags, p.reserved = (UPSAMPLE_LINEAR_WRAP_X if wrap_x else 0), 0
    return p


def _upsample_linear_inputs(film_lo, film_kind, width, height, features_lo, features_hi, upsample):
    """The buffers of an upsample_linear call as plain rows: (film, kind, features_lo, features_hi, the large film's pixels)."""
    if int(width) <= 0 or int(height) <= 0:
        raise ValueError("width and height must be positive")
    f, kind = _glare_film(film_lo, film_kind, width, height)
    fac = max(1, int(upsample.factor))
    P = int(width) * int(height) * fac * fac
    return f, kind, _feature_rows(features_lo, int(width) * int(height), "features_lo"), _feature_rows(features_hi, P, "features_hi"), P


def probe_upsample_linear(film_lo, width, height, features_lo, features_hi, params=None, upsample=None, film_kind=None, info=None):
    """ptss_upsample_linear on the host (csrc/ptlinup.h; the specification of the device's rows) -> (the large film, (factor^2 * width *
    height,) LINEAR_DTYPE; the info, an UPSAMPLE_LINEAR_INFO_DTYPE record). film_lo: (width * height,) LINEAR_DTYPE or SPLAT_DTYPE, or
    (P, 4) uint64 with film_kind; features_lo / features_hi: FEATURE_DTYPE rows of both sizes; params: the film's linear_params;
    upsample: an upsample_linear_params; info: the counters' content beforehand."""
    params = params if params is not None else linear_params()
    upsample = upsample if upsample is not None else upsample_linear_params()
    f, kind, flo, fhi, P = _upsample_linear_inputs(film_lo, film_kind, width, height, features_lo, features_hi, upsample)
    out = np.zeros((P, 4), dtype=np.uint64)
    inf = np.zeros(1, dtype=UPSAMPLE_LINEAR_INFO_DTYPE)
    if info is not None:
        inf[0] = info
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = host_lib().ptss_probe_upsample_linear(ptr(f), kind, int(width), int(height), ptr(flo), ptr(fhi), C.byref(params), C.byref(upsample), ptr(out),
                                               ptr(inf))
    if rc != 0:
        raise PtssError(f"ptss_probe_upsample_linear: {rc}")
    return out.view(LINEAR_DTYPE).reshape(-1), inf[0]


# ---- rays from surface points, the atlas, the gutter fill (ptss_generate_rays_surface / ptss_dilate_linear) ----
_SURFACE_MODES = {"normal": SURFACE_NORMAL, "cosine": SURFACE_COSINE}


def surface_params(mode="cosine", max_distance=float("inf")):
    """A ptss_surface_params. mode: "normal" (no draw) or "cosine" (two draws), or a PTSS_SURFACE_* value; max_distance: every ray's tmax."""
    p = SurfaceParams()
    p.structSize = C.sizeof(SurfaceParams)
    p.mode, p.maxDistance, p.reserved = _SURFACE_MODES.get(mode, mode), float(max_distance), 0
    return p


def surface_draws(params):
    """The uniforms a ray of ptss_generate_rays_surface takes from its stream: 0 or 2."""
    return 2 if params.mode == SURFACE_COSINE else 0


def scene_records(scene):
    """The triangles and spheres of a ptss.Scene as ((T,) TRIANGLE_DTYPE, (S,) SPHERE_DTYPE) copies."""
    d = scene.desc
    tri = np.zeros(d.numTriangles, dtype=TRIANGLE_DTYPE)
    sph = np.zeros(d.numSpheres, dtype=SPHERE_DTYPE)
    if d.numTriangles:
        C.memmove(tri.ctypes.data, d.triangles, tri.nbytes)
    if d.numSpheres:
        C.memmove(sph.ctypes.data, d.spheres, sph.nbytes)
    return tri, sph


def _surface_points(points):
    a = np.asarray(points)
    if a.dtype != SURFACE_POINT_DTYPE:
        a = np.ascontiguousarray(a, dtype=np.uint32)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("points: (P,) SURFACE_POINT_DTYPE or (P, 4) uint32")
        return a
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def _surface_buffers(points, rng, index, rays, surfels):
    """The buffers of a generate_rays_surface call as plain rows: [points, streams (a copy), rays, index or None, surfels or None]."""
    pts, s = _surface_points(points), _rng_words(rng)
    n = len(s)
    idx = _film_index(index, n)
    out = np.zeros((n, 8), dtype=np.float32) if rays is None else _rows(rays, RAY_DTYPE, 8, np.float32, "rays", copy=True)
    sur = None
    if surfels is True:
        sur = np.zeros((n, 12), dtype=np.float32)
    elif surfels is not None and surfels is not False:
        sur = _rows(surfels, HIT_DTYPE, 12, np.float32, "surfels", copy=True)
    if len(out) != n or (sur is not None and len(sur) != n):
        raise ValueError("rays and surfels: one row per stream")
    return [pts, s, out, idx, sur]


def probe_surface_rays(triangles, spheres, points, rng, params=None, first_point=0, index=None, rays=None, surfels=None):
    """ptss_generate_rays_surface on the host (csrc/ptsurface.h; the specification of the device's rays) over the caller's own records.
    triangles: (T,) TRIANGLE_DTYPE or None; spheres: (S,) SPHERE_DTYPE or None; points: (P,) SURFACE_POINT_DTYPE; rng: (N,) PATH_RNG_DTYPE
    or (N, 6) uint32 -> ((N,) RAY_DTYPE, (N,) PATH_RNG_DTYPE: the streams afterwards, (N,) HIT_DTYPE or None, entries rejected).
    rays / surfels: the buffers' content beforehand (surfels=True: zeros; None: no surfels): a rejected entry keeps it."""
    params = params if params is not None else surface_params()
    tri = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1) if triangles is not None else np.zeros(0, dtype=TRIANGLE_DTYPE)
    sph = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1) if spheres is not None else np.zeros(0, dtype=SPHERE_DTYPE)
    pts, s, out, idx, sur = _surface_buffers(points, rng, index, rays, surfels)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rejected = C.c_ulonglong(0)
    rc = host_lib().ptss_probe_surface_rays(ptr(tri), len(tri), ptr(sph), len(sph), C.byref(params), ptr(pts), len(pts), int(first_point), ptr(idx),
                                            len(s), ptr(s), ptr(out), ptr(sur), C.byref(rejected))
    if rc != 0:
        raise PtssError(f"ptss_probe_surface_rays: {rc}")
    return _records(out, RAY_DTYPE), _records(s, PATH_RNG_DTYPE), _records(sur, HIT_DTYPE), int(rejected.value)


def surface_atlas(triangles, texels_per_unit, width, min_side=1, max_side=64, first=0, count=None, fill=True):
    """ptss_surface_atlas (host only): the texels of a light map over triangles[first : first + count] -> ((K,) SURFACE_POINT_DTYPE, (K,)
    uint32 texel numbers y * width + x, the atlas height); with fill=False only (K, height): the count-only call."""
    tri = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    count = len(tri) - int(first) if count is None else int(count)
    if int(first) < 0 or count < 0 or int(first) + count > len(tri):
        raise ValueError("first + count leaves the triangles")
    height, made = C.c_int(0), C.c_size_t(0)
    args = (tri.ctypes.data_as(C.c_void_p) if len(tri) else None, int(first), count, float(texels_per_unit), int(min_side), int(max_side), int(width))
    rc = host_lib().ptss_surface_atlas(*args, None, None, 0, C.byref(height), C.byref(made))
    if rc != 0:
        raise PtssError(f"ptss_surface_atlas: {rc}")
    if not fill:
        return int(made.value), int(height.value)
    points, texels = np.zeros(made.value, dtype=SURFACE_POINT_DTYPE), np.zeros(made.value, dtype=np.uint32)
    if made.value:
        rc = host_lib().ptss_surface_atlas(*args, points.ctypes.data_as(C.c_void_p), texels.ctypes.data_as(C.c_void_p), len(points), C.byref(height),
                                           C.byref(made))
        if rc != 0 or made.value != len(points):
            raise PtssError(f"ptss_surface_atlas: {rc}")
    return points, texels, int(height.value)


def _dilate_film(film, width, height):
    f = _rows(film, LINEAR_DTYPE, 4, np.uint64, "film")
    if int(width) <= 0 or int(height) <= 0 or len(f) != int(width) * int(height):
        raise ValueError("film: width * height entries, both sides positive")
    return f


def probe_dilate_linear(film, width, height):
    """ptss_dilate_linear on the host: one gutter-fill pass over a (width * height,) LINEAR_DTYPE film -> the second film."""
    f = _dilate_film(film, width, height)
    out = np.zeros_like(f)
    rc = host_lib().ptss_probe_dilate_linear(f.ctypes.data_as(C.c_void_p), int(width), int(height), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_dilate_linear: {rc}")
    return out.view(LINEAR_DTYPE).reshape(-1)


# ---- light maps read back: the blocks of the atlas, the lookup (ptss_surface_atlas_blocks / ptss_lookup_lightmap) ----
_LIGHTMAP_FILTERS = {"nearest": LIGHTMAP_NEAREST, "bilinear": LIGHTMAP_BILINEAR}


def surface_atlas_blocks(triangles, spheres, texels_per_unit, width, min_side=1, max_side=64, first_triangle=0, num_triangles=None,
                         first_sphere=0, num_spheres=None, fill=True):
    """ptss_surface_atlas_blocks (host only): the atlas of ptss_surface_atlas with its blocks named, continued over spheres -> ((T,)
    SURFACE_BLOCK_DTYPE, (S,) SURFACE_BLOCK_DTYPE, (K,) SURFACE_POINT_DTYPE, (K,) uint32 texel numbers, the atlas height); with
    fill=False only (K, height): the count-only call. triangles / spheres: records or None."""
    tri = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1) if triangles is not None else np.zeros(0, dtype=TRIANGLE_DTYPE)
    sph = np.ascontiguousarray(spheres, dtype=SPHERE_DTYPE).reshape(-1) if spheres is not None else np.zeros(0, dtype=SPHERE_DTYPE)
    T = len(tri) - int(first_triangle) if num_triangles is None else int(num_triangles)
    S = len(sph) - int(first_sphere) if num_spheres is None else int(num_spheres)
    if min(int(first_triangle), T, int(first_sphere), S) < 0 or int(first_triangle) + T > len(tri) or int(first_sphere) + S > len(sph):
        raise ValueError("first + count leaves the triangles or the spheres")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    height, made = C.c_int(0), C.c_size_t(0)
    args = (ptr(tri), int(first_triangle), T, ptr(sph), int(first_sphere), S, float(texels_per_unit), int(min_side), int(max_side), int(width))
    rc = host_lib().ptss_surface_atlas_blocks(*args, None, None, None, None, 0, C.byref(height), C.byref(made))
    if rc != 0:
        raise PtssError(f"ptss_surface_atlas_blocks: {rc}")
    if not fill:
        return int(made.value), int(height.value)
    bt, bs = np.zeros(T, dtype=SURFACE_BLOCK_DTYPE), np.zeros(S, dtype=SURFACE_BLOCK_DTYPE)
    points, texels = np.zeros(made.value, dtype=SURFACE_POINT_DTYPE), np.zeros(made.value, dtype=np.uint32)
    rc = host_lib().ptss_surface_atlas_blocks(*args, ptr(bt), ptr(bs), ptr(points), ptr(texels), len(points), C.byref(height), C.byref(made))
    if rc != 0 or made.value != len(points):
        raise PtssError(f"ptss_surface_atlas_blocks: {rc}")
    return bt, bs, points, texels, int(height.value)


def lightmap_params(atlas_width, atlas_height, filter="bilinear", modulate=False, emission=False, first_triangle=0, num_triangle_blocks=0,
                    first_sphere=0, num_sphere_blocks=0):
    """A ptss_lightmap_params. filter: "nearest" / "bilinear" or a PTSS_LIGHTMAP_* value; the table counts are what lookup_lightmap is
    given (it fills them in from its tables when they are left 0)."""
    p = LightmapParams()
    p.structSize = C.sizeof(LightmapParams)
    p.atlasWidth, p.atlasHeight = int(atlas_width), int(atlas_height)
    p.filter = _LIGHTMAP_FILTERS.get(filter, filter)
    p.flags = (LIGHTMAP_MODULATE if modulate else 0) | (LIGHTMAP_EMISSION if emission else 0)
    p.firstTriangle, p.numTriangleBlocks, p.firstSphere, p.numSphereBlocks = int(first_triangle), int(num_triangle_blocks), int(first_sphere), int(num_sphere_blocks)
    p.reserved = 0
    return p


def scene_materials(scene):
    """The materials of a ptss.Scene as an (M,) MATERIAL_DTYPE copy."""
    d = scene.desc
    mat = np.zeros(d.numMaterials, dtype=MATERIAL_DTYPE)
    if d.numMaterials:
        C.memmove(mat.ctypes.data, d.materials, mat.nbytes)
    return mat


def _lightmap_blocks(blocks):
    if blocks is None:
        return None
    a = np.asarray(blocks)
    if a.dtype == SURFACE_BLOCK_DTYPE:
        a = np.ascontiguousarray(a).view(np.int32).reshape(-1, 4)
    a = np.ascontiguousarray(a, dtype=np.int32)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("blocks: (N,) SURFACE_BLOCK_DTYPE or (N, 4) int32")
    return a if len(a) else None


def _lightmap_buffers(hits, map, params, blocks_tri, blocks_sph, info, chain=None):
    """The buffers of a lookup_lightmap call as plain rows: [hits, map, triangle blocks or None, sphere blocks or None, out, info or None],
    and with chain rows (lookup_lightmap(chain=...)) those, one per hit, as a seventh."""
    h = _rows(hits, HIT_DTYPE, 12, np.float32, "hits")
    m = _rows(map, LINEAR_DTYPE, 4, np.uint64, "map")
    if len(m) != int(params.atlasWidth) * int(params.atlasHeight):
        raise ValueError("map: atlasWidth * atlasHeight entries")
    bt, bs = _lightmap_blocks(blocks_tri), _lightmap_blocks(blocks_sph)
    if (0 if bt is None else len(bt)) < params.numTriangleBlocks or (0 if bs is None else len(bs)) < params.numSphereBlocks:
        raise ValueError("blocks: fewer rows than params counts")
    inf = None if info is False else np.zeros(4, dtype=np.uint32)
    if info is not None and info is not False:
        inf[:] = info
    bufs = [h, m, bt, bs, np.zeros((len(h), 4), dtype=np.uint64), inf]
    if chain is not None:
        c = _rows(chain, CHAIN_DTYPE, 8, np.float32, "chain")
        if len(c) != len(h):
            raise ValueError("chain: one row per hit")
        bufs.append(c)
    return bufs


def _lightmap_counts(params, blocks_tri, blocks_sph):
    """params with table counts left at 0 filled in from the tables given (a copy)."""
    p = LightmapParams()
    C.memmove(C.byref(p), C.byref(params), C.sizeof(LightmapParams))
    if p.numTriangleBlocks == 0 and blocks_tri is not None:
        p.numTriangleBlocks = len(blocks_tri)
    if p.numSphereBlocks == 0 and blocks_sph is not None:
        p.numSphereBlocks = len(blocks_sph)
    return p


def probe_lookup_lightmap(materials, hits, map, params, blocks_tri=None, blocks_sph=None, film=None, info=None):
    """ptss_lookup_lightmap on the host (csrc/ptlightmap.h; the specification of the device's rows). materials: (M,) MATERIAL_DTYPE, a
    ptss.Scene or None; hits (N,) HIT_DTYPE; map (W H,) LINEAR_DTYPE -> ((N,) LINEAR_DTYPE, the four counts as (4,) uint32, or None with
    info=False). info: the counts' content beforehand."""
    film = film if film is not None else linear_params()
    params = _lightmap_counts(params, blocks_tri, blocks_sph)
    mat = scene_materials(materials) if isinstance(materials, Scene) else materials
    mat = np.ascontiguousarray(mat, dtype=MATERIAL_DTYPE).reshape(-1) if mat is not None else np.zeros(0, dtype=MATERIAL_DTYPE)
    h, m, bt, bs, out, inf = _lightmap_buffers(hits, map, params, blocks_tri, blocks_sph, info)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rc = host_lib().ptss_probe_lookup_lightmap(ptr(mat), len(mat), C.byref(params), C.byref(film), ptr(bt), ptr(bs), ptr(m), ptr(h), len(h), ptr(out),
                                               ptr(inf))
    if rc != 0:
        raise PtssError(f"ptss_probe_lookup_lightmap: {rc}")
    return out.view(LINEAR_DTYPE).reshape(-1), inf


def probe_lookup_lightmap_chain(materials, hits, chain, map, params, blocks_tri=None, blocks_sph=None, film=None, info=None):
    """ptss_lookup_lightmap_chain on the host (csrc/ptlightmap.h step 6; the specification of the device's rows): probe_lookup_lightmap
    with chain, (N,) CHAIN_DTYPE or (N, 8) float32, whose throughput tints every filtered row (clamped into [0, 1])."""
    film = film if film is not None else linear_params()
    params = _lightmap_counts(params, blocks_tri, blocks_sph)
    mat = scene_materials(materials) if isinstance(materials, Scene) else materials
    mat = np.ascontiguousarray(mat, dtype=MATERIAL_DTYPE).reshape(-1) if mat is not None else np.zeros(0, dtype=MATERIAL_DTYPE)
    h, m, bt, bs, out, inf, c = _lightmap_buffers(hits, map, params, blocks_tri, blocks_sph, info, chain)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
    rc = host_lib().ptss_probe_lookup_lightmap_chain(ptr(mat), len(mat), C.byref(params), C.byref(film), ptr(bt), ptr(bs), ptr(m), ptr(h), ptr(c),
                                                     len(h), ptr(out), ptr(inf))
    if rc != 0:
        raise PtssError(f"ptss_probe_lookup_lightmap_chain: {rc}")
    return out.view(LINEAR_DTYPE).reshape(-1), inf


def default_denoise_params(**overrides):
    """ptss_default_denoise_params, with levels / sigmaColor / sigmaNormal / sigmaDepth overridden by keyword."""
    p = DenoiseParams()
    _check(device_lib().ptss_default_denoise_params(C.byref(p)))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, v)
    return p


def probe_denoise(accum, inverse_ticks, features, width, height, params):
    """ptss_denoise on the host (csrc/ptdenoise.h): accum (H*W, 3) uint32, features (H*W,) FEATURE_DTYPE, row-major.
    Returns (rgba (H*W, 4) uint8, the filtered floats (H*W, 3) float32)."""
    a = np.ascontiguousarray(accum, dtype=np.uint32).reshape(-1, 3)
    f = np.ascontiguousarray(features, dtype=FEATURE_DTYPE).reshape(-1)
    if len(a) != width * height or len(f) != width * height:
        raise ValueError("accum and features must hold width * height pixels")
    rgba = np.empty((len(a), 4), dtype=np.uint8)
    flt = np.empty((len(a), 3), dtype=np.float32)
    rc = host_lib().ptss_probe_denoise(a.ctypes.data_as(_u32p), float(inverse_ticks), f.ctypes.data_as(C.c_void_p), width, height,
                                       C.byref(params), rgba.ctypes.data_as(C.c_void_p), flt.ctypes.data_as(_f32p))
    if rc != 0:
        raise PtssError(f"ptss_probe_denoise: {rc}")
    return rgba, flt


def probe_denoise_history(history, features, width, height, params):
    """ptss_denoise_history on the host: the passes of probe_denoise over the colours of `history` ((H*W,) HISTORY_DTYPE)."""
    hst = np.ascontiguousarray(history, dtype=HISTORY_DTYPE).reshape(-1)
    f = np.ascontiguousarray(features, dtype=FEATURE_DTYPE).reshape(-1)
    if len(hst) != width * height or len(f) != width * height:
        raise ValueError("history and features must hold width * height pixels")
    rgba = np.empty((len(hst), 4), dtype=np.uint8)
    flt = np.empty((len(hst), 3), dtype=np.float32)
    rc = host_lib().ptss_probe_denoise_history(hst.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), width, height, C.byref(params),
                                               rgba.ctypes.data_as(C.c_void_p), flt.ctypes.data_as(_f32p))
    if rc != 0:
        raise PtssError(f"ptss_probe_denoise_history: {rc}")
    return rgba, flt


def default_upsample_params(**overrides):
    """ptss_default_upsample_params, with factor / sigmaNormal / sigmaDepth overridden by keyword."""
    p = UpsampleParams()
    _check(device_lib().ptss_default_upsample_params(C.byref(p)))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, v)
    return p


UPSAMPLE_MAX_FACTOR = 4   # PTSS_UPSAMPLE_MAX_FACTOR (include/ptss_types.h)


def _upsample_factor(factor):
    """The factor of features_scaled() / upsample(), refused here before any buffer is sized from it."""
    factor = int(factor)
    if not 1 <= factor <= UPSAMPLE_MAX_FACTOR:
        raise ValueError(f"factor must be in 1..{UPSAMPLE_MAX_FACTOR}")
    return factor


def probe_upsample_axis(X, factor):
    """csrc/ptupsample.h axisOf on the host: (x0, k, fx) of hi-res coordinate X at `factor`."""
    x0, k, fx = C.c_int(), C.c_int(), C.c_float()
    rc = host_lib().ptss_probe_upsample_axis(int(X), int(factor), C.byref(x0), C.byref(k), C.byref(fx))
    if rc != 0:
        raise PtssError(f"ptss_probe_upsample_axis: {rc}")
    return x0.value, k.value, fx.value


def probe_upsample(lo_rgba, features_lo, width, height, features_hi, params):
    """ptss_upsample on the host (csrc/ptupsample.h): lo_rgba (H*W, 4) uint8, features_lo (H*W,) and features_hi (f*H*f*W,)
    FEATURE_DTYPE, row-major. Returns (rgba (f*H*f*W, 4) uint8, floats (f*H*f*W,) HISTORY_DTYPE: the value before the byte
    conversion and the taps' weight sum)."""
    a = np.ascontiguousarray(lo_rgba, dtype=np.uint8).reshape(-1, 4)
    fl = np.ascontiguousarray(features_lo, dtype=FEATURE_DTYPE).reshape(-1)
    fh = np.ascontiguousarray(features_hi, dtype=FEATURE_DTYPE).reshape(-1)
    n_hi = width * height * params.factor * params.factor
    if len(a) != width * height or len(fl) != width * height or len(fh) != n_hi:
        raise ValueError("lo_rgba and features_lo must hold width * height pixels, features_hi factor^2 times as many")
    rgba = np.empty((n_hi, 4), dtype=np.uint8)
    flt = np.empty(n_hi, dtype=HISTORY_DTYPE)
    rc = host_lib().ptss_probe_upsample(a.ctypes.data_as(C.c_void_p), fl.ctypes.data_as(C.c_void_p), width, height, fh.ctypes.data_as(C.c_void_p),
                                        C.byref(params), rgba.ctypes.data_as(C.c_void_p), flt.ctypes.data_as(_f32p))
    if rc != 0:
        raise PtssError(f"ptss_probe_upsample: {rc}")
    return rgba, flt


def default_reproject_params(**overrides):
    """ptss_default_reproject_params, with cosNormal / depthTolerance / maxHistory / minCoverage overridden by keyword."""
    p = ReprojectParams()
    _check(device_lib().ptss_default_reproject_params(C.byref(p)))
    for k, v in overrides.items():
        if v is not None:
            setattr(p, k, v)
    return p


def probe_reproject(accum, inverse_ticks, n, camera_now, camera_prev, width, height, features_now, features_prev, history_prev, params=None):
    """ptss_reproject on the host (csrc/ptreproject.h): accum (H*W, 3) uint32 with n samples per pixel behind it, the features of
    both cameras and the previous history row-major; history_prev None = no history. Returns (H*W,) HISTORY_DTYPE."""
    a = np.ascontiguousarray(accum, dtype=np.uint32).reshape(-1, 3)
    fn = np.ascontiguousarray(features_now, dtype=FEATURE_DTYPE).reshape(-1)
    if len(a) != width * height or len(fn) != width * height:
        raise ValueError("accum and features_now must hold width * height pixels")
    fp = hp = None
    if history_prev is not None:
        fp = np.ascontiguousarray(features_prev, dtype=FEATURE_DTYPE).reshape(-1)
        hp = np.ascontiguousarray(history_prev, dtype=HISTORY_DTYPE).reshape(-1)
        if len(fp) != width * height or len(hp) != width * height:
            raise ValueError("features_prev and history_prev must hold width * height pixels")
    out = np.empty(len(a), dtype=HISTORY_DTYPE)
    rc = host_lib().ptss_probe_reproject(a.ctypes.data_as(_u32p), float(inverse_ticks), int(n), C.byref(camera_now),
                                         C.byref(camera_prev) if camera_prev is not None else None, width, height,
                                         fn.ctypes.data_as(C.c_void_p), fp.ctypes.data_as(C.c_void_p) if fp is not None else None,
                                         hp.ctypes.data_as(C.c_void_p) if hp is not None else None,
                                         C.byref(params if params is not None else default_reproject_params()), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_reproject: {rc}")
    return out


def probe_reproject_motion(accum, inverse_ticks, n, camera_now, camera_prev, width, height, features_now, motion_now, features_prev,
                           history_prev, params=None):
    """ptss_reproject_motion on the host: probe_reproject with the world point of every hit pixel taken from motion_now, (H*W,)
    MOTION_DTYPE. Returns (H*W,) HISTORY_DTYPE."""
    a = np.ascontiguousarray(accum, dtype=np.uint32).reshape(-1, 3)
    fn = np.ascontiguousarray(features_now, dtype=FEATURE_DTYPE).reshape(-1)
    mn = np.ascontiguousarray(motion_now, dtype=MOTION_DTYPE).reshape(-1)
    if len(a) != width * height or len(fn) != width * height or len(mn) != width * height:
        raise ValueError("accum, features_now and motion_now must hold width * height pixels")
    fp = hp = None
    if history_prev is not None:
        fp = np.ascontiguousarray(features_prev, dtype=FEATURE_DTYPE).reshape(-1)
        hp = np.ascontiguousarray(history_prev, dtype=HISTORY_DTYPE).reshape(-1)
        if len(fp) != width * height or len(hp) != width * height:
            raise ValueError("features_prev and history_prev must hold width * height pixels")
    out = np.empty(len(a), dtype=HISTORY_DTYPE)
    rc = host_lib().ptss_probe_reproject_motion(a.ctypes.data_as(_u32p), float(inverse_ticks), int(n), C.byref(camera_now),
                                                C.byref(camera_prev) if camera_prev is not None else None, width, height,
                                                fn.ctypes.data_as(C.c_void_p), mn.ctypes.data_as(C.c_void_p),
                                                fp.ctypes.data_as(C.c_void_p) if fp is not None else None,
                                                hp.ctypes.data_as(C.c_void_p) if hp is not None else None,
                                                C.byref(params if params is not None else default_reproject_params()),
                                                out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_reproject_motion: {rc}")
    return out


def probe_motion(rays, hits, prev_triangles=None, first=0, num_triangles=0):
    """ptss_render_features_motion's rows on the host (csrc/ptmotion.h): rays (N, 8) float32 or (N,) RAY_DTYPE, hits (N,) HIT_DTYPE
    (what intersect() returned for them), prev_triangles an (n,) TRIANGLE_DTYPE array — the previous pose of triangles first ..
    first + n - 1 of a scene of num_triangles — or None: nothing moved. Returns (N,) MOTION_DTYPE."""
    r = np.ascontiguousarray(rays)
    r = (r.view(np.float32) if r.dtype == RAY_DTYPE else r.astype(np.float32, copy=False)).reshape(-1, 8)
    r = np.ascontiguousarray(r)
    h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
    if len(r) != len(h):
        raise ValueError("one hit per ray")
    t = np.ascontiguousarray(prev_triangles, dtype=TRIANGLE_DTYPE).reshape(-1) if prev_triangles is not None else None
    out = np.empty(len(h), dtype=MOTION_DTYPE)
    rc = host_lib().ptss_probe_motion(r.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), len(h),
                                      t.ctypes.data_as(C.c_void_p) if t is not None and len(t) else None, int(first),
                                      len(t) if t is not None else 0, int(num_triangles), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_motion: {rc}")
    return out


SPECULAR_CLASSES = ("terminal", "transmit", "mirror")   # csrc/ptspecular.h Class 0, 1, 2


def _material_table(materials):
    """(pointer, count) of a materials table: a scene description (anything with .materials and .numMaterials) or a sequence of Material."""
    if hasattr(materials, "numMaterials"):
        return C.cast(materials.materials, C.c_void_p), int(materials.numMaterials), materials
    arr = (Material * max(len(materials), 1))(*materials)
    return C.cast(arr, C.c_void_p), len(materials), arr


def specular_class(material):
    """The class csrc/ptspecular.h gives a Material: "terminal", "transmit" or "mirror"."""
    return SPECULAR_CLASSES[host_lib().ptss_probe_specular_class(C.byref(material))]


def probe_specular_step(rays, hits, materials):
    """One step of ptss_render_features_specular's chain on the host (csrc/ptspecular.h): rays (N, 8) float32 or (N,) RAY_DTYPE, hits
    (N,) HIT_DTYPE (what intersect() returned for them), materials a scene description (scene.desc) or a sequence of Material.
    Returns (next (N, 8) float32 — the continued rays, tmax +inf; the rows that do not continue are the input rows, untouched —,
    follows (N,) bool)."""
    r = np.ascontiguousarray(rays)
    r = (r.view(np.float32) if r.dtype == RAY_DTYPE else r.astype(np.float32, copy=False)).reshape(-1, 8)
    r = np.ascontiguousarray(r)
    h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
    if len(r) != len(h):
        raise ValueError("one hit per ray")
    ptr, count, keep = _material_table(materials)
    nxt = r.copy()
    follows = np.zeros(len(h), dtype=np.int32)
    rc = host_lib().ptss_probe_specular_step(r.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), len(h), ptr, count,
                                             nxt.ctypes.data_as(C.c_void_p), follows.ctypes.data_as(C.POINTER(C.c_int)))
    del keep
    if rc != 0:
        raise PtssError(f"ptss_probe_specular_step: {rc}")
    return nxt, follows != 0


def probe_specular_link(rays, hits, materials):
    """One link of ptss_intersect_chain on the host (csrc/ptspecular.h): probe_specular_step's arguments and its very next and follows,
    plus factors (N, 3) float32 — the factor by which each followed link multiplies the radiance; rows that do not follow hold zeros.
    Returns (next, follows, factors)."""
    r = np.ascontiguousarray(rays)
    r = (r.view(np.float32) if r.dtype == RAY_DTYPE else r.astype(np.float32, copy=False)).reshape(-1, 8)
    r = np.ascontiguousarray(r)
    h = np.ascontiguousarray(hits, dtype=HIT_DTYPE).reshape(-1)
    if len(r) != len(h):
        raise ValueError("one hit per ray")
    ptr, count, keep = _material_table(materials)
    nxt = r.copy()
    follows = np.zeros(len(h), dtype=np.int32)
    factors = np.zeros((len(h), 3), dtype=np.float32)
    rc = host_lib().ptss_probe_specular_link(r.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), len(h), ptr, count,
                                             nxt.ctypes.data_as(C.c_void_p), follows.ctypes.data_as(C.POINTER(C.c_int)),
                                             factors.ctypes.data_as(C.c_void_p))
    del keep
    if rc != 0:
        raise PtssError(f"ptss_probe_specular_link: {rc}")
    return nxt, follows != 0, factors


def make_rays(origins, directions, tmax=float("inf")):
    """(N, 8) float32 query rays {origin, tmax, direction, 0} (include/ptss_types.h ptss_ray_query); tmax: scalar or (N,)."""
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape")
    out = np.zeros((o.shape[0], 8), dtype=np.float32)
    out[:, 0:3], out[:, 4:7] = o, d
    out[:, 3] = np.broadcast_to(np.asarray(tmax, dtype=np.float32), (o.shape[0],))
    return out


def camera_ray(cam, width, height, x, y, jitter=(0.5, 0.5)):
    """ptss_camera_ray: the eye ray of pixel (x, y) through (x + jx, y + jy), as an (8,) float32 row."""
    q = RayQuery()
    rc = host_lib().ptss_camera_ray(C.byref(cam), width, height, x, y, jitter[0], jitter[1], C.byref(q))
    if rc != 0:
        raise PtssError(f"ptss_camera_ray: {rc}")
    return np.frombuffer(bytes(q), dtype=np.float32).copy()


def camera_rays(cam, width, height, jitter=(0.5, 0.5)):
    """The eye rays of every pixel of a width x height frame, row-major (index y * width + x), as (width * height, 8) float32."""
    out = np.empty((width * height, 8), dtype=np.float32)
    q = RayQuery()
    fn, jx, jy, ref_cam, ref_q = host_lib().ptss_camera_ray, C.c_float(jitter[0]), C.c_float(jitter[1]), C.byref(cam), C.byref(q)
    buf = (C.c_float * 8).from_buffer(q)
    for y in range(height):
        for x in range(width):
            if fn(ref_cam, width, height, x, y, jx, jy, ref_q) != 0:
                raise PtssError("ptss_camera_ray failed")
            out[y * width + x] = buf
    return out


def probe_strip_masks(scene, cam, width, height, band_rows=8, rank=0, world=1):
    """ptss_probe_strip_masks: (masks, enabled, tri_pos) — the uint64 word of every 64-pixel strip of the rank's local pixel plane
    (bits 0-31 stored spheres, 32-63 stored triangles), whether ptss_generate_frame would use them, and the stored position of each
    triangle (csrc/ptstrip.h on the host)."""
    desc = scene.desc if hasattr(scene, "desc") else scene
    rows = len(tile_rows(height, band_rows, rank, world))
    cap = max((width * rows + 255) // 256, 1) * 4
    masks = np.zeros(cap, dtype=np.uint64)
    tri_pos = np.zeros(max(int(desc.numTriangles), 1), dtype=np.int32)
    n, on = C.c_size_t(), C.c_int()
    rc = host_lib().ptss_probe_strip_masks(C.byref(desc), C.byref(cam), width, height, band_rows, rank, world, masks.ctypes.data_as(C.c_void_p), cap,
                                           C.byref(n), C.byref(on), tri_pos.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise PtssError(f"ptss_probe_strip_masks: {rc}")
    return masks[:n.value], bool(on.value), tri_pos[:int(desc.numTriangles)]


def tile_rows(height, band_rows, rank, world):
    n = host_lib().ptss_tile_rows(height, band_rows, rank, world, None, 0)
    if n < 0:
        raise PtssError("bad tile spec")
    rows = (C.c_int * max(n, 1))()
    host_lib().ptss_tile_rows(height, band_rows, rank, world, rows, n)
    return np.array(rows[:n], dtype=np.int64)


def write_tga(path, rgba_hw4):
    a = np.ascontiguousarray(rgba_hw4, dtype=np.uint8)
    h, w = a.shape[:2]
    rc = host_lib().ptss_write_tga(path.encode(), a.ctypes.data_as(C.c_void_p), w, h)
    if rc != 0:
        raise PtssError(f"write_tga failed ({rc})")


class Renderer:
    """One ptss_context: the reference's ProgramData + device buffers, driven like generateFrame."""

    def __init__(self, scene, width, height, max_iterations=15, seed=0x5EED, device=0, tile_rank=0, tile_world=1,
                 band_rows=8, sync_each_frame=True, float_accumulator=False, time_kernels=False, samples_per_pass=1,
                 every_sphere_loop=False, frame_lanes=0, lanes_free_run=False, one_launch_frames=0):
        L = device_lib()
        cfg = RenderConfig()
        _check(L.ptss_default_config(C.byref(cfg)))
        cfg.width, cfg.height = width, height
        cfg.seed = seed
        cfg.maxIterations = max_iterations
        cfg.device = device
        cfg.tileRank, cfg.tileWorld, cfg.bandRows = tile_rank, tile_world, band_rows
        cfg.syncEachFrame = 1 if sync_each_frame else 0
        cfg.floatAccumulator = 1 if float_accumulator else 0
        cfg.timeKernels = 1 if time_kernels else 0
        cfg.samplesPerPass = samples_per_pass
        cfg.everySphereLoop = 1 if every_sphere_loop else 0
        cfg.frameLanes = frame_lanes
        cfg.lanesFreeRun = 1 if lanes_free_run else 0
        cfg.oneLaunchFrames = one_launch_frames
        self.cfg = cfg
        self._scene = scene  # keep the arrays alive during create
        self._ctx = C.c_void_p()
        _check(L.ptss_create(C.byref(scene.desc), C.byref(cfg), C.byref(self._ctx)))
        n = C.c_size_t()
        _check(L.ptss_local_pixels(self._ctx, C.byref(n)))
        self.local_pixels = n.value
        self.width, self.height = width, height
        self.local_rows = self.local_pixels // width
        self._own_pixels = None
        self._buffers = {}            # device buffers of features() / denoise(), by name; freed by close()
        self._have_features = False   # the features buffer holds the CURRENT camera's features
        self._have_scaled = set()     # factors whose features_scaled buffer holds the current camera's (and scene's) features
        self.ticks = 1  # GPUAnimBitmap::idle_func's static counter starts at 1 (CudaUtils.h:146)

    def close(self):
        if self._ctx:
            L = device_lib()
            if self._own_pixels:
                L.ptss_free_pixels(self._ctx, self._own_pixels)
                self._own_pixels = None
            for p in self._buffers.values():
                _hip_lib().hipFree(p)
            self._buffers = {}
            L.ptss_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- plumbing -------------------------------------------------------------------------------
    def pixels_devptr(self):
        if self._own_pixels is None:
            p = C.c_void_p()
            _check(device_lib().ptss_alloc_pixels(self._ctx, C.byref(p)))
            self._own_pixels = p
        return self._own_pixels

    def set_stream(self, raw_stream):
        _check(device_lib().ptss_set_stream(self._ctx, C.c_void_p(raw_stream)))

    def bind_accumulator(self, devptr):
        _check(device_lib().ptss_bind_accumulator(self._ctx, C.c_void_p(devptr)))

    def rows(self):
        cnt = C.c_int()
        rows = (C.c_int * max(self.local_rows, 1))()
        _check(device_lib().ptss_local_rows(self._ctx, rows, self.local_rows, C.byref(cnt)))
        return np.array(rows[:cnt.value], dtype=np.int64)

    # --- the frame callback ---------------------------------------------------------------------
    def generate_frame(self, dev_pixels=None, ticks=None):
        """generateFrame(pixels, dataBlock, ticks). With no arguments behaves like one GLUT idle tick."""
        if ticks is None:
            ticks = self.ticks
            self.ticks += 1
        if dev_pixels is None:
            dev_pixels = self.pixels_devptr()
        elif isinstance(dev_pixels, int):
            dev_pixels = C.c_void_p(dev_pixels)
        _check(device_lib().ptss_generate_frame(self._ctx, dev_pixels, ticks))

    def set_camera(self, cam):
        _check(device_lib().ptss_set_camera(self._ctx, C.byref(cam)))
        self._have_features = False   # denoise(features=None) renders them again for the new camera
        self._have_scaled = set()

    def get_camera(self):
        cam = Camera()
        _check(device_lib().ptss_get_camera(self._ctx, C.byref(cam)))
        return cam

    def request_reset(self):
        _check(device_lib().ptss_request_reset(self._ctx))

    def set_mode(self, use_path_tracer):
        _check(device_lib().ptss_set_mode(self._ctx, 1 if use_path_tracer else 0))

    def set_max_iterations(self, n):
        _check(device_lib().ptss_set_max_iterations(self._ctx, n))

    def synchronize(self):
        _check(device_lib().ptss_synchronize(self._ctx))

    # --- read-back ------------------------------------------------------------------------------
    def accumulator(self):
        out = np.empty((self.local_pixels, 3), dtype=np.uint32)
        _check(device_lib().ptss_read_accumulator(self._ctx, out.ctypes.data_as(_u32p), out.size))
        return out

    def float_accumulator(self):
        out = np.empty((self.local_pixels, 3), dtype=np.float32)
        _check(device_lib().ptss_read_float_accumulator(self._ctx, out.ctypes.data_as(_f32p), out.size))
        return out

    def pixels(self, dev_pixels=None):
        if dev_pixels is None:
            dev_pixels = self.pixels_devptr()
        elif isinstance(dev_pixels, int):
            dev_pixels = C.c_void_p(dev_pixels)
        out = np.empty((self.local_pixels, 4), dtype=np.uint8)
        _check(device_lib().ptss_read_pixels(self._ctx, dev_pixels, out.ctypes.data_as(C.c_void_p), self.local_pixels))
        return out

    def rng_state(self, local_pixel, lane=0):
        out = np.empty(6, dtype=np.uint32)
        _check(device_lib().ptss_read_rng_state_lane(self._ctx, local_pixel, lane, out.ctypes.data_as(_u32p)))
        return out

    def last_pass_ms(self):
        v = C.c_float()
        _check(device_lib().ptss_last_pass_ms(self._ctx, C.byref(v)))
        return v.value

    def live_counts(self):
        out = (C.c_uint32 * 65)()
        n = C.c_int()
        _check(device_lib().ptss_live_counts(self._ctx, out, 65, C.byref(n)))
        return np.array(out[:n.value], dtype=np.uint32)

    def total_ray_bounces(self):
        v = C.c_ulonglong()
        _check(device_lib().ptss_total_ray_bounces(self._ctx, C.byref(v)))
        return v.value

    @property
    def one_launch_frames(self):
        """True when this context traces a frame with ONE launch (cfg.oneLaunchFrames resolved for the current scene image)."""
        v = C.c_int()
        _check(device_lib().ptss_one_launch_frames(self._ctx, C.byref(v)))
        return bool(v.value)

    @property
    def frame_lanes(self):
        v = C.c_int()
        _check(device_lib().ptss_frame_lanes(self._ctx, C.byref(v)))
        return v.value

    def guard_timeouts(self):
        v = C.c_uint()
        _check(device_lib().ptss_guard_timeouts(self._ctx, C.byref(v)))
        return v.value

    def launched_kernels(self):
        """The kernel instantiations this context has launched since it was created, as all_kernels() names them."""
        v = C.c_ulonglong()
        _check(device_lib().ptss_launched_kernels(self._ctx, C.byref(v)))
        return decode_launched_kernels(v.value)

    def guard_flags(self):
        """ptss_guard_flags: the range guards the current scene's constants satisfy (bit 0 light powers, 1 refraction indices,
        2 Phong exponents), decided at creation and at every set_scene."""
        v = C.c_uint()
        _check(device_lib().ptss_guard_flags(self._ctx, C.byref(v)))
        return v.value

    # --- scene updates (ptss_set_scene / ptss_update_triangles / ptss_reseed) -------------------------------------
    def set_scene(self, scene):
        """ptss_set_scene: replaces the whole scene (a ptss.Scene or anything with a .desc); the context keeps its pools, random
        streams, camera and counters and starts a new accumulation."""
        _check(device_lib().ptss_set_scene(self._ctx, C.byref(scene.desc)))
        self._scene = scene
        self._have_features = False
        self._have_scaled = set()

    def update_triangles(self, triangles, first=0, stream=None):
        """ptss_update_triangles: new vertices and normals for the triangles with original indices first .. first + n - 1.
        triangles: an (n,) TRIANGLE_DTYPE array (uploaded; the call returns once the update has run), or a contiguous float32
        device tensor of n x 19 words in that layout, whose pointer is passed — asynchronous on `stream` (a raw stream handle;
        default: the tensor's current torch stream)."""
        L = device_lib()
        if _is_torch(triangles):
            if triangles.dtype != _torch().float32 or not triangles.is_contiguous() or not triangles.is_cuda or triangles.numel() % 19:
                raise ValueError("triangles: a contiguous float32 device tensor of n x 19 words")
            if stream is None:
                stream = _stream_of(_torch(), triangles.device)
            _check(L.ptss_update_triangles(self._ctx, C.c_void_p(triangles.data_ptr()), first, triangles.numel() // 19, C.c_void_p(stream)))
        else:
            a = np.ascontiguousarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
            d = self._device_buffer_at_least("triangles_upload", a.nbytes) if len(a) else None
            if len(a):   # (every earlier upload has been consumed: this path returns only once its update has run)
                _hip_check(_hip_lib().hipMemcpy(d, a.ctypes.data, a.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
            _check(L.ptss_update_triangles(self._ctx, d, first, len(a), C.c_void_p(stream) if stream else None))
            if len(a):
                if stream:
                    _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
                self.synchronize()
        self._have_features = False
        self._have_scaled = set()

    def resort_triangles(self, stream=None):
        """ptss_resort_triangles: the kd order of a live mesh image rebuilt on the device from its current vertices (behind
        update_triangles, before the next frame). Asynchronous on `stream` (a raw stream handle; default: the context's stream).
        No reset: accumulation continues. Images without a kd order: nothing happens."""
        _check(device_lib().ptss_resort_triangles(self._ctx, C.c_void_p(stream) if stream else None))

    def resort_launches(self):
        """ptss_resort_launches: resort_triangles calls that launched, since the context was created."""
        return self._counters("ptss_resort_launches", 1)

    def strip_words(self):
        """ptss_read_strip_words: (words, enabled) — the uint64 strip words bounce 0 of the latest frame read (csrc/ptstrip.h), and whether it did."""
        cap = max((self.local_pixels + 255) // 256, 1) * 4
        words = np.zeros(cap, dtype=np.uint64)
        n, on = C.c_size_t(), C.c_int()
        _check(device_lib().ptss_read_strip_words(self._ctx, words.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(on)))
        return words[:n.value], bool(on.value)

    def reseed(self, seed):
        """ptss_reseed: the random streams of a context created with this seed, and a reset."""
        _check(device_lib().ptss_reseed(self._ctx, seed))

    def update_rejected(self):
        """Records update_triangles has refused (a vertex not finite or beyond 2^40) since the context was created."""
        return self._counters("ptss_update_rejected", 1)

    def triangle_bounds(self):
        """ptss_read_triangle_bounds: (leaves + groups, 12) float32, the leaves' bounds first (mesh images only)."""
        leaves = self.triangle_leaves()
        out = np.empty((leaves + (leaves + 15) // 16, 12), dtype=np.float32)
        _check(device_lib().ptss_read_triangle_bounds(self._ctx, out.ctypes.data_as(_f32p), out.size))
        return out

    def triangle_positions(self, count):
        """ptss_read_triangle_positions: the stored position of each of the scene's `count` original triangle indices."""
        out = np.empty(count, dtype=np.int32)
        _check(device_lib().ptss_read_triangle_positions(self._ctx, out.ctypes.data_as(C.POINTER(C.c_int)), out.size))
        return out

    def _counters(self, name, k):
        """The k 64-bit counters the library's `name` reads: one as an int, several as a tuple."""
        out = (C.c_ulonglong * k)()
        _check(getattr(device_lib(), name)(self._ctx, out))
        return int(out[0]) if k == 1 else tuple(int(v) for v in out)

    # --- batched ray queries (ptss_intersect / ptss_occluded) ------------------------------------------
    def intersect(self, rays):
        """Closest hits. rays: (N, 8) float32 or an (N,) RAY_DTYPE array -> (N,) HIT_DTYPE array; or a contiguous (N, 8) float32
        torch tensor on the context's device -> (N, 12) float32 tensor (bit-viewable as HIT_DTYPE), on the current stream."""
        return self._query(rays, any_hit=False)

    def occluded(self, rays):
        """Occlusion verdicts (1 = some primitive accepts within tmax). numpy in -> (N,) uint32; torch in -> (N,) int32 tensor."""
        return self._query(rays, any_hit=True)

    def _query(self, rays, any_hit):
        L = device_lib()
        fn = L.ptss_occluded if any_hit else L.ptss_intersect

        def arrays():
            a = _query_rays(rays)
            return [a, np.empty(len(a), dtype=np.uint32 if any_hit else HIT_DTYPE)]

        # without rays the array path calls nothing: that is where `d` holds None
        return self._device_call([("rays", rays, "float32", 8, None, None), ("out", None, *(("int32", 0) if any_hit else ("float32", 12)), "rays", "empty")],
                                 lambda d, n, stream: fn(self._ctx, d[0], d[1], n["rays"], stream) if d[0] is not None else 0,
                                 arrays, read=(1,), null=lambda n: n["rays"] == 0, result=lambda a: a[1], returns="out", texts=_QUERY_TEXTS)

    def intersect_chain(self, rays, max_steps, schedule="lane", max_workgroups=0, chain=True):
        """ptss_intersect_chain: intersect() carried through mirrors and glass for at most max_steps links (0 .. 8; csrc/ptspecular.h).
        schedule: "lane" / "refill" or a CHAIN_* value, or None for the library's default (options NULL); max_workgroups: the refill
        grid's cap. The refill calls of one context are ordered by the caller.
        numpy: rays (N, 8) float32 or (N,) RAY_DTYPE -> ((N,) HIT_DTYPE: the hit of the last link's ray, (N,) CHAIN_DTYPE or None with
        chain=False: dev_chain NULL). torch: a contiguous (N, 8) float32 device tensor -> (hits (N, 12) float32, chain (N, 8) float32 or
        None), on the current stream; chain may also be an (N, 8) float32 tensor to write."""
        L = device_lib()
        options = chain_options(schedule, max_workgroups) if schedule is not None else None
        wanted = chain is not False and chain is not None
        rows = chain if wanted and chain is not True else None

        def arrays():
            a = _query_rays(rays)
            return [a, np.empty(len(a), dtype=HIT_DTYPE), np.empty(len(a), dtype=CHAIN_DTYPE) if wanted else None]

        bufs = [("rays", rays, "float32", 8, None, None), ("hits", None, "float32", 12, "rays", "empty"),
                ("chain", rows, "float32", 8, "rays", "empty" if wanted else "null")]
        call = lambda d, n, stream: L.ptss_intersect_chain(self._ctx, d[0], n["rays"], int(max_steps), C.byref(options) if options is not None else None,
                                                           d[1], d[2], stream)
        if _is_torch(rays):   # two tensors come back: the body returns one, the other is made here
            torch = sys.modules["torch"]
            if wanted and rows is None:
                rows = torch.empty((rays.shape[0] if rays.dim() == 2 else 0, 8), dtype=torch.float32, device=rays.device)
                bufs[2] = ("chain", rows, "float32", 8, "rays", None)
            return self._device_call(bufs, call, arrays, returns="hits", texts=None), rows
        return self._device_call(bufs, call, arrays, read=(1, 2), null=lambda n: n["rays"] == 0, result=lambda a: (a[1], a[2]))

    def chain_launches(self):
        """ptss_chain_launches: (ptss_intersect_chain launches with one lane per ray, with the refill schedule)."""
        return self._counters("ptss_chain_launches", 2)

    # --- batched path queries (ptss_seed_path_rng / ptss_trace_paths) ------------------------------------
    def seed_path_rng(self, n, seed, first_sequence=0, skip=0, device=None):
        """ptss_seed_path_rng: n XORWOW states, entry i that of curand_init(seed, first_sequence + i, 0) after `skip` draws ->
        (n,) PATH_RNG_DTYPE. device: a torch device (or True for the context's) -> an (n, 6) int32 tensor on it instead, seeded on
        the current torch stream and left there for trace_paths."""
        L = device_lib()
        n = int(n)
        seed_into = lambda d, stream: _check(L.ptss_seed_path_rng(self._ctx, d, n, seed, first_sequence, skip, stream))
        if device is not None:   # no tensor comes in to take a device from: this path is the wrapper's own
            torch = _torch()
            if torch is None:
                raise ValueError("device=...: import torch first")
            dev = torch.device("cuda", self.cfg.device) if device is True else torch.device(device)
            out = torch.empty((n, 6), dtype=torch.int32, device=dev)
            seed_into(C.c_void_p(out.data_ptr()) if n else None, C.c_void_p(_stream_of(torch, dev)))
            return out
        out = np.empty(n, dtype=PATH_RNG_DTYPE)
        if n == 0:
            seed_into(None, None)
        else:
            self._round_trip([out], lambda d: seed_into(d[0], None), read=(0,))
        return out

    def trace_paths(self, rays, rng, max_iterations, schedule=None, max_workgroups=0):
        """ptss_trace_paths: radiance along the caller's rays. schedule: None (ptss_trace_paths itself) or PATHS_LANE_PER_RAY /
        PATHS_REFILL / their names (ptss_trace_paths_opt with max_workgroups; the refill calls of one context are ordered by the caller).
        rays: (N, 8) float32 or (N,) RAY_DTYPE (tmax is ignored); rng: (N,)
        PATH_RNG_DTYPE or (N, 6) uint32, one stream per ray -> ((N,) PATH_RESULT_DTYPE, (N,) PATH_RNG_DTYPE: the streams afterwards,
        to be handed to the next call). Or torch: rays a contiguous (N, 8) float32 device tensor and rng a contiguous (N, 6) int32
        tensor on the same device, which is UPDATED IN PLACE -> an (N, 4) float32 tensor (radiance; column 3 holds the bits of
        `bounces`), on the current stream."""
        L = device_lib()
        if schedule is None:
            call = lambda d, n, stream: L.ptss_trace_paths(self._ctx, d[0], d[1], d[2], n["rays"], int(max_iterations), stream)
        else:
            options = path_options(schedule, max_workgroups)
            call = lambda d, n, stream: L.ptss_trace_paths_opt(self._ctx, d[0], d[1], d[2], n["rays"], int(max_iterations), C.byref(options), stream)

        def arrays():
            a = _query_rays(rays)
            s = np.asarray(rng)
            if s.dtype == PATH_RNG_DTYPE:
                s = np.ascontiguousarray(s).view(np.uint32).reshape(-1, 6)
            s = np.array(s, dtype=np.uint32, order="C")   # a copy: the streams afterwards are read back into it
            if s.shape != (len(a), 6):
                raise ValueError("rng: (N,) PATH_RNG_DTYPE or (N, 6) uint32, one state per ray")
            return [a, s, np.empty(len(a), dtype=PATH_RESULT_DTYPE)]

        return self._device_call([("rays", rays, "float32", 8, None, None), ("rng", rng, "int32", 6, "rays", None), ("out", None, "float32", 4, "rays", "empty")],
                                 call, arrays, read=(1, 2), null=lambda n: n["rays"] == 0, result=lambda a: (a[2], _records(a[1], PATH_RNG_DTYPE)),
                                 returns="out", texts=_QUERY_TEXTS)

    def path_launches(self):
        """ptss_path_launches: (ptss_trace_paths launches with the scene image read in place, with it staged in LDS)."""
        return self._counters("ptss_path_launches", 2)

    def path_refill_stats(self):
        """ptss_path_refill_stats: (refill launches with the scene image read in place, staged in LDS, wave iterations, lane iterations,
        dequeues) since the context was created; synchronises with the stream of the latest refill call."""
        return self._counters("ptss_path_refill_stats", 5)

    # --- the film of a path query (ptss_generate_rays / ptss_accumulate_paths / ptss_ray_features) ------------------
    def _round_trip(self, arrays, call, read):
        """Uploads `arrays` (None entries stay NULL), runs call(device pointers) on the context's stream, waits, downloads those at `read`."""
        H = _hip_lib()
        _hip_check(H.hipSetDevice(self.cfg.device), "hipSetDevice")
        bufs = [C.c_void_p() if a is not None else None for a in arrays]
        try:
            for b, a in zip(bufs, arrays):
                if a is not None:
                    _hip_check(H.hipMalloc(C.byref(b), max(a.nbytes, 16)), "hipMalloc")
                    _hip_check(H.hipMemcpy(b, a.ctypes.data, a.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
            call(bufs)
            self.synchronize()
            for k in read:
                a, b = arrays[k], bufs[k]
                if a is not None:
                    _hip_check(H.hipMemcpy(a.ctypes.data, b, a.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
        finally:
            for b in bufs:
                if b:
                    H.hipFree(b)

    def _device_call(self, bufs, call, arrays, read=(), null=None, result=None, primary=0, returns=None, tensors=None, texts=None):
        """One library call over buffers that come as device tensors or as arrays: both paths of a wrapper.
        bufs: a row (name, value, torch dtype name, columns (0: one-dimensional), rows, absent) per buffer argument, in the order in which
        they are checked. rows: the row count expected: a number, the name of an earlier buffer (as many as it has), a function of the
        counts so far, or None (any). absent: what a value of None is: None (refused like any other wrong value), "null" (a NULL pointer),
        "empty" / "zeros" (a new tensor). call(d, n, stream) -> the library's status: d the device pointers in bufs' order, n each buffer's
        row count by name.
        Tensors, where the value of bufs[primary] is one (`tensors`: a verdict of the wrapper's instead): every tensor is held against its
        row (ValueError: texts[name] where given) and the primary's device, the call goes to that device's current stream and is not
        waited for -> the tensor of the buffer named `returns`, or None.
        Arrays otherwise: arrays() -> the buffers in bufs' order as the helpers above normalise them (None: NULL); _round_trip uploads
        them, calls on the context's stream, waits and downloads those at `read` — or, where null(n) finds a call of size zero, the library
        is called with NULL for every buffer — -> result(the arrays)."""
        head = bufs[primary][1]
        if _is_torch(head) if tensors is None else tensors:
            torch, dev = sys.modules["torch"], getattr(head, "device", None)
            Tensor, on_gpu = torch.Tensor, getattr(head, "is_cuda", False)   # a tensor on the primary's device is on a GPU if the primary is
            d, n, kept = [], {}, None   # (the pointers go as plain integers: the library's argument types convert them)
            for what, t, dtype, columns, rows, absent in bufs:
                if t is None and absent == "null":
                    d.append(None)
                    continue
                if type(rows) is str:
                    rows = n[rows]
                elif rows is not None and type(rows) is not int:
                    rows = rows(n)
                if t is None and absent is not None:
                    t = getattr(torch, absent)((rows, columns) if columns else (rows,), dtype=getattr(torch, dtype), device=dev)
                    shape = t.shape
                else:
                    shape = t.shape if isinstance(t, Tensor) else None
                    if (shape is None or t.dtype is not getattr(torch, dtype) or not t.is_contiguous() or not on_gpu or t.device != dev or
                            len(shape) != (2 if columns else 1) or (columns and shape[1] != columns) or (rows is not None and shape[0] != rows)):
                        raise ValueError(texts[what] if texts else f"{what}: a contiguous {dtype} device tensor of shape "
                                         f"({'N' if rows is None else rows}{', %d' % columns if columns else ''})")
                if what == returns:
                    kept = t
                n[what] = shape[0]
                d.append(t.data_ptr())
            _check(call(d, n, _stream_of(torch, dev)))
            return kept
        a = arrays()
        n = {row[0]: len(x) if x is not None else 0 for row, x in zip(bufs, a)}
        if null is not None and null(n):
            _check(call([None] * len(a), n, None))
        else:
            self._round_trip(a, lambda d: _check(call(d, n, None)), read)
        return result(a)

    def generate_rays(self, film, rng, first_pixel=0, index=None, rays=None, positions=None):
        """ptss_generate_rays: the eye rays of film pixels index[i] (first_pixel + i without an index) from streams rng[i].
        positions (ptss_generate_rays_positions): numpy: True -> a third result, the samples' places on the film, (N,) POSITION_DTYPE;
        torch: an (N, 2) float32 tensor to write.
        numpy: rng (N,) PATH_RNG_DTYPE or (N, 6) uint32 -> ((N,) RAY_DTYPE, (N,) PATH_RNG_DTYPE: the streams afterwards); rays: the
        buffer's content beforehand (zeros otherwise; an entry whose index leaves the film keeps it). torch: rng a contiguous (N, 6)
        int32 device tensor, UPDATED IN PLACE, index an (N,) int32 tensor or None, rays an (N, 8) float32 tensor to write (a new one
        otherwise) -> rays, on the current stream."""
        L = device_lib()
        first_pixel, placed = int(first_pixel), positions is not None
        bufs = [("rng", rng, "int32", 6, None, None), ("rays", rays, "float32", 8, "rng", "zeros"), ("index", index, "int32", 0, "rng", "null")]
        if placed:
            bufs.append(("positions", positions, "float32", 2, "rng", None))

        def arrays():
            s = _rng_words(rng)
            n = len(s)
            idx = _film_index(index, n)
            out = np.zeros((n, 8), dtype=np.float32) if rays is None else _rows(rays, RAY_DTYPE, 8, np.float32, "rays", copy=True)
            if len(out) != n:
                raise ValueError("rays: one row per stream")
            return [s, out, idx] + ([np.zeros((n, 2), dtype=np.float32)] if placed else [])

        def call(d, n, stream):
            if placed:
                return L.ptss_generate_rays_positions(self._ctx, C.byref(film), first_pixel, d[2], n["rng"], d[0], d[1], d[3], stream)
            return L.ptss_generate_rays(self._ctx, C.byref(film), first_pixel, d[2], n["rng"], d[0], d[1], stream)

        def result(a):
            out = (_records(a[1], RAY_DTYPE), _records(a[0], PATH_RNG_DTYPE))
            return out + (_records(a[3], POSITION_DTYPE),) if placed else out

        # without streams ptss_generate_rays is called with NULL; ptss_generate_rays_positions always with buffers
        return self._device_call(bufs, call, arrays, read=(0, 1, 3) if placed else (0, 1), null=None if placed else lambda n: n["rng"] == 0,
                                 result=result, returns="rays")

    _NO_MOMENTS = object()   # _accumulate's `moments` for a film that keeps none

    def _accumulate(self, call, film_dtype, word, results, film, index, moments=_NO_MOMENTS, pixels=None, history=None):
        """The body of accumulate_paths, accumulate_paths_stats and accumulate_paths_linear (accumulate_paths_linear_stats, whose film may
        be None and whose moments are records, has its own). film_dtype, word: the film's record and the type of its four words (a torch
        film holds them signed); call(d, n, stream): the C call as _device_call makes it, d the pointers of (results, film, moments, index,
        pixels, history). torch -> None; numpy -> (film, moments or None, pixels, history) afterwards."""
        keeps_moments = moments is not self._NO_MOMENTS

        def arrays():
            r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
            idx = _film_index(index, len(r))
            f = _rows(film, film_dtype, 4, word, "film", copy=True)
            m = _moments(moments, len(f)) if keeps_moments else None
            px, hs = _film_outputs(len(f), pixels=pixels, history=history)
            return [r, f, m, idx, px, hs]

        return self._device_call(
            [("results", results, "float32", 4, None, None), ("film", film, "int32" if word is np.uint32 else "int64", 4, None, None),
             ("moments", moments, "int64", 0, "film", None) if keeps_moments else ("moments", None, "int64", 0, "film", "null"),
             ("index", index, "int32", 0, "results", "null"), ("pixels", pixels, "uint8", 4, "film", "null"),
             ("history", history, "float32", 4, "film", "null")],
            call, arrays, read=(1, 2, 4, 5), null=lambda n: n["results"] == 0,
            result=lambda a: (_records(a[1], film_dtype), a[2], a[4], _records(a[5], HISTORY_DTYPE)))

    def accumulate_paths(self, results, film, first_pixel=0, index=None, pixels=None, history=None):
        """ptss_accumulate_paths: the samples of `results` added to the film, the touched pixels resolved.
        numpy: results (N,) PATH_RESULT_DTYPE or (N, 4) float32; film (P,) FILM_DTYPE or (P, 4) uint32 (not modified); pixels / history:
        None (NULL), True (zeros beforehand) or the buffer's content beforehand -> (film afterwards (P,) FILM_DTYPE, pixels (P, 4) uint8
        or None, history (P,) HISTORY_DTYPE or None). torch: results (N, 4) float32, film (P, 4) int32 UPDATED IN PLACE, index (N,) int32
        or None, pixels (P, 4) uint8 or None, history (P, 4) float32 or None, all on one device -> None, on the current stream."""
        L = device_lib()
        out = self._accumulate(lambda d, n, st: L.ptss_accumulate_paths(self._ctx, d[0], d[3], int(first_pixel), n["results"], d[1], n["film"], d[4], d[5], st),
                               FILM_DTYPE, np.uint32, results, film, index, pixels=pixels, history=history)
        return None if out is None else (out[0], out[2], out[3])

    def ray_features(self, rays):
        """ptss_ray_features: the first-hit feature row of every ray. rays: (N, 8) float32 or (N,) RAY_DTYPE -> (N,) FEATURE_DTYPE; or
        a contiguous (N, 8) float32 device tensor -> an (N, 8) float32 tensor (word 7 holds the bits of materialIdx), on the current
        stream."""
        L = device_lib()

        def arrays():
            a = _rows(rays, RAY_DTYPE, 8, np.float32, "rays")
            return [a, np.zeros(len(a), dtype=FEATURE_DTYPE)]

        return self._device_call([("rays", rays, "float32", 8, None, None), ("out", None, "float32", 8, "rays", "empty")],
                                 lambda d, n, stream: L.ptss_ray_features(self._ctx, d[0], d[1], n["rays"], stream),
                                 arrays, read=(1,), null=lambda n: n["rays"] == 0, result=lambda a: a[1], returns="out")

    def accumulate_paths_stats(self, results, film, moments, first_pixel=0, index=None, pixels=None, history=None):
        """ptss_accumulate_paths_stats: accumulate_paths, with the second moments kept as well.
        numpy: accumulate_paths' arguments and moments (P,) uint64 (not modified) -> (film, moments afterwards, pixels, history).
        torch: moments a contiguous (P,) int64 device tensor UPDATED IN PLACE like the film -> None, on the current stream."""
        L = device_lib()
        return self._accumulate(lambda d, n, st: L.ptss_accumulate_paths_stats(self._ctx, d[0], d[3], int(first_pixel), n["results"], d[1], d[2], n["film"],
                                                                                d[4], d[5], st),
                                FILM_DTYPE, np.uint32, results, film, index, moments, pixels, history)

    def plan_samples(self, film, moments, n, params=None, cdf=None, index=None, info=None):
        """ptss_plan_samples: the next round's index from film and moments.
        numpy: film (P,) FILM_DTYPE or (P, 4) uint32, moments (P,) uint64 -> (cdf (P,) uint64, index (n,) uint32, info: a dict).
        torch: film (P, 4) int32, moments (P,) int64, cdf a (plan_cdf_entries(P),) int64 tensor, index an (n,) int32 tensor and info a
        (4,) int64 tensor or None, all contiguous on one device, WRITTEN IN PLACE -> None, on the current stream."""
        L = device_lib()
        params = params if params is not None else plan_params()
        return self._plan(lambda d, rows, st: L.ptss_plan_samples(self._ctx, d[0], d[1], rows["film"], C.byref(params), int(n), d[2], d[3], d[4], st),
                          [(film, "film", FILM_DTYPE, np.uint32), (moments, "moments", None, np.uint64)], n, cdf, index, info)

    def _plan(self, call, inputs, n, cdf, index, info):
        """The body of plan_samples and plan_samples_linear. inputs: what the plan reads, a row (value, name, record dtype, type of its
        words) per array: P records of four words, or P plain words where the record is None; the first has records. call(d, rows,
        stream): the C call as _device_call makes it, d the pointers of (the inputs, cdf, index, info). torch -> None; numpy -> (cdf, index,
        info)."""
        n, k, first = int(n), len(inputs), inputs[0][1]
        bufs = [(what, value, "int32" if word is np.uint32 else "int64", 4 if record is not None else 0, first if j else None, None)
                for j, (value, what, record, word) in enumerate(inputs)]
        bufs += [("cdf", cdf, "int64", 0, lambda rows: plan_cdf_entries(rows[first]), None), ("index", index, "int32", 0, n, None),
                 ("info", info, "int64", 0, 4, "null")]

        def arrays():
            rows = []
            for value, what, record, word in inputs:
                rows.append(_rows(value, record, 4, word, what) if record is not None else _moments(value, len(rows[0])))
            return rows + [np.zeros(plan_cdf_entries(len(rows[0])), dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros(4, dtype=np.uint64)]

        return self._device_call(bufs, call, arrays, read=(k, k + 1, k + 2), null=lambda rows: n == 0,
                                 result=lambda a: (a[k][:len(a[0])], a[k + 1], plan_info_dict(a[k + 2])))

    def adaptive_launches(self):
        """ptss_adaptive_launches: (accumulate_paths_stats, plan_samples calls that launched since the context was created)."""
        return self._counters("ptss_adaptive_launches", 2)

    # --- the linear film (ptss_accumulate_paths_linear / ptss_resolve_linear) ------------------
    def accumulate_paths_linear(self, results, film, first_pixel=0, index=None, params=None):
        """ptss_accumulate_paths_linear: the linear radiance of `results` added to the fixed-point film.
        numpy: results (N,) PATH_RESULT_DTYPE or (N, 4) float32; film (P,) LINEAR_DTYPE or (P, 4) uint64 (not modified) -> the film
        afterwards, (P,) LINEAR_DTYPE. torch: results (N, 4) float32, film (P, 4) int64 UPDATED IN PLACE, index (N,) int32 or None, all
        on one device -> None, on the current stream."""
        L = device_lib()
        params = params if params is not None else linear_params()
        out = self._accumulate(lambda d, n, st: L.ptss_accumulate_paths_linear(self._ctx, d[0], d[3], int(first_pixel), n["results"], d[1], n["film"],
                                                                               C.byref(params), st),
                               LINEAR_DTYPE, np.uint64, results, film, index)
        return None if out is None else out[0]

    # --- adaptive sampling on the linear film (ptss_accumulate_paths_linear_stats / ptss_plan_samples_linear) ------------------
    def accumulate_paths_linear_stats(self, results, film, moments, first_pixel=0, index=None, params=None):
        """ptss_accumulate_paths_linear_stats: accumulate_paths_linear, with the luminance moments kept as well; film may be None
        (moments only). numpy: results (N,) PATH_RESULT_DTYPE or (N, 4) float32; film (P,) LINEAR_DTYPE or (P, 4) uint64 or None;
        moments (P,) MOMENT_DTYPE or (P, 4) uint64 (neither modified) -> (film afterwards or None, moments afterwards (P,) MOMENT_DTYPE).
        torch: results (N, 4) float32, film (P, 4) int64 or None, moments (P, 4) int64, both UPDATED IN PLACE, index (N,) int32 or None,
        all on one device -> None, on the current stream."""
        L = device_lib()
        params = params if params is not None else linear_params()

        def arrays():
            r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
            idx = _film_index(index, len(r))
            m = _rows(moments, MOMENT_DTYPE, 4, np.uint64, "moments", copy=True)
            f = _rows(film, LINEAR_DTYPE, 4, np.uint64, "film", copy=True) if film is not None else None
            if f is not None and len(f) != len(m):
                raise ValueError("moments: one row per film pixel")
            return [r, m, f, idx]

        return self._device_call(
            [("results", results, "float32", 4, None, None), ("moments", moments, "int64", 4, None, None), ("film", film, "int64", 4, "moments", "null"),
             ("index", index, "int32", 0, "results", "null")],
            lambda d, n, stream: L.ptss_accumulate_paths_linear_stats(self._ctx, d[0], d[3], int(first_pixel), n["results"], d[2], d[1], n["moments"],
                                                                      C.byref(params), stream),
            arrays, read=(1, 2), null=lambda n: n["results"] == 0, result=lambda a: (_records(a[2], LINEAR_DTYPE), _records(a[1], MOMENT_DTYPE)))

    def plan_samples_linear(self, moments, n, params=None, plan=None, cdf=None, index=None, info=None):
        """ptss_plan_samples_linear: the next round's index from a linear film's moments.
        numpy: moments (P,) MOMENT_DTYPE or (P, 4) uint64 -> (cdf (P,) uint64, index (n,) uint32, info: a dict). torch: moments (P, 4)
        int64, cdf a (plan_cdf_entries(P),) int64 tensor, index an (n,) int32 tensor and info a (4,) int64 tensor or None, all contiguous
        on one device, WRITTEN IN PLACE -> None, on the current stream. params: the film's linear_params; plan: a linear_plan_params."""
        L = device_lib()
        params = params if params is not None else linear_params()
        plan = plan if plan is not None else linear_plan_params()
        return self._plan(lambda d, rows, st: L.ptss_plan_samples_linear(self._ctx, d[0], rows["moments"], C.byref(params), C.byref(plan), int(n), d[1],
                                                                         d[2], d[3], st),
                          [(moments, "moments", MOMENT_DTYPE, np.uint64)], n, cdf, index, info)

    def linear_stats_launches(self):
        """ptss_linear_stats_launches: (accumulate_paths_linear_stats, plan_samples_linear calls that launched since the context was
        created)."""
        return self._counters("ptss_linear_stats_launches", 2)

    def resolve_linear(self, film, first_pixel=0, count=None, params=None, linear=True, pixels=True, history=True, metered=None, glare=None, tone=None):
        """ptss_resolve_linear: pixels first_pixel .. first_pixel + count (None: to the film's end) of a linear film resolved.
        numpy: film (P,) LINEAR_DTYPE or (P, 4) uint64; linear / pixels / history: None (NULL), True (zeros beforehand) or the buffer's
        content beforehand -> (linear (P,) HISTORY_DTYPE: the unexposed means and the sample count, pixels (P, 4) uint8, history (P,)
        HISTORY_DTYPE), each None when NULL. torch: film (P, 4) int64, linear (P, 4) float32 or None, pixels (P, 4) uint8 or None,
        history (P, 4) float32 or None, all on one device, WRITTEN IN PLACE -> None, on the current stream.
        metered: a meter's state (numpy: a METER_STATE_DTYPE record; torch: a (6,) int64 device tensor) -> ptss_resolve_linear_metered:
        the exposure is the state's times params.exposure. Without it ptss_resolve_linear is called.
        glare: (width, height, a glare_params, the pyramid glare_build gave for this film and those parameters; torch: an (entries, 4)
        int64 device tensor) -> ptss_resolve_linear_glare, with `metered` as its state or NULL.
        tone: (a tone_params, the table tone_build gave for it; torch: a (tone_table_floats(bits),) float32 device tensor) ->
        ptss_resolve_toned, with `metered` and `glare` as its state and its pyramid; pixels are the words' bytes (unpack_pixels10)."""
        L = device_lib()
        return self._resolve(L.ptss_resolve_linear, L.ptss_resolve_linear_metered, LINEAR_DTYPE, film, first_pixel, count, params, linear, pixels,
                             history, metered, L.ptss_resolve_linear_glare, glare, tone, FILM_LINEAR)

    def _resolve(self, plain, with_state, film_dtype, film, first_pixel, count, params, linear, pixels, history, metered, with_glare=None, glare=None,
                 tone=None, film_kind=FILM_LINEAR):
        """The body of resolve_linear and resolve_splat over a film of 32-byte entries: `plain`, `with_state` where `metered` is a state,
        `with_glare` where `glare` is (width, height, glare_params, pyramid), or ptss_resolve_toned where `tone` is (tone_params, table)."""
        L = device_lib()
        params = params if params is not None else linear_params()
        g_width, g_height, g_params, g_pyramid = glare if glare is not None else (0, 0, None, None)
        g_width, g_height, g_entries = int(g_width), int(g_height), glare_layout(g_width, g_height, g_params.levels)[1] if glare is not None else None
        t_params, t_table = tone if tone is not None else (None, None)

        span = lambda n: _linear_range(n["film"], first_pixel, count)

        def entries(n):   # of the pyramid, which is looked at once the film is seen to be the glare's
            if n["film"] != g_width * g_height:
                raise ValueError("film: width * height entries")
            return g_entries

        def call(d, n, stream):
            first, many = span(n)
            f, state, pyr, table, *out = d
            if tone is not None:
                return L.ptss_resolve_toned(self._ctx, f, int(film_kind), first, many, C.byref(params), C.byref(t_params), table, state, g_width,
                                            g_height, C.byref(g_params) if glare is not None else None, pyr, *out, stream)
            if glare is not None:
                return with_glare(self._ctx, f, first, many, C.byref(params), g_width, g_height, C.byref(g_params), pyr, state, *out, stream)
            if metered is not None:
                return with_state(self._ctx, f, first, many, C.byref(params), state, *out, stream)
            return plain(self._ctx, f, first, many, C.byref(params), *out, stream)

        def arrays():
            f = _rows(film, film_dtype, 4, np.uint64, "film")
            span({"film": len(f)})
            ln, px, hs = _film_outputs(len(f), linear=linear, pixels=pixels, history=history)
            state = _meter_state(metered) if metered is not None else None
            pyr = _glare_pyramid(g_pyramid, entries({"film": len(f)})) if glare is not None else None
            return [f, state, pyr, _tone_table(t_table, t_params.bits) if tone is not None else None, ln, px, hs]

        return self._device_call(
            [("film", film, "int64", 4, None, None), ("metered", metered, "int64", 0, 6, "null"),
             ("pyramid", g_pyramid, "int64", 4, entries if glare is not None else None, None if glare is not None else "null"),
             ("table", t_table, "float32", 0, tone_table_floats(t_params.bits) if tone is not None else None, None if tone is not None else "null"),
             ("linear", linear, "float32", 4, "film", "null"), ("pixels", pixels, "uint8", 4, "film", "null"),
             ("history", history, "float32", 4, "film", "null")],
            call, arrays, read=(4, 5, 6), null=lambda n: span(n)[1] == 0,
            result=lambda a: (_records(a[4], HISTORY_DTYPE), a[5], _records(a[6], HISTORY_DTYPE)))

    # --- the filtered linear film (ptss_splat_paths / ptss_splat_paths_homed / ptss_resolve_splat) ------------------
    def splat_paths(self, results, positions, film, width, height, filter=None, params=None, homed_first_pixel=None):
        """ptss_splat_paths, or with homed_first_pixel ptss_splat_paths_homed (sample i was aimed at pixel homed_first_pixel + i): the
        linear radiance of `results` spread around `positions` by the filter.
        numpy: results (N,) PATH_RESULT_DTYPE or (N, 4) float32; positions (N,) POSITION_DTYPE or (N, 2) float32; film (width * height,)
        SPLAT_DTYPE or (P, 4) uint64 (not modified) -> the film afterwards, (P,) SPLAT_DTYPE. torch: results (N, 4) float32, positions
        (N, 2) float32, film (P, 4) int64 UPDATED IN PLACE, all on one device -> None, on the current stream."""
        L = device_lib()
        filter = filter if filter is not None else splat_filter()
        params = params if params is not None else linear_params()
        width, height = int(width), int(height)

        def call(d, n, stream):
            if homed_first_pixel is None:
                return L.ptss_splat_paths(self._ctx, d[0], d[1], n["results"], d[2], width, height, C.byref(filter), C.byref(params), stream)
            return L.ptss_splat_paths_homed(self._ctx, d[0], d[1], int(homed_first_pixel), n["results"], d[2], width, height, C.byref(filter),
                                            C.byref(params), stream)

        def arrays():
            r = _rows(results, PATH_RESULT_DTYPE, 4, np.float32, "results")
            pos = _positions(positions, len(r))
            f = _rows(film, SPLAT_DTYPE, 4, np.uint64, "film", copy=True)
            if len(f) != width * height:
                raise ValueError("film: width * height entries")
            return [r, pos, f]

        return self._device_call([("results", results, "float32", 4, None, None), ("positions", positions, "float32", 2, "results", None),
                                  ("film", film, "int64", 4, width * height, None)],
                                 call, arrays, read=(2,), null=lambda n: n["results"] == 0, result=lambda a: _records(a[2], SPLAT_DTYPE))

    def resolve_splat(self, film, first_pixel=0, count=None, params=None, linear=True, pixels=True, history=True, metered=None, glare=None, tone=None):
        """ptss_resolve_splat: resolve_linear's arguments and results over a filtered film, (P,) SPLAT_DTYPE (torch: (P, 4) int64); the
        weight of linear and history is the summed filter weight. metered: as in resolve_linear (ptss_resolve_splat_metered); glare: as in
        resolve_linear (ptss_resolve_splat_glare); tone: as in resolve_linear (ptss_resolve_toned with PTSS_FILM_SPLAT)."""
        L = device_lib()
        return self._resolve(L.ptss_resolve_splat, L.ptss_resolve_splat_metered, SPLAT_DTYPE, film, first_pixel, count, params, linear, pixels,
                             history, metered, L.ptss_resolve_splat_glare, glare, tone, FILM_SPLAT)

    # --- tone curves for the two linear films (ptss_tone_build; the resolves take tone=) ------------------
    def tone_build(self, tone=None, table=None):
        """ptss_tone_build: the table of a tone_params on the device. numpy (table None) -> (tone_table_floats(bits),) float32, the bytes of
        probe_tone_build; raises where the thresholds came out of order. torch: table a (tone_table_floats(bits),) float32 device tensor
        WRITTEN IN PLACE -> None, on the current stream (tone_table_sorted reads its flag)."""
        L = device_lib()
        tone = tone if tone is not None else tone_params()
        floats = tone_table_floats(tone.bits) if tone.bits in (8, 10) else None   # other bits are the library's to refuse

        def result(a):
            if not tone_table_sorted(a[0]):
                raise PtssError("ptss_tone_build: the thresholds are not in order")
            return a[0]

        return self._device_call([("table", table, "float32", 0, floats, None)],
                                 lambda d, n, stream: L.ptss_tone_build(self._ctx, C.byref(tone), d[0], stream),
                                 lambda: [np.zeros(floats or 4, dtype=np.float32)], read=(0,), result=result, tensors=table is not None)

    def tone_launches(self):
        """ptss_tone_launches: (tone_build calls, toned resolves that launched since the context was created)."""
        return self._counters("ptss_tone_launches", 2)

    def debug_tone_form(self, form):
        """ptss_debug_tone_form: 0 the shipped lookup, 1 the table staged in LDS, 2 the guess settled against global memory."""
        _check(device_lib().ptss_debug_tone_form(self._ctx, int(form)))

    # --- glare for the two linear films (ptss_glare_build; the resolves take glare=) ------------------
    def glare_build(self, film, width, height, params=None, glare=None, film_kind=None, pyramid=None):
        """ptss_glare_build: the glare pyramid of a whole film. numpy: film (width * height,) LINEAR_DTYPE or SPLAT_DTYPE, or (P, 4)
        uint64 with film_kind "linear" / "splat" -> the pyramid, (entries,) GLARE_DTYPE: u_1 .. u_L as glare_layout places them. torch:
        film (P, 4) int64, film_kind given ("linear" where None), pyramid an (entries, 4) int64 device tensor WRITTEN IN PLACE -> None,
        on the current stream. params: the film's linear_params; glare: a glare_params."""
        L = device_lib()
        params = params if params is not None else linear_params()
        glare = glare if glare is not None else glare_params()
        width, height, kind = int(width), int(height), _film_kind(film_kind, FILM_LINEAR)
        entries = lambda n=None: glare_layout(width, height, glare.levels)[1]

        def arrays():
            nonlocal kind   # of an array it is what the film's dtype says
            f, kind = _glare_film(film, film_kind, width, height)
            return [f, np.zeros((entries(), 4), dtype=np.uint64)]

        return self._device_call([("film", film, "int64", 4, width * height, None), ("pyramid", pyramid, "int64", 4, entries, None)],
                                 lambda d, n, stream: L.ptss_glare_build(self._ctx, d[0], kind, width, height, C.byref(params), C.byref(glare), d[1], stream),
                                 arrays, read=(1,), result=lambda a: _records(a[1], GLARE_DTYPE))

    def glare_launches(self):
        """ptss_glare_launches: (glare_build calls, the kernels they launched, glare resolves that launched since the context was
        created)."""
        return self._counters("ptss_glare_launches", 3)

    # --- the denoiser of the two linear films (ptss_denoise_linear) ------------------
    def denoise_linear(self, film, width, height, moments, features, params=None, denoise=None, film_kind=None, out=None, workspace=None):
        """ptss_denoise_linear: a whole linear or filtered linear film filtered in linear light, guided by its moments, into a linear film.
        numpy: film (width * height,) LINEAR_DTYPE or SPLAT_DTYPE, or (P, 4) uint64 with film_kind "linear" / "splat"; moments (P,)
        MOMENT_DTYPE; features (P,) FEATURE_DTYPE -> the denoised film, (P,) LINEAR_DTYPE; workspace=True -> (film, the workspace's bytes
        afterwards as a uint8 array). torch: film and moments (P, 4) int64, features (P, 8) float32, out a (P, 4) int64 device tensor
        WRITTEN IN PLACE, workspace a uint8 device tensor of denoise_linear_workspace(width, height) bytes (a new one where None) -> None,
        on the current stream. params: the film's linear_params; denoise: a denoise_linear_params."""
        L = device_lib()
        params = params if params is not None else linear_params()
        denoise = denoise if denoise is not None else denoise_linear_params()
        width, height, kind = int(width), int(height), _film_kind(film_kind, FILM_LINEAR)
        P, nbytes = width * height, denoise_linear_workspace(width, height)

        def call(d, n, stream):
            if n["workspace"] < nbytes:
                raise ValueError("workspace: denoise_linear_workspace(width, height) bytes")
            return L.ptss_denoise_linear(self._ctx, d[0], kind, width, height, d[1], d[2], C.byref(params), C.byref(denoise), d[4], d[3], stream)

        def arrays():
            nonlocal kind   # of an array it is what the film's dtype says
            f, kind, m, ft = _denoise_linear_inputs(film, film_kind, width, height, moments, features)
            return [f, m, ft, np.zeros((len(f), 4), dtype=np.uint64), np.zeros((nbytes,), dtype=np.uint8)]

        return self._device_call([("film", film, "int64", 4, P, None), ("moments", moments, "int64", 4, P, None), ("features", features, "float32", 8, P, None),
                                  ("out", out, "int64", 4, P, None), ("workspace", workspace, "uint8", 0, nbytes if workspace is None else None, "empty")],
                                 call, arrays, read=(3, 4),
                                 result=lambda a: (_records(a[3], LINEAR_DTYPE), a[4]) if workspace else _records(a[3], LINEAR_DTYPE))

    def denoise_linear_launches(self):
        """ptss_denoise_linear_launches: (denoise_linear calls that launched, the kernels inside them since the context was created)."""
        return self._counters("ptss_denoise_linear_launches", 2)

    def debug_denoise_linear_form(self, form):
        """ptss_debug_denoise_linear_form (tests and measurements): 0 the measured form per spacing, 1 taps from global memory, 2 staged in
        LDS wherever that kernel exists, 4 + mask staged at pass k where bit k of the mask (0 .. 7) is set. The bytes are the same."""
        _check(device_lib().ptss_debug_denoise_linear_form(self._ctx, int(form)))

    # --- carrying the two linear films across a camera move (ptss_reproject_linear) ------------------
    def reproject_linear(self, now, features_now, prev, features_prev, film_prev, moments_prev=None, params=None, reproject=None, film_kind=None,
                         motion_now=None, out=None, moments_out=None, info=None):
        """ptss_reproject_linear: the previous pose's film seeds the new pose's. now, prev: film_camera()s; params: the film's
        linear_params; reproject: a reproject_linear_params.
        numpy: features_* FEATURE_DTYPE rows of each film's centre rays, film_prev (P',) LINEAR_DTYPE or SPLAT_DTYPE (or (P', 4) uint64
        with film_kind), moments_prev (P',) MOMENT_DTYPE or None, motion_now (P,) MOTION_DTYPE or None -> (the seeded film, its kind
        film_prev's; its moments or None; the info as a REPROJECT_LINEAR_INFO_DTYPE record). info: the counters' content beforehand.
        torch: features (P, 8) float32, film_prev and moments_prev (P', 4) int64, motion_now (P, 4) float32 or None; out and moments_out
        (P, 4) int64 device tensors WRITTEN IN PLACE, info a (4,) int64 device tensor ADDED TO or None -> None, on the current stream."""
        L = device_lib()
        params = params if params is not None else linear_params()
        reproject = reproject if reproject is not None else reproject_linear_params()
        Pn, Pp, kind = int(now.width) * int(now.height), int(prev.width) * int(prev.height), _film_kind(film_kind, FILM_LINEAR)

        def arrays():
            nonlocal kind   # of an array it is what the film's dtype says
            fn, mo, fp, f, kind, m = _reproject_linear_inputs(now, features_now, motion_now, prev, features_prev, film_prev, film_kind, moments_prev)
            inf = np.zeros(1, dtype=REPROJECT_LINEAR_INFO_DTYPE)
            if info is not None:
                inf[0] = info
            return [fn, fp, f, m, mo, np.zeros((len(fn), 4), dtype=np.uint64), np.zeros((len(fn), 4), dtype=np.uint64) if m is not None else None, inf]

        return self._device_call(
            [("features_now", features_now, "float32", 8, Pn, None), ("features_prev", features_prev, "float32", 8, Pp, None),
             ("film_prev", film_prev, "int64", 4, Pp, None), ("moments_prev", moments_prev, "int64", 4, Pp, "null"),
             ("motion_now", motion_now, "float32", 4, Pn, "null"), ("out", out, "int64", 4, Pn, None), ("moments_out", moments_out, "int64", 4, Pn, "null"),
             ("info", info, "int64", 0, 4, "null")],
            lambda d, n, stream: L.ptss_reproject_linear(self._ctx, C.byref(now), d[0], d[4], C.byref(prev), d[1], d[2], kind, d[3], C.byref(params),
                                                         C.byref(reproject), d[5], d[6], d[7], stream),
            arrays, read=(5, 6, 7), primary=2,   # the device is film_prev's
            result=lambda a: (_records(a[5], SPLAT_DTYPE if kind == FILM_SPLAT else LINEAR_DTYPE), _records(a[6], MOMENT_DTYPE), a[7][0]))

    def reproject_linear_launches(self):
        """ptss_reproject_linear_launches: the reproject_linear calls that launched since the context was created."""
        return self._counters("ptss_reproject_linear_launches", 1)

    # --- upsampling the two linear films (ptss_upsample_linear) ------------------
    def upsample_linear(self, film_lo, width, height, features_lo, features_hi, params=None, upsample=None, film_kind=None, out=None, info=None):
        """ptss_upsample_linear: a linear or a filtered linear film of width x height -> a linear film of factor times the size. params: the
        film's linear_params; upsample: an upsample_linear_params.
        numpy: film_lo (P,) LINEAR_DTYPE or SPLAT_DTYPE (or (P, 4) uint64 with film_kind), features_lo / features_hi FEATURE_DTYPE rows of
        both sizes -> (the large film, (factor^2 P,) LINEAR_DTYPE; the info as an UPSAMPLE_LINEAR_INFO_DTYPE record, or None with
        info=False: dev_info NULL). info: the counters' content beforehand.
        torch: film_lo (P, 4) int64, features (., 8) float32; out a (factor^2 P, 4) int64 device tensor WRITTEN IN PLACE, info a (3,) int64
        device tensor ADDED TO or None -> None, on the current stream."""
        L = device_lib()
        params = params if params is not None else linear_params()
        upsample = upsample if upsample is not None else upsample_linear_params()
        Pl, kind = int(width) * int(height), _film_kind(film_kind, FILM_LINEAR)
        Ph = Pl * int(upsample.factor) ** 2

        def arrays():
            nonlocal kind   # of an array it is what the film's dtype says
            f, kind, flo, fhi, P = _upsample_linear_inputs(film_lo, film_kind, width, height, features_lo, features_hi, upsample)
            inf = np.zeros(1, dtype=UPSAMPLE_LINEAR_INFO_DTYPE) if info is not False else None
            if info is not None and info is not False:
                inf[0] = info
            return [f, flo, fhi, np.zeros((P, 4), dtype=np.uint64), inf]

        return self._device_call(
            [("film_lo", film_lo, "int64", 4, Pl, None), ("features_lo", features_lo, "float32", 8, Pl, None),
             ("features_hi", features_hi, "float32", 8, Ph, None), ("out", out, "int64", 4, Ph, None), ("info", info, "int64", 0, 3, "null")],
            lambda d, n, stream: L.ptss_upsample_linear(self._ctx, d[0], kind, int(width), int(height), d[1], d[2], C.byref(params), C.byref(upsample),
                                                        d[3], d[4], stream),
            arrays, read=(3, 4), result=lambda a: (_records(a[3], LINEAR_DTYPE), a[4][0] if a[4] is not None else None))

    def upsample_linear_launches(self):
        """ptss_upsample_linear_launches: the upsample_linear calls that launched since the context was created."""
        return self._counters("ptss_upsample_linear_launches", 1)

    def debug_upsample_linear_form(self, form):
        """ptss_debug_upsample_linear_form (tests and measurements): 0 the form measured faster at each factor, 1 every tap from global
        memory, 2 the lo pixels of a tile divided once and staged in LDS. The bytes are the same."""
        _check(device_lib().ptss_debug_upsample_linear_form(self._ctx, int(form)))

    # --- rays from surface points and the gutter fill (ptss_generate_rays_surface / ptss_dilate_linear) ------------------
    def generate_rays_surface(self, points, rng, params=None, first_point=0, index=None, rays=None, surfels=None):
        """ptss_generate_rays_surface: ray i leaves from points[index[i]] (points[first_point + i] without an index) with stream rng[i].
        numpy: points (P,) SURFACE_POINT_DTYPE, rng (N,) PATH_RNG_DTYPE or (N, 6) uint32 -> ((N,) RAY_DTYPE, (N,) PATH_RNG_DTYPE: the
        streams afterwards, (N,) HIT_DTYPE surfels or None). rays / surfels: the buffers' content beforehand (zeros otherwise; surfels
        None: dev_surfels NULL, True: zeros): a rejected entry keeps it.
        torch: points a contiguous (P, 4) int32 device tensor, rng (N, 6) int32 UPDATED IN PLACE, index (N,) int32 or None, rays an
        (N, 8) float32 tensor to write (a new one otherwise), surfels an (N, 12) float32 tensor to write or None -> rays, on the
        current stream."""
        L = device_lib()
        params = params if params is not None else surface_params()
        first_point = int(first_point)
        bufs = [("points", points, "int32", 4, None, None), ("rng", rng, "int32", 6, None, None), ("rays", rays, "float32", 8, "rng", "zeros"),
                ("index", index, "int32", 0, "rng", "null"), ("surfels", surfels, "float32", 12, "rng", "null")]
        return self._device_call(
            bufs, lambda d, n, stream: L.ptss_generate_rays_surface(self._ctx, C.byref(params), d[0], n["points"], first_point, d[3], n["rng"], d[1],
                                                                    d[2], d[4], stream),
            lambda: _surface_buffers(points, rng, index, rays, surfels), read=(1, 2, 4), null=lambda n: n["rng"] == 0,
            result=lambda a: (_records(a[2], RAY_DTYPE), _records(a[1], PATH_RNG_DTYPE), _records(a[4], HIT_DTYPE)), primary=1, returns="rays")

    def dilate_linear(self, film, width, height, out=None):
        """ptss_dilate_linear: one gutter-fill pass over a width x height linear film. numpy: film (P,) LINEAR_DTYPE or (P, 4) uint64 ->
        the second film, (P,) LINEAR_DTYPE. torch: film (P, 4) int64, out a (P, 4) int64 device tensor to write (a new one otherwise)
        -> out, on the current stream."""
        L = device_lib()
        P = int(width) * int(height)
        return self._device_call(
            [("film", film, "int64", 4, P, None), ("out", out, "int64", 4, P, "empty")],
            lambda d, n, stream: L.ptss_dilate_linear(self._ctx, d[0], int(width), int(height), d[1], stream),
            lambda: [_dilate_film(film, width, height), np.zeros((P, 4), dtype=np.uint64)], read=(1,),
            result=lambda a: _records(a[1], LINEAR_DTYPE), returns="out")

    def surface_launches(self):
        """ptss_surface_launches: (generate_rays_surface, dilate_linear calls that launched since the context was created)."""
        return self._counters("ptss_surface_launches", 2)

    def surface_rejected(self):
        """ptss_surface_rejected: the entries generate_rays_surface dropped since the context was created (synchronises)."""
        return self._counters("ptss_surface_rejected", 1)

    def debug_dilate_linear_form(self, form):
        """ptss_debug_dilate_linear_form (tests and measurements): 0 the shipped form, 1 the nine rows from global memory, 2 a tile with
        its ring staged in LDS. The bytes are the same."""
        _check(device_lib().ptss_debug_dilate_linear_form(self._ctx, int(form)))

    # --- light maps read back (ptss_lookup_lightmap) ------------------
    def lookup_lightmap(self, hits, map, params, blocks_tri=None, blocks_sph=None, film=None, info=None, out=None, chain=None):
        """ptss_lookup_lightmap: hits -> linear film rows through a baked map. params: a lightmap_params (table counts left at 0 are
        the tables' lengths); film: the map's linear_params.
        numpy: hits (N,) HIT_DTYPE, map (W H,) LINEAR_DTYPE, blocks (.,) SURFACE_BLOCK_DTYPE or None -> ((N,) LINEAR_DTYPE, the four
        counts — filtered, empty, no block, rejected — as (4,) uint32, or None with info=False: dev_info NULL). info: the counts' content
        beforehand.
        torch: hits (N, 12) float32, map (W H, 4) int64, blocks (., 4) int32 or None, out an (N, 4) int64 device tensor to write (a new
        one otherwise), info a (4,) int32 device tensor ADDED TO or None -> out, on the current stream.
        chain (ptss_lookup_lightmap_chain): intersect_chain's rows for the hits — (N,) CHAIN_DTYPE or (N, 8) float32,
        torch (N, 8) float32 — whose throughput, clamped into [0, 1], tints every filtered row."""
        L = device_lib()
        film = film if film is not None else linear_params()
        params = _lightmap_counts(params, blocks_tri, blocks_sph)
        P = int(params.atlasWidth) * int(params.atlasHeight)
        if chain is not None:
            return self._device_call(
                [("hits", hits, "float32", 12, None, None), ("map", map, "int64", 4, P, None), ("blocks_tri", blocks_tri, "int32", 4, None, "null"),
                 ("blocks_sph", blocks_sph, "int32", 4, None, "null"), ("out", out, "int64", 4, "hits", "empty"),
                 ("info", info if info is not False else None, "int32", 0, 4, "null"), ("chain", chain, "float32", 8, "hits", None)],
                lambda d, n, stream: L.ptss_lookup_lightmap_chain(self._ctx, C.byref(params), C.byref(film), d[2], d[3], d[1], d[0], d[6], n["hits"], d[4],
                                                                  d[5], stream),
                lambda: _lightmap_buffers(hits, map, params, blocks_tri, blocks_sph, info, chain), read=(4, 5),
                result=lambda a: (_records(a[4], LINEAR_DTYPE), a[5]), returns="out")
        return self._device_call(
            [("hits", hits, "float32", 12, None, None), ("map", map, "int64", 4, P, None), ("blocks_tri", blocks_tri, "int32", 4, None, "null"),
             ("blocks_sph", blocks_sph, "int32", 4, None, "null"), ("out", out, "int64", 4, "hits", "empty"),
             ("info", info if info is not False else None, "int32", 0, 4, "null")],
            lambda d, n, stream: L.ptss_lookup_lightmap(self._ctx, C.byref(params), C.byref(film), d[2], d[3], d[1], d[0], n["hits"], d[4], d[5], stream),
            lambda: _lightmap_buffers(hits, map, params, blocks_tri, blocks_sph, info), read=(4, 5),
            result=lambda a: (_records(a[4], LINEAR_DTYPE), a[5]), returns="out")

    def lightmap_launches(self):
        """ptss_lightmap_launches: the lookup_lightmap calls that launched since the context was created."""
        return self._counters("ptss_lightmap_launches", 1)

    def lightmap_chain_launches(self):
        """ptss_lightmap_chain_launches: the lookup_lightmap(chain=...) calls that launched since the context was created."""
        return self._counters("ptss_lightmap_chain_launches", 1)

    def debug_lightmap_form(self, form):
        """ptss_debug_lightmap_form (tests and measurements): 0 the shipped form, 1 one lane per hit, 2 four lanes per hit. The bytes are
        the same."""
        _check(device_lib().ptss_debug_lightmap_form(self._ctx, int(form)))

    # --- the meter of the two linear films (ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure) ------------------
    def _meter(self, call, film_dtype, film, first_pixel, count, histogram):
        """The body of meter_linear and meter_splat."""
        span = lambda n: _linear_range(n["film"], first_pixel, count)
        return self._device_call([("film", film, "int64", 4, None, None), ("histogram", histogram, "int32", 0, METER_BINS, None)],
                                 lambda d, n, stream: call(self._ctx, d[0], *span(n), d[1], stream),
                                 lambda: [_rows(film, film_dtype, 4, np.uint64, "film"), _histogram(histogram)],
                                 read=(1,), null=lambda n: span(n)[1] == 0, result=lambda a: a[1])

    def meter_linear(self, film, first_pixel=0, count=None, histogram=None):
        """ptss_meter_linear: pixels first_pixel .. first_pixel + count (None: to the film's end) of a linear film counted into a
        luminance histogram. numpy: film (P,) LINEAR_DTYPE or (P, 4) uint64; histogram: the counts beforehand (not modified; None =
        zeros) -> the histogram afterwards, (METER_BINS,) uint32. torch: film (P, 4) int64, histogram a (METER_BINS,) int32 device tensor
        UPDATED IN PLACE -> None, on the current stream."""
        return self._meter(device_lib().ptss_meter_linear, LINEAR_DTYPE, film, first_pixel, count, histogram)

    def meter_splat(self, film, first_pixel=0, count=None, histogram=None):
        """ptss_meter_splat: meter_linear over a filtered film, (P,) SPLAT_DTYPE (torch: (P, 4) int64)."""
        return self._meter(device_lib().ptss_meter_splat, SPLAT_DTYPE, film, first_pixel, count, histogram)

    def meter_exposure(self, histogram, state=None, params=None, meter=None):
        """ptss_meter_exposure: one update of a meter's state from a histogram. numpy: histogram (METER_BINS,) uint32; state: the state
        beforehand (not modified; None = a new one) -> the state afterwards, (1,) METER_STATE_DTYPE. torch: histogram a (METER_BINS,)
        int32 device tensor, state a (6,) int64 device tensor (zeros = new) UPDATED IN PLACE -> None, on the current stream.
        params: the film's linear_params; meter: a meter_params."""
        L = device_lib()
        params = params if params is not None else linear_params()
        meter = meter if meter is not None else meter_params()
        return self._device_call([("histogram", histogram, "int32", 0, METER_BINS, None), ("state", state, "int64", 0, 6, None)],
                                 lambda d, n, stream: L.ptss_meter_exposure(self._ctx, d[0], C.byref(params), C.byref(meter), d[1], stream),
                                 lambda: [_histogram(histogram), _meter_state(state)], read=(1,), result=lambda a: a[1])

    def meter_launches(self):
        """ptss_meter_launches: (meter_linear / meter_splat, meter_exposure, metered resolve calls that launched since the context was
        created)."""
        return self._counters("ptss_meter_launches", 3)

    def splat_stats(self):
        """ptss_splat_stats: (scatter launches, homed launches, resolves, samples dropped, samples clamped) since the context was
        created; synchronises with the stream of the latest splat."""
        return self._counters("ptss_splat_stats", 5)

    def linear_launches(self):
        """ptss_linear_launches: (accumulate_paths_linear, resolve_linear calls that launched since the context was created)."""
        return self._counters("ptss_linear_launches", 2)

    def film_launches(self):
        """ptss_film_launches: (generate_rays, accumulate_paths, ray_features calls that launched since the context was created)."""
        return self._counters("ptss_film_launches", 3)

    def film_rejected(self):
        """ptss_film_rejected: the index entries the film calls dropped since the context was created (synchronises)."""
        return self._counters("ptss_film_rejected", 1)

    # --- first-hit features and the denoiser (ptss_render_features / ptss_denoise) ---------------------
    def _device_buffer(self, name, nbytes):
        """A device buffer owned by this renderer, allocated once per name and freed by close()."""
        bufs = self._buffers
        if name not in bufs:
            H = _hip_lib()
            _hip_check(H.hipSetDevice(self.cfg.device), "hipSetDevice")
            p = C.c_void_p()
            _hip_check(H.hipMalloc(C.byref(p), max(nbytes, 16)), "hipMalloc")
            bufs[name] = p
        return bufs[name]

    def _device_buffer_at_least(self, name, nbytes):
        """Like _device_buffer, but grown when a later call needs more."""
        have = getattr(self, "_buffer_bytes", {})
        if name in self._buffers and have.get(name, 0) < nbytes:
            _hip_lib().hipFree(self._buffers.pop(name))
        have[name] = max(have.get(name, 0), nbytes)
        self._buffer_bytes = have
        return self._device_buffer(name, nbytes)

    def features_devptr(self):
        return self._device_buffer("features", self.local_pixels * FEATURE_DTYPE.itemsize)

    def features(self, stream=None):
        """The first-hit feature buffer of the current camera: (local_pixels,) FEATURE_DTYPE. The device buffer is kept
        (features_devptr) and is what denoise() uses by default."""
        d = self.features_devptr()
        _check(device_lib().ptss_render_features(self._ctx, d, C.c_void_p(stream) if stream else None))
        out = np.empty(self.local_pixels, dtype=FEATURE_DTYPE)
        if self.local_pixels:
            if stream:
                _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
            self.synchronize()
            _hip_check(_hip_lib().hipMemcpy(out.ctypes.data, d, out.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
        self._have_features = True
        return out

    def motion_devptr(self):
        return self._device_buffer("motion", self.local_pixels * MOTION_DTYPE.itemsize)

    def features_motion(self, prev_triangles=None, first=0, stream=None):
        """ptss_render_features_motion: the first-hit features of the current camera AND where each pixel's surface point was in the
        previous pose -> ((local_pixels,) FEATURE_DTYPE, (local_pixels,) MOTION_DTYPE). prev_triangles: the previous pose of the
        triangles first .. first + n - 1 — an (n,) TRIANGLE_DTYPE array to upload, or a contiguous float32 device tensor of n x 19
        words (as update_triangles takes them; asynchronous work is ordered on `stream`, default the tensor's current torch stream)
        — or None: nothing moved. Both device buffers are kept (features_devptr, motion_devptr): denoise() and reproject(motion=True)
        use them."""
        L = device_lib()
        d_feat, d_mot = self.features_devptr(), self.motion_devptr()
        if _is_torch(prev_triangles):
            t = prev_triangles
            if t.dtype != _torch().float32 or not t.is_contiguous() or not t.is_cuda or t.numel() % 19:
                raise ValueError("prev_triangles: a contiguous float32 device tensor of n x 19 words")
            if stream is None:
                stream = _stream_of(_torch(), t.device)
            d_prev, count = C.c_void_p(t.data_ptr()) if t.numel() else None, t.numel() // 19
        elif prev_triangles is None:
            d_prev, count = None, 0
        else:
            a = np.ascontiguousarray(prev_triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
            d_prev, count = None, len(a)
            if count:
                d_prev = self._device_buffer_at_least("prev_triangles_upload", a.nbytes)
                _hip_check(_hip_lib().hipMemcpy(d_prev, a.ctypes.data, a.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
        _check(L.ptss_render_features_motion(self._ctx, d_prev, first, count, d_feat, d_mot, C.c_void_p(stream) if stream else None))
        feat = np.empty(self.local_pixels, dtype=FEATURE_DTYPE)
        mot = np.empty(self.local_pixels, dtype=MOTION_DTYPE)
        if self.local_pixels:
            if stream:
                _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
            self.synchronize()
            _hip_check(_hip_lib().hipMemcpy(feat.ctypes.data, d_feat, feat.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
            _hip_check(_hip_lib().hipMemcpy(mot.ctypes.data, d_mot, mot.nbytes, 2), "hipMemcpy")
        self._have_features = True
        return feat, mot

    def features_specular_devptr(self):
        return self._device_buffer("features_specular", self.local_pixels * FEATURE_DTYPE.itemsize)

    def features_specular(self, max_steps, steps=False, stream=None):
        """ptss_render_features_specular: the features behind mirrors and glass — the centre ray carried through at most max_steps
        (0..8) perfect reflections and refractions; depth is the chain's path length -> (local_pixels,) FEATURE_DTYPE, with
        steps=True also the steps taken per pixel, (local_pixels,) uint32. The device buffer is a separate one
        (features_specular_devptr): hand it, or the returned array, to denoise(features=...) / denoise_history(features=...);
        reproject() keeps using the first-hit features of features()."""
        d = self.features_specular_devptr()
        d_steps = self._device_buffer("specular_steps", self.local_pixels * 4) if steps else None
        _check(device_lib().ptss_render_features_specular(self._ctx, int(max_steps), d, d_steps, C.c_void_p(stream) if stream else None))
        out = np.empty(self.local_pixels, dtype=FEATURE_DTYPE)
        taken = np.zeros(self.local_pixels, dtype=np.uint32)
        if self.local_pixels:
            if stream:
                _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
            self.synchronize()
            _hip_check(_hip_lib().hipMemcpy(out.ctypes.data, d, out.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
            if steps:
                _hip_check(_hip_lib().hipMemcpy(taken.ctypes.data, d_steps, taken.nbytes, 2), "hipMemcpy")
        return (out, taken) if steps else out

    def specular_feature_launches(self):
        """ptss_specular_feature_launches: (launches with the scene image read in place, launches with it staged in LDS)."""
        return self._counters("ptss_specular_feature_launches", 2)

    # --- rendering below display size (ptss_render_features_scaled / ptss_upsample) ---------------------------
    def features_scaled_devptr(self, factor):
        return self._device_buffer(f"features_x{int(factor)}", self.local_pixels * factor * factor * FEATURE_DTYPE.itemsize)

    def features_scaled(self, factor, stream=None):
        """ptss_render_features_scaled: the first-hit features of the current camera for the frame of factor * width x factor * height
        -> (factor^2 * local_pixels,) FEATURE_DTYPE, factor hi-res rows per local row. The device buffer is kept per factor
        (features_scaled_devptr) and is what upsample() uses by default."""
        factor = _upsample_factor(factor)
        d = self.features_scaled_devptr(factor)
        _check(device_lib().ptss_render_features_scaled(self._ctx, factor, d, C.c_void_p(stream) if stream else None))
        out = np.empty(self.local_pixels * factor * factor, dtype=FEATURE_DTYPE)
        if self.local_pixels:
            if stream:
                _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
            self.synchronize()
            _hip_check(_hip_lib().hipMemcpy(out.ctypes.data, d, out.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
        self._have_scaled.add(factor)
        return out

    def upsample(self, lo=None, features_lo=None, features_hi=None, factor=2, sigma_normal=None, sigma_depth=None, dev_out=None, floats=False,
                 stream=None):
        """ptss_upsample -> (factor^2 * local_pixels, 4) uint8 RGBA of the factor times larger frame; with floats=True also the
        (factor^2 * local_pixels,) HISTORY_DTYPE floats before the byte conversion (weight = the taps' weight sum). lo: None (the
        context's pixels, pixels_devptr()), a device pointer (int) or an (local_pixels, 4) uint8 array to upload — e.g. what
        denoise() returned. features_lo: as denoise()'s features (None: rendered on demand); features_hi: None (features_scaled(factor),
        rendered now unless the buffer holds this camera's), a device pointer (int) or an array to upload."""
        factor = _upsample_factor(factor)
        params = default_upsample_params(factor=factor, sigmaNormal=sigma_normal, sigmaDepth=sigma_depth)
        n_hi = self.local_pixels * factor ** 2
        if lo is None:
            d_lo = self.pixels_devptr()
        elif isinstance(lo, int):
            d_lo = C.c_void_p(lo)
        else:
            a = np.ascontiguousarray(lo, dtype=np.uint8).reshape(-1, 4)
            if len(a) != self.local_pixels:
                raise ValueError("lo: one RGBA pixel per local pixel")
            d_lo = self._device_buffer("upsample_lo_upload", a.nbytes)
            _hip_check(_hip_lib().hipMemcpy(d_lo, a.ctypes.data, a.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
        if features_lo is None:
            if not self._have_features:
                self.features()
            d_flo = self.features_devptr()
        else:
            d_flo = self._device_input("features_upload", features_lo, FEATURE_DTYPE)
        if features_hi is None:
            if factor not in self._have_scaled:
                self.features_scaled(factor)
            d_fhi = self.features_scaled_devptr(factor)
        elif isinstance(features_hi, int):
            d_fhi = C.c_void_p(features_hi)
        else:
            f = np.ascontiguousarray(features_hi, dtype=FEATURE_DTYPE).reshape(-1)
            if len(f) != n_hi:
                raise ValueError("features_hi: factor^2 entries per local pixel")
            d_fhi = self._device_buffer_at_least("features_hi_upload", f.nbytes)
            _hip_check(_hip_lib().hipMemcpy(d_fhi, f.ctypes.data, f.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
        if dev_out is None:
            dev_out = self._device_buffer_at_least("upsampled", max(n_hi, 1) * 4)
        elif isinstance(dev_out, int):
            dev_out = C.c_void_p(dev_out)
        d_flt = self._device_buffer_at_least("upsampled_float", max(n_hi, 1) * HISTORY_DTYPE.itemsize) if floats else None
        _check(device_lib().ptss_upsample(self._ctx, d_lo, d_flo, d_fhi, C.byref(params), dev_out, d_flt, C.c_void_p(stream) if stream else None))
        rgba = np.empty((n_hi, 4), dtype=np.uint8)
        flt = np.empty(n_hi, dtype=HISTORY_DTYPE)
        if n_hi:
            if stream:
                _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
            self.synchronize()
            _hip_check(_hip_lib().hipMemcpy(rgba.ctypes.data, dev_out, rgba.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
            if floats:
                _hip_check(_hip_lib().hipMemcpy(flt.ctypes.data, d_flt, flt.nbytes, 2), "hipMemcpy")
        return (rgba, flt) if floats else rgba

    def upsample_launches(self):
        """ptss_upsample_launches: accepted ptss_upsample calls that launched, since the context was created."""
        return self._counters("ptss_upsample_launches", 1)

    def denoise(self, features=None, levels=None, sigma_color=None, sigma_normal=None, sigma_depth=None, dev_out=None, stream=None):
        """ptss_denoise of the accumulated image -> (local_pixels, 4) uint8 RGBA. features: None (the buffer of the last
        features() call, rendered now if there is none or the camera was set since), a FEATURE_DTYPE array to upload, or a device
        pointer (int). dev_out: a
        device pointer to write to (e.g. pixels_devptr()); default a buffer of its own."""
        L = device_lib()
        if features is None:
            if not self._have_features:
                self.features()
            d_feat = self.features_devptr()
        elif isinstance(features, int):
            d_feat = C.c_void_p(features)
        else:
            f = np.ascontiguousarray(features, dtype=FEATURE_DTYPE).reshape(-1)
            if len(f) != self.local_pixels:
                raise ValueError("features: one entry per local pixel")
            d_feat = self._device_buffer("features_upload", f.nbytes)
            _hip_check(_hip_lib().hipMemcpy(d_feat, f.ctypes.data, f.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
        params = default_denoise_params(levels=levels, sigmaColor=sigma_color, sigmaNormal=sigma_normal, sigmaDepth=sigma_depth)
        if dev_out is None:
            dev_out = self._device_buffer("denoised", self.local_pixels * 4)
        elif isinstance(dev_out, int):
            dev_out = C.c_void_p(dev_out)
        _check(L.ptss_denoise(self._ctx, d_feat, C.byref(params), dev_out, C.c_void_p(stream) if stream else None))
        if stream:
            _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
        return self.pixels(dev_out)

    def _device_input(self, name, value, dtype):
        """A device pointer for `value`: an int is one already; an array is uploaded into the renderer's buffer `name`."""
        if isinstance(value, int):
            return C.c_void_p(value)
        a = np.ascontiguousarray(value, dtype=dtype).reshape(-1)
        if len(a) != self.local_pixels:
            raise ValueError(f"{name}: one entry per local pixel")
        d = self._device_buffer(name, a.nbytes)
        _hip_check(_hip_lib().hipMemcpy(d, a.ctypes.data, a.nbytes, 1), "hipMemcpy")   # hipMemcpyHostToDevice
        return d

    def history_devptr(self, which=0):
        """One of the renderer's own history buffers (local_pixels HISTORY_DTYPE entries): reproject() writes number 0 by default."""
        return self._device_buffer(f"history{which}", self.local_pixels * HISTORY_DTYPE.itemsize)

    def read_history(self, devptr=None):
        """Device -> host copy of a history buffer (default: history_devptr()) -> (local_pixels,) HISTORY_DTYPE."""
        d = self.history_devptr() if devptr is None else (C.c_void_p(devptr) if isinstance(devptr, int) else devptr)
        out = np.empty(self.local_pixels, dtype=HISTORY_DTYPE)
        if self.local_pixels:
            _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
            _hip_check(_hip_lib().hipMemcpy(out.ctypes.data, d, out.nbytes, 2), "hipMemcpy")   # hipMemcpyDeviceToHost
        return out

    def reproject(self, prev_camera=None, prev_features=None, prev_history=None, features=None, params=None, dev_out=None, stream=None,
                  read=True, motion=None, **overrides):
        """ptss_reproject: the history of the previous pose carried into the current frame -> (local_pixels,) HISTORY_DTYPE (None
        with read=False: the caller keeps the device buffer). prev_history None = no history. prev_features / prev_history /
        features: device pointers (int) the caller keeps, or arrays that are uploaded; features None = the buffer of the last
        features() call, rendered now if the camera was set since. dev_out: a device pointer (default history_devptr()), never
        prev_history's. params: a ReprojectParams (default_reproject_params(**overrides) otherwise). motion: None = ptss_reproject;
        otherwise ptss_reproject_motion with these rows of the CURRENT pose — True (the buffer of the last features_motion() call),
        a device pointer (int) or a MOTION_DTYPE array to upload."""
        if features is None:
            if not self._have_features:
                self.features()
            d_now = self.features_devptr()
        else:
            d_now = self._device_input("features_upload", features, FEATURE_DTYPE)
        d_fprev = d_hprev = None
        if prev_history is not None:
            if prev_camera is None or prev_features is None:
                raise ValueError("a history needs its camera and its features")
            d_fprev = self._device_input("prev_features_upload", prev_features, FEATURE_DTYPE)
            d_hprev = self._device_input("prev_history_upload", prev_history, HISTORY_DTYPE)
        if params is None:
            params = default_reproject_params(**overrides)
        if dev_out is None:
            dev_out = self.history_devptr()
        elif isinstance(dev_out, int):
            dev_out = C.c_void_p(dev_out)
        cam = C.byref(prev_camera) if prev_camera is not None else None
        if motion is None or motion is False:
            _check(device_lib().ptss_reproject(self._ctx, d_now, cam, d_fprev, d_hprev, C.byref(params), dev_out,
                                               C.c_void_p(stream) if stream else None))
        else:
            d_mot = self.motion_devptr() if motion is True else self._device_input("motion_upload", motion, MOTION_DTYPE)
            _check(device_lib().ptss_reproject_motion(self._ctx, d_now, d_mot, cam, d_fprev, d_hprev, C.byref(params), dev_out,
                                                      C.c_void_p(stream) if stream else None))
        return self.read_history(dev_out) if read else None

    def denoise_history(self, history=None, features=None, levels=None, sigma_color=None, sigma_normal=None, sigma_depth=None, dev_out=None,
                        stream=None):
        """ptss_denoise_history: the A-trous passes over a history's colours -> (local_pixels, 4) uint8 RGBA. history: None (the
        buffer reproject() wrote last by default, history_devptr()), a device pointer (int) or a HISTORY_DTYPE array to upload;
        features and dev_out as in denoise()."""
        d_hist = self.history_devptr() if history is None else self._device_input("history_upload", history, HISTORY_DTYPE)
        if features is None:
            if not self._have_features:
                self.features()
            d_feat = self.features_devptr()
        else:
            d_feat = self._device_input("features_upload", features, FEATURE_DTYPE)
        params = default_denoise_params(levels=levels, sigmaColor=sigma_color, sigmaNormal=sigma_normal, sigmaDepth=sigma_depth)
        if dev_out is None:
            dev_out = self._device_buffer("denoised", self.local_pixels * 4)
        elif isinstance(dev_out, int):
            dev_out = C.c_void_p(dev_out)
        _check(device_lib().ptss_denoise_history(self._ctx, d_hist, d_feat, C.byref(params), dev_out, C.c_void_p(stream) if stream else None))
        if stream:
            _hip_check(_hip_lib().hipDeviceSynchronize(), "hipDeviceSynchronize")
        return self.pixels(dev_out)

    def denoise_plane(self):
        """ptss_read_denoise_plane: (the filtered floats (local_pixels, 3) float32 that the last non-final pass of the latest
        denoise() left, that pass's level index)."""
        out = np.empty((self.local_pixels, 3), dtype=np.float32)
        level = C.c_int(-1)
        _check(device_lib().ptss_read_denoise_plane(self._ctx, out.ctypes.data_as(_f32p), out.size, C.byref(level)))
        return out, level.value

    def triangle_leaves(self):
        """Leaves (16 triangles each) of the mesh image in use; 0 when the image walks every triangle."""
        v = C.c_int()
        _check(device_lib().ptss_triangle_leaves(self._ctx, C.byref(v)))
        return v.value

    def debug_counters(self):
        """The eight counter words of a diagnostic build (-DPTSS_DIAG); zeros from the shipped library."""
        out = (C.c_ulonglong * 8)()
        _check(device_lib().ptss_debug_counters(self._ctx, out))
        return [int(x) for x in out]

    def bounce_kernel_time(self):
        ms = C.c_double()
        n = C.c_ulonglong()
        _check(device_lib().ptss_bounce_kernel_time(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value
