"""ctypes mirrors of include/ptss_types.h (field order = the reference's RenderStructs.h / Primitives.h)."""
import ctypes as C

import numpy as np


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tuple(self):
        return (self.x, self.y, self.z)


class Quat(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class UChar4(C.Structure):
    _fields_ = [("x", C.c_ubyte), ("y", C.c_ubyte), ("z", C.c_ubyte), ("w", C.c_ubyte)]


class Sphere(C.Structure):
    _fields_ = [("position", Vec3), ("radius", C.c_float), ("materialIdx", C.c_int)]


class Triangle(C.Structure):
    _fields_ = [("vertex0", Vec3), ("vertex1", Vec3), ("vertex2", Vec3),
                ("normal0", Vec3), ("normal1", Vec3), ("normal2", Vec3), ("materialIdx", C.c_int)]


class Material(C.Structure):
    _fields_ = [("diffuseColor", Vec3), ("specularColor", Vec3), ("absorption", Vec3), ("emmitance", Vec3),
                ("specularExponent", C.c_float), ("indexOfRefraction", C.c_float), ("diffAvg", C.c_float),
                ("specAvg", C.c_float), ("refrAvg", C.c_float), ("roughness", C.c_float), ("flags", C.c_char)]


class PointLight(C.Structure):
    _fields_ = [("position", Vec3), ("power", Vec3)]


class AreaLight(C.Structure):
    _fields_ = [("power", Vec3), ("area", C.c_float), ("triangleIdx", C.c_int), ("numTriangles", C.c_size_t)]


class Camera(C.Structure):
    _fields_ = [("rotation", Quat), ("position", Vec3), ("zNear", C.c_float), ("zFar", C.c_float),
                ("fieldOfView", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [("spheres", C.POINTER(Sphere)), ("numSpheres", C.c_size_t),
                ("triangles", C.POINTER(Triangle)), ("numTriangles", C.c_size_t),
                ("materials", C.POINTER(Material)), ("numMaterials", C.c_size_t),
                ("pointLights", C.POINTER(PointLight)), ("numPointLights", C.c_size_t),
                ("areaLights", C.POINTER(AreaLight)), ("numAreaLights", C.c_size_t),
                ("defaultColor", Vec3)]


class RayQuery(C.Structure):
    _fields_ = [("origin", Vec3), ("tmax", C.c_float), ("direction", Vec3), ("pad", C.c_float)]


class RayHit(C.Structure):
    _fields_ = [("point", Vec3), ("distance", C.c_float), ("normal", Vec3), ("materialIdx", C.c_int), ("kind", C.c_int),
                ("primitive", C.c_int), ("w1", C.c_float), ("w2", C.c_float)]


class PixelFeature(C.Structure):
    _fields_ = [("normal", Vec3), ("depth", C.c_float), ("albedo", Vec3), ("materialIdx", C.c_int)]


class DenoiseParams(C.Structure):
    _fields_ = [("structSize", C.c_uint), ("levels", C.c_int), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float),
                ("sigmaDepth", C.c_float)]


class HistoryEntry(C.Structure):
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("weight", C.c_float)]


class PixelMotion(C.Structure):
    _fields_ = [("prevPoint", Vec3), ("surface", C.c_int)]


SURFACE_TRIANGLE = 0x40000000   # PixelMotion.surface of triangle t: this | t


class PathRng(C.Structure):   # ptss_path_rng: one XORWOW state, in the order of ptss_read_rng_state
    _fields_ = [("v", C.c_uint32 * 5), ("d", C.c_uint32)]


class PathResult(C.Structure):   # ptss_path_result: linear radiance0 and the iterations entered
    _fields_ = [("radiance", Vec3), ("bounces", C.c_uint32)]


# the same two rows as numpy record types (Renderer.seed_path_rng / trace_paths)
PATH_RNG_DTYPE = np.dtype([("v", np.uint32, 5), ("d", np.uint32)])
PATH_RESULT_DTYPE = np.dtype([("radiance", np.float32, 3), ("bounces", np.uint32)])


class PathOptions(C.Structure):   # ptss_path_options: how ptss_trace_paths_opt schedules a batch
    _fields_ = [("structSize", C.c_uint), ("schedule", C.c_int), ("maxWorkgroups", C.c_int), ("reserved", C.c_int)]


PATHS_LANE_PER_RAY, PATHS_REFILL = 0, 1   # PTSS_PATHS_*


class FilmCamera(C.Structure):   # ptss_film_camera: the camera model of a film (ptss_generate_rays)
    _fields_ = [("structSize", C.c_uint), ("kind", C.c_int), ("camera", Camera), ("width", C.c_int), ("height", C.c_int),
                ("lensRadius", C.c_float), ("focusDistance", C.c_float), ("jitter", C.c_int)]


FILM_PINHOLE, FILM_THIN_LENS, FILM_EQUIRECT = 0, 1, 2   # PTSS_FILM_*


class FilmEntry(C.Structure):   # ptss_film_entry: the 8-bit sample sums of one film pixel and their count
    _fields_ = [("r", C.c_uint32), ("g", C.c_uint32), ("b", C.c_uint32), ("samples", C.c_uint32)]


FILM_DTYPE = np.dtype([("r", np.uint32), ("g", np.uint32), ("b", np.uint32), ("samples", np.uint32)])


class PlanParams(C.Structure):   # ptss_plan_params: how ptss_plan_samples weighs a film pixel
    _fields_ = [("structSize", C.c_uint), ("minSamples", C.c_uint32), ("maxSamples", C.c_uint32), ("threshold", C.c_float)]


class PlanInfo(C.Structure):   # ptss_plan_info: what a plan found
    _fields_ = [("totalWeight", C.c_ulonglong), ("activePixels", C.c_uint32), ("unsampledPixels", C.c_uint32), ("cappedPixels", C.c_uint32),
                ("uniform", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class LinearEntry(C.Structure):   # ptss_linear_entry: the fixed-point radiance sums of one linear-film pixel and their counts
    _fields_ = [("r", C.c_ulonglong), ("g", C.c_ulonglong), ("b", C.c_ulonglong), ("samples", C.c_uint32), ("clamped", C.c_uint32)]


LINEAR_DTYPE = np.dtype([("r", np.uint64), ("g", np.uint64), ("b", np.uint64), ("samples", np.uint32), ("clamped", np.uint32)])


class LinearParams(C.Structure):   # ptss_linear_params: how a linear film counts and shows radiance
    _fields_ = [("structSize", C.c_uint), ("scaleLog2", C.c_int), ("clampMax", C.c_float), ("exposure", C.c_float), ("reserved", C.c_uint)]


class LinearMoment(C.Structure):   # ptss_linear_moment: the luminance moments of one linear-film pixel (y^2 kept as two sums) and their count
    _fields_ = [("sumY", C.c_ulonglong), ("sqLo", C.c_ulonglong), ("sqHi", C.c_ulonglong), ("samples", C.c_ulonglong)]


MOMENT_DTYPE = np.dtype([("sumY", np.uint64), ("sqLo", np.uint64), ("sqHi", np.uint64), ("samples", np.uint64)])


class LinearPlanParams(C.Structure):   # ptss_linear_plan_params: how ptss_plan_samples_linear weighs a pixel
    _fields_ = [("structSize", C.c_uint), ("minSamples", C.c_uint32), ("maxSamples", C.c_uint32), ("threshold", C.c_float), ("floor", C.c_float),
                ("reserved", C.c_uint32 * 3)]


class FilmPosition(C.Structure):   # ptss_film_position: where a sample lies on the film, in pixels
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


POSITION_DTYPE = np.dtype([("x", np.float32), ("y", np.float32)])
SPLAT_BOX, SPLAT_TENT, SPLAT_GAUSSIAN = 0, 1, 2


class SplatFilter(C.Structure):   # ptss_splat_filter: the reconstruction filter of a filtered linear film
    _fields_ = [("structSize", C.c_uint), ("kind", C.c_int), ("radius", C.c_float), ("alpha", C.c_float), ("reserved", C.c_uint)]


class SplatEntry(C.Structure):   # ptss_splat_entry: the weighted fixed-point sums of one filtered-film pixel and the sum of the weights
    _fields_ = [("r", C.c_ulonglong), ("g", C.c_ulonglong), ("b", C.c_ulonglong), ("weight", C.c_ulonglong)]


SPLAT_DTYPE = np.dtype([("r", np.uint64), ("g", np.uint64), ("b", np.uint64), ("weight", np.uint64)])
METER_BINS = 329   # PTSS_METER_BINS: the 32-bit counts of a meter's histogram
# the launch shape of the histogram kernels (csrc/ptmeter.h kBlock, kGridCap): a film of more than their product makes the grid stride
METER_BLOCK, METER_GRID_CAP = 1024, 256


class MeterParams(C.Structure):   # ptss_meter_params: how a histogram becomes an exposure
    _fields_ = [("structSize", C.c_uint), ("key", C.c_float), ("lowPermille", C.c_uint), ("highPermille", C.c_uint), ("rate", C.c_float),
                ("minExposure", C.c_float), ("maxExposure", C.c_float), ("reserved", C.c_uint)]


class MeterState(C.Structure):   # ptss_meter_state: a meter's exposure and the integers of its latest update
    _fields_ = [("exposure", C.c_float), ("target", C.c_float), ("meanLog2", C.c_float), ("updates", C.c_uint32), ("metered", C.c_ulonglong),
                ("black", C.c_ulonglong), ("counted", C.c_ulonglong), ("sumLog", C.c_ulonglong)]


METER_STATE_DTYPE = np.dtype([("exposure", np.float32), ("target", np.float32), ("meanLog2", np.float32), ("updates", np.uint32),
                              ("metered", np.uint64), ("black", np.uint64), ("counted", np.uint64), ("sumLog", np.uint64)])


# glare for the two linear films (include/ptss_types.h PTSS_GLARE_*; csrc/ptglare.h kTile, kTailEntries: the shapes of ptss_glare.hip)
GLARE_MAX_LEVELS, GLARE_ADD, GLARE_MIX, GLARE_FILM_LINEAR, GLARE_FILM_SPLAT = 8, 0, 1, 0, 1
GLARE_TILE, GLARE_TAIL_ENTRIES = 16, 2730


class GlareParams(C.Structure):   # ptss_glare_params: the pyramid's levels, how it joins the mean, what counts as a highlight
    _fields_ = [("structSize", C.c_uint), ("levels", C.c_int), ("mode", C.c_int), ("threshold", C.c_float), ("strength", C.c_float),
                ("reserved", C.c_uint)]


class GlareLevel(C.Structure):   # ptss_glare_level: one level of a pyramid
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("first", C.c_ulonglong)]


GLARE_DTYPE = np.dtype([("r", np.uint64), ("g", np.uint64), ("b", np.uint64), ("zero", np.uint64)])   # ptss_glare_entry


# the denoiser of the two linear films (include/ptss_types.h PTSS_FILM_*; csrc/ptlindn.h: an empty pixel's variance, workspace bytes per pixel)
FILM_LINEAR, FILM_SPLAT = GLARE_FILM_LINEAR, GLARE_FILM_SPLAT
DENOISE_MAX_LEVELS = 6
DENOISE_LINEAR_EMPTY, DENOISE_LINEAR_WORKSPACE_BYTES = -1.0, 52


class DenoiseLinearParams(C.Structure):   # ptss_denoise_linear_params: the passes and the three tolerances of ptss_denoise_linear
    _fields_ = [("structSize", C.c_uint), ("levels", C.c_int), ("sigmaLuminance", C.c_float), ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float),
                ("reserved", C.c_uint32 * 3)]


# carrying the two linear films across a camera move (ptss_reproject_linear)
REPROJECT_LINEAR_MAX_HISTORY = (1 << 23) - 1


class ReprojectLinearParams(C.Structure):   # ptss_reproject_linear_params: the tap tests and the cap of the history count
    _fields_ = [("structSize", C.c_uint), ("cosNormal", C.c_float), ("depthTolerance", C.c_float), ("minCoverage", C.c_float),
                ("maxHistory", C.c_uint32), ("reserved", C.c_uint)]


# ptss_reproject_linear_info: what a call adds to the caller's four counters
REPROJECT_LINEAR_INFO_DTYPE = np.dtype([("seeded", np.uint64), ("offFilm", np.uint64), ("noTap", np.uint64), ("noVariance", np.uint64)])


# upsampling the two linear films (ptss_upsample_linear)
UPSAMPLE_LINEAR_WRAP_X = 1


class UpsampleLinearParams(C.Structure):   # ptss_upsample_linear_params
    _fields_ = [("structSize", C.c_uint), ("factor", C.c_int), ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float), ("flags", C.c_uint),
                ("reserved", C.c_uint)]


# ptss_upsample_linear_info: what a call adds to the caller's three counters
UPSAMPLE_LINEAR_INFO_DTYPE = np.dtype([("filtered", np.uint64), ("fallback", np.uint64), ("empty", np.uint64)])


# tone curves for the two linear films (include/ptss_types.h PTSS_TONE_*, PTSS_TRANSFER_*)
TONE_CLAMP, TONE_REINHARD, TONE_FILMIC = 0, 1, 2
TRANSFER_GAMMA22, TRANSFER_SRGB = 0, 1
TONE_LUMINANCE = 1


class ToneParams(C.Structure):   # ptss_tone_params: the curve, the transfer function, the bit depth
    _fields_ = [("structSize", C.c_uint), ("curve", C.c_int), ("transfer", C.c_int), ("bits", C.c_int), ("flags", C.c_uint), ("white", C.c_float),
                ("filmic", C.c_float * 5), ("reserved", C.c_uint)]


# rays from surface points (ptss_generate_rays_surface)
SURFACE_NORMAL, SURFACE_COSINE = 0, 1   # PTSS_SURFACE_NORMAL, PTSS_SURFACE_COSINE
SURFACE_BACK = 1                        # PTSS_SURFACE_BACK
SURFACE_TRIANGLE = 0x40000000           # PTSS_SURFACE_TRIANGLE


class SurfaceParams(C.Structure):   # ptss_surface_params
    _fields_ = [("structSize", C.c_uint), ("mode", C.c_int), ("maxDistance", C.c_float), ("reserved", C.c_uint)]


SURFACE_POINT_DTYPE = np.dtype([("surface", np.int32), ("a", np.float32), ("b", np.float32), ("flags", np.uint32)])   # ptss_surface_point
SPHERE_DTYPE = np.dtype([("position", np.float32, 3), ("radius", np.float32), ("materialIdx", np.int32)])             # ptss_sphere


# light maps read back (ptss_surface_atlas_blocks, ptss_lookup_lightmap)
LIGHTMAP_NEAREST, LIGHTMAP_BILINEAR = 0, 1     # PTSS_LIGHTMAP_NEAREST, PTSS_LIGHTMAP_BILINEAR
LIGHTMAP_MODULATE, LIGHTMAP_EMISSION = 1, 2    # PTSS_LIGHTMAP_MODULATE, PTSS_LIGHTMAP_EMISSION
SURFACE_BLOCK_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("width", np.int32), ("height", np.int32)])          # ptss_surface_block
MATERIAL_DTYPE = np.dtype({"names": ["diffuseColor", "specularColor", "absorption", "emmitance", "specularExponent", "indexOfRefraction",
                                     "diffAvg", "specAvg", "refrAvg", "roughness", "flags"],
                           "formats": [(np.float32, 3)] * 4 + [np.float32] * 6 + [np.int8],
                           "offsets": [0, 12, 24, 36, 48, 52, 56, 60, 64, 68, 72], "itemsize": 76})                           # ptss_material


class LightmapParams(C.Structure):   # ptss_lightmap_params
    _fields_ = [("structSize", C.c_uint), ("atlasWidth", C.c_int), ("atlasHeight", C.c_int), ("filter", C.c_int), ("flags", C.c_uint),
                ("firstTriangle", C.c_int), ("numTriangleBlocks", C.c_int), ("firstSphere", C.c_int), ("numSphereBlocks", C.c_int),
                ("reserved", C.c_uint)]


# ray queries that follow mirrors and glass (ptss_intersect_chain, ptss_lookup_lightmap_chain)
CHAIN_DTYPE = np.dtype([("throughput", np.float32, 3), ("steps", np.uint32), ("direction", np.float32, 3), ("pathLength", np.float32)])   # ptss_chain_result
CHAIN_LANE_PER_RAY, CHAIN_REFILL = 0, 1   # PTSS_CHAIN_*


class ChainOptions(C.Structure):   # ptss_chain_options: how ptss_intersect_chain schedules a batch
    _fields_ = [("structSize", C.c_uint), ("schedule", C.c_int), ("maxWorkgroups", C.c_int), ("reserved", C.c_int)]


assert CHAIN_DTYPE.itemsize == 32 and CHAIN_DTYPE.fields["steps"][1] == 12 and CHAIN_DTYPE.fields["pathLength"][1] == 28 and C.sizeof(ChainOptions) == 16


# The bits of ptss_launched_kernels: PTSS_KERNEL_<name> and PTSS_KERNEL_WIDTH_<name> of include/ptss_types.h as name: (first bit,
# bits owned). ptss.py names the instantiation behind every bit (KERNEL_OF_BIT).
KERNEL_BITS = {
    "BOUNCE": (0, 32),
    "FRAME": (32, 4),
    "BOUNCE_MESH": (40, 8),
    "QUERY": (48, 4),
    "FEATURES": (52, 2),
    "DENOISE": (54, 1),
    "UPDATE": (55, 1),
    "REFIT": (56, 1),
    "REPROJECT": (57, 1),
    "FEATURES_MOTION": (58, 2),
    "REPROJECT_MOTION": (60, 1),
}


class ReprojectParams(C.Structure):
    _fields_ = [("structSize", C.c_uint), ("cosNormal", C.c_float), ("depthTolerance", C.c_float), ("maxHistory", C.c_float),
                ("minCoverage", C.c_float)]


class UpsampleParams(C.Structure):
    _fields_ = [("structSize", C.c_uint), ("factor", C.c_int), ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float)]


# The 4-byte words of csrc/ptscene.h SceneLayout, in order (ptss.probe_pack_scene decodes the layout with this list). The five
# words of its union appear under both of their names: triClassPack0..4 (classed images) and the mesh image's dimensions.
SCENE_LAYOUT_FIELDS = ("numSpheres", "numTriangles", "numMaterials", "numPointLights", "numAreaLights", "offSphere", "offSphereMat",
                       "offTri", "offTriNormal", "offTriVert", "offMaterial", "offPointLight", "offAreaLight", "accelSpheres", "numChunks",
                       "offChunk", "offSphereOrig", "offSpherePos", "offQuant", "offPrimSphere", "offPrimTri", "offPrimChunk", "totalVec4",
                       "ldsVec4", "neeSkipSafe", "sphereBounded", "neePairs", "triDetBounded", "triClassed", "triClassPack0",
                       "triClassPack1", "triClassPack2", "triClassPack3", "triClassPack4", "offTriPos")
SCENE_LAYOUT_MESH_FIELDS = ("numLeaves", "numGroups", "offGroup", "offLeaf", "reserved")   # the same five words, as the mesh image reads them


assert C.sizeof(Sphere) == 20 and C.sizeof(Triangle) == 76 and C.sizeof(Material) == 76
assert C.sizeof(PointLight) == 24 and C.sizeof(AreaLight) == 32 and C.sizeof(Camera) == 40
assert C.sizeof(RayQuery) == 32 and C.sizeof(RayHit) == 48 and C.sizeof(PixelFeature) == 32 and C.sizeof(HistoryEntry) == 16
assert C.sizeof(PixelMotion) == 16 and PixelMotion.surface.offset == 12
assert C.sizeof(PathRng) == 24 == PATH_RNG_DTYPE.itemsize and PathRng.d.offset == 20 == PATH_RNG_DTYPE.fields["d"][1]
assert C.sizeof(PathResult) == 16 == PATH_RESULT_DTYPE.itemsize and PathResult.bounces.offset == 12 == PATH_RESULT_DTYPE.fields["bounces"][1]
assert C.sizeof(FilmCamera) == 68 and FilmCamera.camera.offset == 8 and FilmCamera.width.offset == 48 and FilmCamera.jitter.offset == 64
assert C.sizeof(FilmEntry) == 16 == FILM_DTYPE.itemsize and FilmEntry.samples.offset == 12 == FILM_DTYPE.fields["samples"][1]
assert C.sizeof(PlanParams) == 16 and PlanParams.threshold.offset == 12 and C.sizeof(PlanInfo) == 32 and PlanInfo.uniform.offset == 20
assert C.sizeof(LinearEntry) == 32 == LINEAR_DTYPE.itemsize and LinearEntry.samples.offset == 24 == LINEAR_DTYPE.fields["samples"][1]
assert LinearEntry.clamped.offset == 28 == LINEAR_DTYPE.fields["clamped"][1] and C.sizeof(LinearParams) == 20 and LinearParams.reserved.offset == 16
assert C.sizeof(FilmPosition) == 8 == POSITION_DTYPE.itemsize and C.sizeof(SplatFilter) == 20 and SplatFilter.reserved.offset == 16
assert C.sizeof(SplatEntry) == 32 == SPLAT_DTYPE.itemsize and SplatEntry.weight.offset == 24 == SPLAT_DTYPE.fields["weight"][1]
assert C.sizeof(MeterParams) == 32 and MeterParams.reserved.offset == 28 and C.sizeof(MeterState) == 48 == METER_STATE_DTYPE.itemsize
assert MeterState.metered.offset == 16 == METER_STATE_DTYPE.fields["metered"][1] and MeterState.sumLog.offset == 40 == METER_STATE_DTYPE.fields["sumLog"][1]
assert C.sizeof(GlareParams) == 24 and GlareParams.reserved.offset == 20 and C.sizeof(GlareLevel) == 16 and GLARE_DTYPE.itemsize == 32
assert C.sizeof(ToneParams) == 48 and ToneParams.white.offset == 20 and ToneParams.filmic.offset == 24 and ToneParams.reserved.offset == 44


def struct_to_dict(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out[name] = struct_to_dict(v)
        elif isinstance(v, bytes):
            out[name] = v[0] if v else 0
        else:
            out[name] = v
    return out
