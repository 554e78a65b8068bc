/* ptss_types.h — plain-C layouts of the scene/camera records that cross the drop-in boundary.
 *
 * Field order and sizes mirror the reference's host/device-shared structs so a maintainer can
 * hand the reference's std::vector<T>::data() straight to ptss_create():
 *   ptss_sphere      <- class Sphere      CudaTracer/Primitives.h:86-93       (20 B)
 *   ptss_triangle    <- class Triangle    CudaTracer/Primitives.h:6-16        (76 B)
 *   ptss_material    <- struct Material   CudaTracer/RenderStructs.h:80-107   (76 B, flags at 72)
 *   ptss_point_light <- struct PointLight CudaTracer/RenderStructs.h:56-63    (24 B)
 *   ptss_area_light  <- struct AreaLight  CudaTracer/RenderStructs.h:66-75    (32 B)
 *   ptss_camera      <- struct Camera     CudaTracer/RenderStructs.h:42-53    (40 B)
 *   ptss_uchar4      <- CUDA uchar4 (display pixel, RGBA)  CudaTracer/CudaTracer.cu:88-101
 * glm::vec3 is three packed floats; glm::quat is stored x,y,z,w (its constructor takes w first).
 */
#ifndef PTSS_TYPES_H
#define PTSS_TYPES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ptss_vec3 { float x, y, z; } ptss_vec3;
typedef struct ptss_quat { float x, y, z, w; } ptss_quat;
typedef struct ptss_uchar4 { unsigned char x, y, z, w; } ptss_uchar4;

typedef struct ptss_sphere {
    ptss_vec3 position;
    float radius;
    int materialIdx;
} ptss_sphere;

typedef struct ptss_triangle {
    ptss_vec3 vertex0, vertex1, vertex2;
    ptss_vec3 normal0, normal1, normal2;
    int materialIdx;
} ptss_triangle;

#define PTSS_MAT_FLAG_PURE_REFLECTION 0x01 /* RenderStructs.h:77 */
#define PTSS_MAT_FLAG_COOK_TORRANCE 0x03   /* RenderStructs.h:78 (overlaps bit 0 — kept literal) */

typedef struct ptss_material {
    ptss_vec3 diffuseColor;
    ptss_vec3 specularColor;
    ptss_vec3 absorption;
    ptss_vec3 emmitance; /* sic — reference spelling */
    float specularExponent;
    float indexOfRefraction;
    float diffAvg;
    float specAvg;
    float refrAvg;
    float roughness;
    char flags;
} ptss_material;

typedef struct ptss_point_light {
    ptss_vec3 position;
    ptss_vec3 power;
} ptss_point_light;

typedef struct ptss_area_light {
    ptss_vec3 power;
    float area;
    int triangleIdx;
    size_t numTriangles;
} ptss_area_light;

typedef struct ptss_camera {
    ptss_quat rotation;
    ptss_vec3 position;
    float zNear;
    float zFar;
    float fieldOfView;
} ptss_camera;

/* The five scene vectors of class Scene (CudaTracer/Scene.h:11-15), as uploaded verbatim by
 * main (CudaTracer/CudaTracer.cu:696-700), plus RendererData::defaultColor (CudaTracer.h:15). */
typedef struct ptss_scene_desc {
    const ptss_sphere* spheres;
    size_t numSpheres;
    const ptss_triangle* triangles;
    size_t numTriangles;
    const ptss_material* materials;
    size_t numMaterials;
    const ptss_point_light* pointLights;
    size_t numPointLights;
    const ptss_area_light* areaLights;
    size_t numAreaLights;
    ptss_vec3 defaultColor;
} ptss_scene_desc;

/* One ray of a batched query (ptss_intersect / ptss_occluded): two 16-byte rows. The direction is used as given (not
 * normalised); tmax is the initial `distance` of the reference's intersectScene loop (CudaTracer.cu:120-141). */
typedef struct ptss_ray_query {
    ptss_vec3 origin;
    float tmax;
    ptss_vec3 direction;
    float pad;
} ptss_ray_query;

/* The closest hit of one query: the reference's SurfaceElement (RenderStructs.h:110-121) plus what found it.
 * kind: 0 miss, 1 sphere, 2 triangle; primitive: index into the caller's spheres[] / triangles[]; w1, w2: the triangle's
 * weight[1], weight[2] (Primitives.h:58-60), 0 for spheres. A miss: distance = tmax, primitive = materialIdx = -1, the rest 0. */
typedef struct ptss_ray_hit {
    ptss_vec3 point;
    float distance;
    ptss_vec3 normal;
    int materialIdx;
    int kind;
    int primitive;
    float w1, w2;
} ptss_ray_hit;

#define PTSS_HIT_MISS 0
#define PTSS_HIT_SPHERE 1
#define PTSS_HIT_TRIANGLE 2

/* What the centre ray of one pixel hits first (ptss_render_features): 32 B = one memory sector, two 16-byte rows.
 * normal, depth, materialIdx: ptss_ray_hit.normal, .distance, .materialIdx of that ray; albedo: materials[materialIdx].diffuseColor.
 * A miss: normal 0, depth +inf, materialIdx -1, albedo = the scene's defaultColor. */
typedef struct ptss_pixel_feature {
    ptss_vec3 normal;
    float depth;
    ptss_vec3 albedo;
    int materialIdx;
} ptss_pixel_feature;

/* Parameters of ptss_denoise (ptss_default_denoise_params fills them in; DESIGN.md §3.17 has the weight functions). */
typedef struct ptss_denoise_params {
    unsigned int structSize; /* sizeof(ptss_denoise_params) as the caller compiled it */
    int levels;              /* A-trous passes, tap spacing 2^i in pass i: 0 (the display value, unfiltered) .. 6 */
    float sigmaColor;        /* colour tolerance of pass 0 on the 0..255 scale; halves with every pass */
    float sigmaNormal;       /* tolerance of 1 - cos(angle between the normals) */
    float sigmaDepth;        /* depth tolerance, in units of the depth change the local slope predicts for the tap's offset */
} ptss_denoise_params;

#define PTSS_DENOISE_MAX_LEVELS 6

/* One pixel of a reprojected history (ptss_reproject): 16 B, laid out as an entry of the denoiser's colour planes.
 * r, g, b: the colour on the display's 0..255 scale; weight: the effective number of samples per pixel behind it. */
typedef struct ptss_history_entry {
    float r, g, b;
    float weight;
} ptss_history_entry;

/* Parameters of ptss_reproject (ptss_default_reproject_params fills them in; DESIGN.md §3.19 has the formulas). */
typedef struct ptss_reproject_params {
    unsigned int structSize; /* sizeof(ptss_reproject_params) as the caller compiled it */
    float cosNormal;         /* a previous pixel counts only if its normal and the current one enclose at most this cosine: [-1, 1] */
    float depthTolerance;    /* ... and only if its depth is within this fraction of the reprojected point's distance: >= 0 */
    float maxHistory;        /* cap of the history's weight, in samples per pixel: >= 0 */
    float minCoverage;       /* bilinear weight the counting taps must reach together, else the history is dropped: [0, 1] */
} ptss_reproject_params;

/* Parameters of ptss_upsample (ptss_default_upsample_params fills them in; DESIGN.md §3.22 has the formulas). */
typedef struct ptss_upsample_params {
    unsigned int structSize; /* sizeof(ptss_upsample_params) as the caller compiled it */
    int factor;              /* hi-res pixels per lo-res pixel and axis: 1 .. 4 */
    float sigmaNormal;       /* tolerance of 1 - cos(angle between the normals): finite, > 0 */
    float sigmaDepth;        /* depth tolerance, in units of the depth change the hi-res slope predicts for the tap's offset: finite, > 0 */
} ptss_upsample_params;

#define PTSS_UPSAMPLE_MAX_FACTOR 4

/* Where the surface point under a pixel's centre was in the PREVIOUS pose (ptss_render_features_motion): one
 * 16-byte row. A miss: prevPoint 0, surface -1. */
typedef struct ptss_pixel_motion {
    ptss_vec3 prevPoint;
    int surface; /* -1 miss; k for sphere k; 0x40000000 | t for triangle t (the caller's indices) */
} ptss_pixel_motion;

#define PTSS_SURFACE_TRIANGLE 0x40000000

/* One random stream of a batched path query (ptss_seed_path_rng / ptss_trace_paths): the XORWOW state in the order
 * of ptss_read_rng_state. 24 B, 4-byte aligned. */
typedef struct ptss_path_rng {
    uint32_t v[5];
    uint32_t d;
} ptss_path_rng;

/* What ptss_trace_paths returns for one ray: one 16-byte row. radiance: the path's radiance0, linear (no tone map, no clamp; NaN and
 * inf as they come); bounces: the iterations the ray entered, 0 .. maxIterations. */
typedef struct ptss_path_result {
    ptss_vec3 radiance;
    uint32_t bounces;
} ptss_path_result;

/* How ptss_trace_paths_opt schedules a batch (ptss_default_path_options fills it in). */
#define PTSS_PATHS_LANE_PER_RAY 0 /* ptss_trace_paths' schedule: one lane per ray for the ray's whole life */
#define PTSS_PATHS_REFILL 1       /* a lane whose path has ended takes the next unclaimed ray of the batch */
typedef struct ptss_path_options {
    unsigned int structSize; /* sizeof(ptss_path_options) as the caller compiled it */
    int schedule;            /* PTSS_PATHS_* */
    int maxWorkgroups;       /* REFILL: cap on the grid, 0 = the library's choice (the resident workgroups); >= 0. Also the way to leave
                                part of the device to frames running beside the query. LANE_PER_RAY: not read */
    int reserved;            /* 0 */
} ptss_path_options;

/* The camera of a film (ptss_generate_rays): which model makes the eye ray of a film pixel, and from what.
 * kind: PTSS_FILM_*; camera: position and rotation for every model, zNear and fieldOfView for the pinhole and the thin lens only;
 * width, height: the film's own size, independent of any context's; lensRadius >= 0, focusDistance > 0: the thin lens only;
 * jitter: 1 draws the sample position (and the lens point) from the ray's stream, 0 draws nothing (pixel centre, lens centre). */
typedef struct ptss_film_camera {
    unsigned int structSize; /* sizeof(ptss_film_camera) as the caller compiled it */
    int kind;
    ptss_camera camera;
    int width, height;
    float lensRadius;
    float focusDistance;
    int jitter;
} ptss_film_camera;

#define PTSS_FILM_PINHOLE 0
#define PTSS_FILM_THIN_LENS 1
#define PTSS_FILM_EQUIRECT 2

/* One pixel of a film (ptss_accumulate_paths): the sums of the tone-mapped 8-bit samples (writeToPixelsKernel's totalPixelColors entry)
 * and how many there are. 16 B, 16-byte aligned access; a new film is all zero; samples < 2^24. */
typedef struct ptss_film_entry {
    uint32_t r, g, b;
    uint32_t samples;
} ptss_film_entry;

/* How ptss_plan_samples weighs a film pixel (ptss.h). minSamples >= 1: a pixel with fewer samples cannot be judged yet
 * and outranks every measured one; maxSamples in [minSamples, 2^23]: a pixel with that many gets no more; threshold >= 0, finite: the
 * standard error of the pixel's mean, in display steps (0..255), at or below which the pixel counts as converged. */
typedef struct ptss_plan_params {
    unsigned int structSize; /* sizeof(ptss_plan_params) as the caller compiled it */
    uint32_t minSamples;
    uint32_t maxSamples;
    float threshold;
} ptss_plan_params;

/* What a plan found (ptss_plan_samples writes it on the device). totalWeight: the sum of the weights, at most 2^50; activePixels: weight
 * > 0; unsampledPixels: below minSamples; cappedPixels: at or above maxSamples; uniform: 1 when the total was 0 and the budget was spread
 * evenly instead. 32 B, 8-byte aligned. */
typedef struct ptss_plan_info {
    unsigned long long totalWeight;
    uint32_t activePixels, unsampledPixels, cappedPixels, uniform;
    uint32_t reserved[2];
} ptss_plan_info;

/* One pixel of a linear film (ptss_accumulate_paths_linear): the sums of the samples' linear radiance as unsigned
 * fixed point with ptss_linear_params.scaleLog2 fraction bits, how many samples there are, and how many of them had a channel that was
 * NaN or above clampMax. 32 B, 16-byte aligned access; a new film is all zero; samples < 2^23 keeps the sums below 2^63. */
typedef struct ptss_linear_entry {
    unsigned long long r, g, b;
    uint32_t samples;
    uint32_t clamped;
} ptss_linear_entry;

/* How a linear film counts and shows radiance (ptss.h). scaleLog2 in [0, 32]: the fraction bits of the sums; clampMax > 0, finite, with
 * clampMax * 2^scaleLog2 <= 2^40: a channel above it counts as clampMax; exposure >= 0, finite: what ptss_resolve_linear multiplies the
 * mean by in front of the tone map (the linear means stay unexposed). */
typedef struct ptss_linear_params {
    unsigned int structSize; /* sizeof(ptss_linear_params) as the caller compiled it */
    int scaleLog2;
    float clampMax;
    float exposure;
    unsigned int reserved;   /* 0 */
} ptss_linear_params;

/* A pixel's luminance moments beside a linear film (ptss_accumulate_paths_linear_stats). y is the Rec. 709 luminance of a
 * sample's fixed-point channels (at most 2^40); sumY: the sum of y; sqLo, sqHi: the sums of y^2 & (2^40 - 1) and of y^2 >> 40, kept
 * apart because y^2 does not fit one word (the second moment is sqHi * 2^40 + sqLo); samples: how many. 32 B, 16-byte aligned access; a
 * new film is all zero; samples < 2^23 keeps every word below 2^64. */
typedef struct ptss_linear_moment {
    unsigned long long sumY, sqLo, sqHi, samples;
} ptss_linear_moment;

/* How ptss_plan_samples_linear weighs a pixel (ptss.h). minSamples, maxSamples: as in ptss_plan_params; threshold >= 0,
 * finite: the relative standard error of the pixel's mean luminance at or below which it counts as converged; floor: finite, in linear
 * radiance, added to the mean luminance under the error so that dark pixels do not outrank everything, with floor * 2^scaleLog2 >= 1 and
 * floor <= clampMax of the film's ptss_linear_params. */
typedef struct ptss_linear_plan_params {
    unsigned int structSize; /* sizeof(ptss_linear_plan_params) as the caller compiled it */
    uint32_t minSamples;
    uint32_t maxSamples;
    float threshold;
    float floor;
    uint32_t reserved[3];    /* 0 */
} ptss_linear_plan_params;

/* Where on the film a sample lies, in pixels (ptss_generate_rays_positions): pixel (i, j) owns [i, i + 1) x [j, j + 1),
 * its centre is (i + 0.5, j + 0.5). 8 B, 8-byte aligned access. */
typedef struct ptss_film_position {
    float x, y;
} ptss_film_position;

/* The reconstruction filter of a filtered linear film (ptss_splat_paths). kind: PTSS_SPLAT_*; radius in [0.5, 2], in
 * pixels: the filter is separable and zero from radius on; alpha > 0, finite: the Gaussian's exp(-alpha d^2) (the other kinds do not
 * read it). */
typedef struct ptss_splat_filter {
    unsigned int structSize; /* sizeof(ptss_splat_filter) as the caller compiled it */
    int kind;
    float radius;
    float alpha;
    unsigned int reserved;   /* 0 */
} ptss_splat_filter;

#define PTSS_SPLAT_BOX 0
#define PTSS_SPLAT_TENT 1
#define PTSS_SPLAT_GAUSSIAN 2

/* One pixel of a filtered linear film: the weighted sums of the samples' fixed-point radiance (ptss_linear_params.scaleLog2 fraction
 * bits) and the sum of the weights, a weight of 1 being 65536. 32 B, 16-byte aligned access; a new film is all zero; fewer than 2^23
 * taps per pixel keep the sums below 2^63. */
typedef struct ptss_splat_entry {
    unsigned long long r, g, b;
    unsigned long long weight;
} ptss_splat_entry;

/* Metering a linear or a filtered linear film (ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure). A histogram
 * is PTSS_METER_BINS 32-bit counts, zero-filled by the caller: bin 0 counts black pixels, bin 1 + 8 e + sub the pixels whose fixed-point
 * luminance Y has floor(log2 Y) = e (0 .. 40) and whose next three bits are sub: an eighth of a stop per bin. */
#define PTSS_METER_BINS 329

/* How a histogram becomes an exposure (ptss.h). key > 0, finite: the exposed mean luminance aimed at; lowPermille, highPermille, at most
 * 999 together: the darkest and brightest thousandths of the non-black pixels left out of the mean; rate in [0, 1]: the share of the way
 * towards the target one update goes (1: all of it); 0 <= minExposure <= maxExposure, finite: what target and exposure are clamped to. */
typedef struct ptss_meter_params {
    unsigned int structSize; /* sizeof(ptss_meter_params) as the caller compiled it */
    float key;
    unsigned int lowPermille;
    unsigned int highPermille;
    float rate;
    float minExposure;
    float maxExposure;
    unsigned int reserved;   /* 0 */
} ptss_meter_params;

/* The state of a meter, in device memory (ptss_meter_exposure reads and writes it, the metered resolves read exposure). 48 B, 8-byte
 * aligned access; all zero = new. exposure: what the metered resolves multiply by; target: the exposure the latest histogram asked for;
 * meanLog2: the mean log2 luminance it found; updates: the updates so far, saturating. The integers of the latest update: metered = the
 * non-black pixels counted (T), black = bin 0, counted = the ranks the percentile cuts left (C), sumLog = their bin centres summed, in
 * 1/16 stop. */
typedef struct ptss_meter_state {
    float exposure, target, meanLog2;
    uint32_t updates;
    unsigned long long metered, black, counted, sumLog;
} ptss_meter_state;

/* Glare for the two linear films (ptss_glare_build and the glare resolves): a pyramid of rounded integer averages of
 * what a film's integer pixel means hold above a threshold, added to or mixed with the means in front of the tone map. */
#define PTSS_GLARE_MAX_LEVELS 8
#define PTSS_GLARE_ADD 0          /* m' = m + strength * g */
#define PTSS_GLARE_MIX 1          /* m' = (1 - strength) * m + strength * g */
#define PTSS_GLARE_FILM_LINEAR 0  /* the film is ptss_linear_entry */
#define PTSS_GLARE_FILM_SPLAT 1   /* the film is ptss_splat_entry */

/* levels in [1, 8]: the pyramid's levels, each half the one below, rounded up; mode: PTSS_GLARE_*; threshold >= 0, finite, in the film's
 * radiance units with threshold * 2^scaleLog2 <= 2^40: what is taken off every channel of a mean (what is left, never negative, is the
 * pyramid's source); strength in [0, 1]: 0 leaves the plain resolve's bytes. */
typedef struct ptss_glare_params {
    unsigned int structSize; /* sizeof(ptss_glare_params) as the caller compiled it */
    int levels;
    int mode;
    float threshold;
    float strength;
    unsigned int reserved;   /* 0 */
} ptss_glare_params;

/* One texel of a glare pyramid, in the film's fixed point. 32 B, 16-byte aligned access; the fourth word is always written as 0. */
typedef struct ptss_glare_entry {
    unsigned long long r, g, b;
    unsigned long long zero;
} ptss_glare_entry;

/* Where level k (1 .. levels; out[k - 1]) of a pyramid lies: width x height entries in rows, the first at entry `first` (ptss_glare_layout). */
typedef struct ptss_glare_level {
    int width, height;
    unsigned long long first;
} ptss_glare_level;

/* Denoising a linear or a filtered linear film in linear light (ptss_denoise_linear). The film's kind is one of
 * PTSS_GLARE_FILM_*; the two names below say the same without the glare. levels in [0, PTSS_DENOISE_MAX_LEVELS]: A-trous passes, tap
 * spacing 2^i in pass i (0: the film's means, unfiltered); sigmaLuminance: the luminance tolerance in units of the pixel's measured
 * standard error (it does not halve per pass); sigmaNormal, sigmaDepth: as in ptss_denoise_params. All three finite and positive. */
#define PTSS_FILM_LINEAR PTSS_GLARE_FILM_LINEAR
#define PTSS_FILM_SPLAT PTSS_GLARE_FILM_SPLAT
typedef struct ptss_denoise_linear_params {
    unsigned int structSize; /* sizeof(ptss_denoise_linear_params) as the caller compiled it */
    int levels;
    float sigmaLuminance;
    float sigmaNormal;
    float sigmaDepth;
    uint32_t reserved[3];    /* 0 */
} ptss_denoise_linear_params;

/* Carrying a linear or a filtered linear film across a camera move (ptss_reproject_linear). cosNormal, depthTolerance,
 * minCoverage: as in ptss_reproject_params; maxHistory: the cap of the history count K a seeded pixel starts with. */
typedef struct ptss_reproject_linear_params {
    unsigned int structSize; /* sizeof(ptss_reproject_linear_params) as the caller compiled it */
    float cosNormal;         /* [-1, 1]                       default 0.9  */
    float depthTolerance;    /* finite, >= 0                  default 0.02 */
    float minCoverage;       /* [0, 1]                        default 0.25 */
    uint32_t maxHistory;     /* 1 .. 2^23 - 1: cap of K       default 64   */
    unsigned int reserved;   /* 0 */
} ptss_reproject_linear_params;

/* What ptss_reproject_linear counts, written with integer adds: the caller zero-fills. 32 B, 8-byte aligned. seeded + offFilm + noTap
 * is the number of pixels of the new film. */
typedef struct ptss_reproject_linear_info {
    unsigned long long seeded;     /* pixels that got K >= 1 */
    unsigned long long offFilm;    /* projection rejected: behind the previous camera, outside its film, not finite */
    unsigned long long noTap;      /* on the film, but no tap counted or coverage below minCoverage: disoccluded, other material, empty history */
    unsigned long long noVariance; /* seeded, moments asked for, but no counting tap had a moment row of N >= 2 */
} ptss_reproject_linear_info;

/* Upsampling a linear or a filtered linear film in linear light (ptss_upsample_linear). factor, sigmaNormal,
 * sigmaDepth: as in ptss_upsample_params. PTSS_UPSAMPLE_LINEAR_WRAP_X: the film is an equirect one, its columns wrap at the seam. */
#define PTSS_UPSAMPLE_LINEAR_WRAP_X 1u
typedef struct ptss_upsample_linear_params {
    unsigned int structSize; /* sizeof(ptss_upsample_linear_params) as the caller compiled it */
    int factor;              /* hi pixels per lo pixel and axis: 1 .. 4   default 2   */
    float sigmaNormal;       /* finite, > 0                               default 0.1 */
    float sigmaDepth;        /* finite, > 0                               default 4   */
    unsigned int flags;      /* PTSS_UPSAMPLE_LINEAR_*                    default 0   */
    unsigned int reserved;   /* 0 */
} ptss_upsample_linear_params;

/* What ptss_upsample_linear counts, written with integer adds: the caller zero-fills. 24 B, 8-byte aligned. The three sum to the
 * number of pixels of the large film. */
typedef struct ptss_upsample_linear_info {
    unsigned long long filtered; /* hi pixels with at least one counted tap */
    unsigned long long fallback; /* no tap counted: the row of the nearest lo pixel's means */
    unsigned long long empty;    /* no tap counted and the nearest lo pixel is empty: an all-zero row */
} ptss_upsample_linear_info;

/* Tone curves for the two linear films (ptss_tone_build, ptss_resolve_toned; csrc/pttone.h): a curve, a transfer
 * function and a bit depth, evaluated once into a table of thresholds that the resolve searches. white: PTSS_TONE_REINHARD only, the input
 * that reaches display white, finite, in (0, 65536] with 1 / white^2 finite in float32. filmic[5] = a, b, c, d, e of
 * x (a x + b) / (x (c x + d) + e), PTSS_TONE_FILMIC only: finite, >= 0, e > 0, and such that the curve is a number at the saturation
 * bound 2^40 (csrc/pttone.h). PTSS_TONE_LUMINANCE: the curve moves the luminance and the channels follow it, keeping their ratios. */
#define PTSS_TONE_CLAMP 0
#define PTSS_TONE_REINHARD 1
#define PTSS_TONE_FILMIC 2
#define PTSS_TRANSFER_GAMMA22 0
#define PTSS_TRANSFER_SRGB 1
#define PTSS_TONE_LUMINANCE 1u
typedef struct ptss_tone_params {
    unsigned int structSize; /* sizeof(ptss_tone_params) as the caller compiled it */
    int curve;               /* PTSS_TONE_*                  default PTSS_TONE_FILMIC   */
    int transfer;            /* PTSS_TRANSFER_*              default PTSS_TRANSFER_SRGB */
    int bits;                /* 8 or 10                      default 8                  */
    unsigned int flags;      /* PTSS_TONE_LUMINANCE          default 0                  */
    float white;             /*                              default 4                  */
    float filmic[5];         /*                              default 2.51, 0.03, 2.43, 0.59, 0.14 */
    unsigned int reserved;   /* 0 */
} ptss_tone_params;

/* Rays from points on the scene's own surfaces (ptss_generate_rays_surface; csrc/ptsurface.h): a light-map texel, a
 * probe on a wall. surface: ptss_pixel_motion::surface's encoding — sphere k is k, triangle t is PTSS_SURFACE_TRIANGLE | t, both the
 * caller's indices. a, b: on a triangle the weights w1, w2 of a ptss_ray_hit (a >= 0, b >= 0, a + b <= 1 as float32 rounds the sum); on
 * a sphere unit fractions of longitude and latitude as on an equirect film (both in [0, 1]). flags: PTSS_SURFACE_BACK — the ray leaves
 * from the other side (the normal negated); every other bit 0. 16 B, 16-byte aligned access. */
#define PTSS_SURFACE_BACK 1u
typedef struct ptss_surface_point {
    int surface;
    float a, b;
    uint32_t flags;
} ptss_surface_point;

/* How ptss_generate_rays_surface makes the ray of a point. PTSS_SURFACE_NORMAL: along the normal, no draw; PTSS_SURFACE_COSINE: two
 * draws from the ray's stream, cosine-weighted about the normal (the reference's Lambert sampler). maxDistance > 0, +inf allowed: every
 * ray's tmax (ptss_trace_paths ignores it; with ptss_occluded a finite one makes ambient-occlusion rays). */
#define PTSS_SURFACE_NORMAL 0
#define PTSS_SURFACE_COSINE 1
typedef struct ptss_surface_params {
    unsigned int structSize; /* sizeof(ptss_surface_params) as the caller compiled it */
    int mode;                /* PTSS_SURFACE_NORMAL or PTSS_SURFACE_COSINE */
    float maxDistance;       /* > 0 */
    unsigned int reserved;   /* 0 */
} ptss_surface_params;

/* Where a primitive's texels lie in a light map's atlas (ptss_surface_atlas_blocks, ptss_lookup_lightmap): the block's
 * lower-left texel and its extent. width == 0: the primitive has no block. 16 B, one row, 16-byte aligned access. */
typedef struct ptss_surface_block {
    int x, y, width, height;
} ptss_surface_block;

/* How ptss_lookup_lightmap reads a baked map (csrc/ptlightmap.h). atlasWidth x atlasHeight: the map's sides, both >= 1,
 * their product below 2^31. filter: the nearest texel or four taps with integer weights. flags: PTSS_LIGHTMAP_MODULATE multiplies the
 * looked-up mean by the hit's diffuseColor (the radiance a Lambert surface sends out), PTSS_LIGHTMAP_EMISSION adds the hit's emmitance.
 * Block table row k of the triangles belongs to the caller's triangle firstTriangle + k, k < numTriangleBlocks; the spheres alike. */
#define PTSS_LIGHTMAP_NEAREST 0
#define PTSS_LIGHTMAP_BILINEAR 1
#define PTSS_LIGHTMAP_MODULATE 1u
#define PTSS_LIGHTMAP_EMISSION 2u
typedef struct ptss_lightmap_params {
    unsigned int structSize; /* sizeof(ptss_lightmap_params) as the caller compiled it */
    int atlasWidth, atlasHeight;
    int filter;              /* PTSS_LIGHTMAP_NEAREST or PTSS_LIGHTMAP_BILINEAR    default PTSS_LIGHTMAP_BILINEAR */
    unsigned int flags;      /* PTSS_LIGHTMAP_MODULATE | PTSS_LIGHTMAP_EMISSION    default 0 */
    int firstTriangle, numTriangleBlocks;
    int firstSphere, numSphereBlocks;
    unsigned int reserved;   /* 0 */
} ptss_lightmap_params;

/* What ptss_intersect_chain returns for one ray beside the hit (csrc/ptspecular.h): two 16-byte rows. throughput:
 * (1, 1, 1) times the factor of every followed link, in chain order, component by component in float32 (ptsp::linkFactor: the
 * followed lobe's probability times its weight in the reference's scatter); steps: the links followed, 0 .. maxSteps; direction: of
 * the last link's ray (the caller's own for steps == 0); pathLength: the float32 sum of the chain's hit distances in chain order,
 * +inf when the chain ends in a miss. */
typedef struct ptss_chain_result {
    ptss_vec3 throughput;
    unsigned int steps;
    ptss_vec3 direction;
    float pathLength;
} ptss_chain_result;

/* How ptss_intersect_chain schedules a batch (ptss_default_chain_options fills it in). */
#define PTSS_CHAIN_LANE_PER_RAY 0 /* one lane per ray for the chain's whole life */
#define PTSS_CHAIN_REFILL 1       /* a lane whose chain has ended takes the next unclaimed ray of the batch */
typedef struct ptss_chain_options {
    unsigned int structSize; /* sizeof(ptss_chain_options) as the caller compiled it */
    int schedule;            /* PTSS_CHAIN_* */
    int maxWorkgroups;       /* REFILL: cap on the grid, 0 = the library's choice (the resident workgroups); >= 0. LANE_PER_RAY: not read */
    int reserved;            /* 0 */
} ptss_chain_options;

/* The bits of ptss_launched_kernels (ptss.h): every kernel owns the range [PTSS_KERNEL_x, PTSS_KERNEL_x + PTSS_KERNEL_WIDTH_x).
 * Inside a range: the bounce kernels variant*8 + last*4 + inLds*2 + first (variant 0 many-sphere chunks, 1 bounded sphere test with
 * paired shadow segments, 2 bounded sphere test, 3 the reference's sphere test; the mesh image's eight have a range of their own
 * and no frame kernel), the frame kernels their variant, the query kernel any*2 + inLds, the feature kernels inLds.
 * cuda-path-tracer-ss_amd/ptss_types.py mirrors the table; a new kernel takes bits from the free ones (36-39, 61-63). */
enum ptss_kernel_bit {
    PTSS_KERNEL_BOUNCE = 0,            /* bounceKernel of the four variants that also have a frame kernel */
    PTSS_KERNEL_FRAME = 32,            /* frameKernel: a whole frame in one launch */
    PTSS_KERNEL_BOUNCE_MESH = 40,      /* bounceKernel of the mesh image */
    PTSS_KERNEL_QUERY = 48,            /* queryKernel (ptss_intersect, ptss_occluded) */
    PTSS_KERNEL_FEATURES = 52,         /* featureKernel (ptss_render_features) */
    PTSS_KERNEL_DENOISE = 54,          /* denoiseKernel (ptss_denoise, ptss_denoise_history) */
    PTSS_KERNEL_UPDATE = 55,           /* sceneUpdateKernel (ptss_update_triangles) */
    PTSS_KERNEL_REFIT = 56,            /* meshRefitKernel (ptss_update_triangles on a mesh image) */
    PTSS_KERNEL_REPROJECT = 57,        /* reprojectKernel (ptss_reproject) */
    PTSS_KERNEL_FEATURES_MOTION = 58,  /* featureKernel with motion rows (ptss_render_features_motion) */
    PTSS_KERNEL_REPROJECT_MOTION = 60  /* reprojectKernel reading motion rows (ptss_reproject_motion) */
};
enum ptss_kernel_width {
    PTSS_KERNEL_WIDTH_BOUNCE = 32,
    PTSS_KERNEL_WIDTH_FRAME = 4,
    PTSS_KERNEL_WIDTH_BOUNCE_MESH = 8,
    PTSS_KERNEL_WIDTH_QUERY = 4,
    PTSS_KERNEL_WIDTH_FEATURES = 2,
    PTSS_KERNEL_WIDTH_DENOISE = 1,
    PTSS_KERNEL_WIDTH_UPDATE = 1,
    PTSS_KERNEL_WIDTH_REFIT = 1,
    PTSS_KERNEL_WIDTH_REPROJECT = 1,
    PTSS_KERNEL_WIDTH_FEATURES_MOTION = 2,
    PTSS_KERNEL_WIDTH_REPROJECT_MOTION = 1
};

#if defined(__cplusplus)
static_assert(sizeof(ptss_ray_query) == 32 && offsetof(ptss_ray_query, tmax) == 12 && offsetof(ptss_ray_query, direction) == 16,
              "ptss_ray_query is two 16-byte rows");
static_assert(sizeof(ptss_ray_hit) == 48 && offsetof(ptss_ray_hit, distance) == 12 && offsetof(ptss_ray_hit, normal) == 16 &&
                  offsetof(ptss_ray_hit, materialIdx) == 28 && offsetof(ptss_ray_hit, kind) == 32 &&
                  offsetof(ptss_ray_hit, primitive) == 36 && offsetof(ptss_ray_hit, w1) == 40 && offsetof(ptss_ray_hit, w2) == 44,
              "ptss_ray_hit is three 16-byte rows");
static_assert(sizeof(ptss_pixel_feature) == 32 && offsetof(ptss_pixel_feature, depth) == 12 && offsetof(ptss_pixel_feature, albedo) == 16 &&
                  offsetof(ptss_pixel_feature, materialIdx) == 28,
              "ptss_pixel_feature is two 16-byte rows");
static_assert(sizeof(ptss_history_entry) == 16 && offsetof(ptss_history_entry, weight) == 12, "ptss_history_entry is one 16-byte row");
static_assert(sizeof(ptss_pixel_motion) == 16 && offsetof(ptss_pixel_motion, surface) == 12, "ptss_pixel_motion is one 16-byte row");
static_assert(sizeof(ptss_path_rng) == 24 && offsetof(ptss_path_rng, d) == 20, "ptss_path_rng is six 32-bit words: v[0..4], d");
static_assert(sizeof(ptss_path_result) == 16 && offsetof(ptss_path_result, bounces) == 12, "ptss_path_result is one 16-byte row");
static_assert(sizeof(ptss_film_camera) == 68 && offsetof(ptss_film_camera, camera) == 8 && offsetof(ptss_film_camera, width) == 48 &&
                  offsetof(ptss_film_camera, lensRadius) == 56 && offsetof(ptss_film_camera, jitter) == 64,
              "ptss_film_camera is seventeen 32-bit words");
static_assert(sizeof(ptss_film_entry) == 16 && offsetof(ptss_film_entry, samples) == 12, "ptss_film_entry is one 16-byte row");
static_assert(sizeof(ptss_path_options) == 16 && offsetof(ptss_path_options, schedule) == 4 && offsetof(ptss_path_options, maxWorkgroups) == 8 &&
                  offsetof(ptss_path_options, reserved) == 12,
              "ptss_path_options is four 32-bit words");
static_assert(sizeof(ptss_plan_params) == 16 && offsetof(ptss_plan_params, minSamples) == 4 && offsetof(ptss_plan_params, threshold) == 12,
              "ptss_plan_params is four 32-bit words");
static_assert(sizeof(ptss_plan_info) == 32 && offsetof(ptss_plan_info, activePixels) == 8 && offsetof(ptss_plan_info, uniform) == 20 &&
                  offsetof(ptss_plan_info, reserved) == 24,
              "ptss_plan_info is four 64-bit words");
static_assert(sizeof(ptss_linear_entry) == 32 && offsetof(ptss_linear_entry, g) == 8 && offsetof(ptss_linear_entry, samples) == 24 &&
                  offsetof(ptss_linear_entry, clamped) == 28,
              "ptss_linear_entry is two 16-byte rows");
static_assert(sizeof(ptss_linear_params) == 20 && offsetof(ptss_linear_params, scaleLog2) == 4 && offsetof(ptss_linear_params, clampMax) == 8 &&
                  offsetof(ptss_linear_params, exposure) == 12 && offsetof(ptss_linear_params, reserved) == 16,
              "ptss_linear_params is five 32-bit words");
static_assert(sizeof(ptss_linear_moment) == 32 && offsetof(ptss_linear_moment, sqLo) == 8 && offsetof(ptss_linear_moment, samples) == 24,
              "ptss_linear_moment is two 16-byte rows");
static_assert(sizeof(ptss_linear_plan_params) == 32 && offsetof(ptss_linear_plan_params, threshold) == 12 &&
                  offsetof(ptss_linear_plan_params, floor) == 16 && offsetof(ptss_linear_plan_params, reserved) == 20,
              "ptss_linear_plan_params is eight 32-bit words");
static_assert(sizeof(ptss_film_position) == 8 && offsetof(ptss_film_position, y) == 4, "ptss_film_position is two floats");
static_assert(sizeof(ptss_splat_filter) == 20 && offsetof(ptss_splat_filter, kind) == 4 && offsetof(ptss_splat_filter, radius) == 8 &&
                  offsetof(ptss_splat_filter, alpha) == 12 && offsetof(ptss_splat_filter, reserved) == 16,
              "ptss_splat_filter is five 32-bit words");
static_assert(sizeof(ptss_splat_entry) == 32 && offsetof(ptss_splat_entry, g) == 8 && offsetof(ptss_splat_entry, weight) == 24,
              "ptss_splat_entry is two 16-byte rows");
static_assert(sizeof(ptss_meter_params) == 32 && offsetof(ptss_meter_params, key) == 4 && offsetof(ptss_meter_params, rate) == 16 &&
                  offsetof(ptss_meter_params, maxExposure) == 24 && offsetof(ptss_meter_params, reserved) == 28,
              "ptss_meter_params is eight 32-bit words");
static_assert(sizeof(ptss_meter_state) == 48 && offsetof(ptss_meter_state, updates) == 12 && offsetof(ptss_meter_state, metered) == 16 &&
                  offsetof(ptss_meter_state, sumLog) == 40,
              "ptss_meter_state is four 32-bit and four 64-bit words");
static_assert(sizeof(ptss_glare_params) == 24 && offsetof(ptss_glare_params, levels) == 4 && offsetof(ptss_glare_params, threshold) == 12 &&
                  offsetof(ptss_glare_params, reserved) == 20,
              "ptss_glare_params is six 32-bit words");
static_assert(sizeof(ptss_glare_entry) == 32 && offsetof(ptss_glare_entry, g) == 8 && offsetof(ptss_glare_entry, zero) == 24,
              "ptss_glare_entry is two 16-byte rows");
static_assert(sizeof(ptss_glare_level) == 16 && offsetof(ptss_glare_level, height) == 4 && offsetof(ptss_glare_level, first) == 8,
              "ptss_glare_level is two 32-bit words and one 64-bit word");
static_assert(sizeof(ptss_denoise_linear_params) == 32 && offsetof(ptss_denoise_linear_params, levels) == 4 &&
                  offsetof(ptss_denoise_linear_params, sigmaLuminance) == 8 && offsetof(ptss_denoise_linear_params, sigmaDepth) == 16 &&
                  offsetof(ptss_denoise_linear_params, reserved) == 20,
              "ptss_denoise_linear_params is eight 32-bit words");
static_assert(sizeof(ptss_reproject_linear_params) == 24 && offsetof(ptss_reproject_linear_params, cosNormal) == 4 &&
                  offsetof(ptss_reproject_linear_params, minCoverage) == 12 && offsetof(ptss_reproject_linear_params, maxHistory) == 16 &&
                  offsetof(ptss_reproject_linear_params, reserved) == 20,
              "ptss_reproject_linear_params is six 32-bit words");
static_assert(sizeof(ptss_reproject_linear_info) == 32 && offsetof(ptss_reproject_linear_info, offFilm) == 8 &&
                  offsetof(ptss_reproject_linear_info, noVariance) == 24,
              "ptss_reproject_linear_info is four 64-bit words");
static_assert(sizeof(ptss_upsample_linear_params) == 24 && offsetof(ptss_upsample_linear_params, factor) == 4 &&
                  offsetof(ptss_upsample_linear_params, sigmaDepth) == 12 && offsetof(ptss_upsample_linear_params, flags) == 16 &&
                  offsetof(ptss_upsample_linear_params, reserved) == 20,
              "ptss_upsample_linear_params is six 32-bit words");
static_assert(sizeof(ptss_upsample_linear_info) == 24 && offsetof(ptss_upsample_linear_info, fallback) == 8 &&
                  offsetof(ptss_upsample_linear_info, empty) == 16,
              "ptss_upsample_linear_info is three 64-bit words");
static_assert(sizeof(ptss_tone_params) == 48 && offsetof(ptss_tone_params, curve) == 4 && offsetof(ptss_tone_params, bits) == 12 &&
                  offsetof(ptss_tone_params, white) == 20 && offsetof(ptss_tone_params, filmic) == 24 && offsetof(ptss_tone_params, reserved) == 44,
              "ptss_tone_params is twelve 32-bit words");
static_assert(sizeof(ptss_surface_point) == 16 && offsetof(ptss_surface_point, a) == 4 && offsetof(ptss_surface_point, b) == 8 &&
                  offsetof(ptss_surface_point, flags) == 12,
              "ptss_surface_point is one 16-byte row");
static_assert(sizeof(ptss_surface_params) == 16 && offsetof(ptss_surface_params, mode) == 4 && offsetof(ptss_surface_params, maxDistance) == 8 &&
                  offsetof(ptss_surface_params, reserved) == 12,
              "ptss_surface_params is four 32-bit words");
static_assert(sizeof(ptss_surface_block) == 16 && offsetof(ptss_surface_block, y) == 4 && offsetof(ptss_surface_block, width) == 8 &&
                  offsetof(ptss_surface_block, height) == 12,
              "ptss_surface_block is one 16-byte row");
static_assert(sizeof(ptss_chain_result) == 32 && offsetof(ptss_chain_result, steps) == 12 && offsetof(ptss_chain_result, direction) == 16 &&
                  offsetof(ptss_chain_result, pathLength) == 28,
              "ptss_chain_result is two 16-byte rows");
static_assert(sizeof(ptss_chain_options) == 16 && offsetof(ptss_chain_options, schedule) == 4 && offsetof(ptss_chain_options, maxWorkgroups) == 8 &&
                  offsetof(ptss_chain_options, reserved) == 12,
              "ptss_chain_options is four 32-bit words");
static_assert(sizeof(ptss_lightmap_params) == 40 && offsetof(ptss_lightmap_params, atlasWidth) == 4 && offsetof(ptss_lightmap_params, filter) == 12 &&
                  offsetof(ptss_lightmap_params, flags) == 16 && offsetof(ptss_lightmap_params, firstTriangle) == 20 &&
                  offsetof(ptss_lightmap_params, firstSphere) == 28 && offsetof(ptss_lightmap_params, reserved) == 36,
              "ptss_lightmap_params is ten 32-bit words");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(ptss_ray_query) == 32 && offsetof(ptss_ray_query, tmax) == 12 && offsetof(ptss_ray_query, direction) == 16,
               "ptss_ray_query is two 16-byte rows");
_Static_assert(sizeof(ptss_ray_hit) == 48 && offsetof(ptss_ray_hit, distance) == 12 && offsetof(ptss_ray_hit, normal) == 16 &&
                   offsetof(ptss_ray_hit, materialIdx) == 28 && offsetof(ptss_ray_hit, kind) == 32 &&
                   offsetof(ptss_ray_hit, primitive) == 36 && offsetof(ptss_ray_hit, w1) == 40 && offsetof(ptss_ray_hit, w2) == 44,
               "ptss_ray_hit is three 16-byte rows");
_Static_assert(sizeof(ptss_pixel_feature) == 32 && offsetof(ptss_pixel_feature, depth) == 12 && offsetof(ptss_pixel_feature, albedo) == 16 &&
                   offsetof(ptss_pixel_feature, materialIdx) == 28,
               "ptss_pixel_feature is two 16-byte rows");
_Static_assert(sizeof(ptss_history_entry) == 16 && offsetof(ptss_history_entry, weight) == 12, "ptss_history_entry is one 16-byte row");
_Static_assert(sizeof(ptss_pixel_motion) == 16 && offsetof(ptss_pixel_motion, surface) == 12, "ptss_pixel_motion is one 16-byte row");
_Static_assert(sizeof(ptss_path_rng) == 24 && offsetof(ptss_path_rng, d) == 20, "ptss_path_rng is six 32-bit words: v[0..4], d");
_Static_assert(sizeof(ptss_path_result) == 16 && offsetof(ptss_path_result, bounces) == 12, "ptss_path_result is one 16-byte row");
_Static_assert(sizeof(ptss_film_camera) == 68 && offsetof(ptss_film_camera, camera) == 8 && offsetof(ptss_film_camera, width) == 48 &&
                   offsetof(ptss_film_camera, lensRadius) == 56 && offsetof(ptss_film_camera, jitter) == 64,
               "ptss_film_camera is seventeen 32-bit words");
_Static_assert(sizeof(ptss_film_entry) == 16 && offsetof(ptss_film_entry, samples) == 12, "ptss_film_entry is one 16-byte row");
_Static_assert(sizeof(ptss_path_options) == 16 && offsetof(ptss_path_options, schedule) == 4 && offsetof(ptss_path_options, maxWorkgroups) == 8 &&
                   offsetof(ptss_path_options, reserved) == 12,
               "ptss_path_options is four 32-bit words");
_Static_assert(sizeof(ptss_plan_params) == 16 && offsetof(ptss_plan_params, minSamples) == 4 && offsetof(ptss_plan_params, threshold) == 12,
               "ptss_plan_params is four 32-bit words");
_Static_assert(sizeof(ptss_plan_info) == 32 && offsetof(ptss_plan_info, activePixels) == 8 && offsetof(ptss_plan_info, uniform) == 20 &&
                   offsetof(ptss_plan_info, reserved) == 24,
               "ptss_plan_info is four 64-bit words");
_Static_assert(sizeof(ptss_linear_entry) == 32 && offsetof(ptss_linear_entry, g) == 8 && offsetof(ptss_linear_entry, samples) == 24 &&
                   offsetof(ptss_linear_entry, clamped) == 28,
               "ptss_linear_entry is two 16-byte rows");
_Static_assert(sizeof(ptss_linear_params) == 20 && offsetof(ptss_linear_params, scaleLog2) == 4 && offsetof(ptss_linear_params, clampMax) == 8 &&
                   offsetof(ptss_linear_params, exposure) == 12 && offsetof(ptss_linear_params, reserved) == 16,
               "ptss_linear_params is five 32-bit words");
_Static_assert(sizeof(ptss_linear_moment) == 32 && offsetof(ptss_linear_moment, sqLo) == 8 && offsetof(ptss_linear_moment, samples) == 24,
               "ptss_linear_moment is two 16-byte rows");
_Static_assert(sizeof(ptss_linear_plan_params) == 32 && offsetof(ptss_linear_plan_params, threshold) == 12 &&
                   offsetof(ptss_linear_plan_params, floor) == 16 && offsetof(ptss_linear_plan_params, reserved) == 20,
               "ptss_linear_plan_params is eight 32-bit words");
_Static_assert(sizeof(ptss_film_position) == 8 && offsetof(ptss_film_position, y) == 4, "ptss_film_position is two floats");
_Static_assert(sizeof(ptss_splat_filter) == 20 && offsetof(ptss_splat_filter, kind) == 4 && offsetof(ptss_splat_filter, radius) == 8 &&
                   offsetof(ptss_splat_filter, alpha) == 12 && offsetof(ptss_splat_filter, reserved) == 16,
               "ptss_splat_filter is five 32-bit words");
_Static_assert(sizeof(ptss_splat_entry) == 32 && offsetof(ptss_splat_entry, g) == 8 && offsetof(ptss_splat_entry, weight) == 24,
               "ptss_splat_entry is two 16-byte rows");
_Static_assert(sizeof(ptss_meter_params) == 32 && offsetof(ptss_meter_params, key) == 4 && offsetof(ptss_meter_params, rate) == 16 &&
                   offsetof(ptss_meter_params, maxExposure) == 24 && offsetof(ptss_meter_params, reserved) == 28,
               "ptss_meter_params is eight 32-bit words");
_Static_assert(sizeof(ptss_meter_state) == 48 && offsetof(ptss_meter_state, updates) == 12 && offsetof(ptss_meter_state, metered) == 16 &&
                   offsetof(ptss_meter_state, sumLog) == 40,
               "ptss_meter_state is four 32-bit and four 64-bit words");
_Static_assert(sizeof(ptss_glare_params) == 24 && offsetof(ptss_glare_params, levels) == 4 && offsetof(ptss_glare_params, threshold) == 12 &&
                   offsetof(ptss_glare_params, reserved) == 20,
               "ptss_glare_params is six 32-bit words");
_Static_assert(sizeof(ptss_glare_entry) == 32 && offsetof(ptss_glare_entry, g) == 8 && offsetof(ptss_glare_entry, zero) == 24,
               "ptss_glare_entry is two 16-byte rows");
_Static_assert(sizeof(ptss_glare_level) == 16 && offsetof(ptss_glare_level, height) == 4 && offsetof(ptss_glare_level, first) == 8,
               "ptss_glare_level is two 32-bit words and one 64-bit word");
_Static_assert(sizeof(ptss_denoise_linear_params) == 32 && offsetof(ptss_denoise_linear_params, levels) == 4 &&
                   offsetof(ptss_denoise_linear_params, sigmaLuminance) == 8 && offsetof(ptss_denoise_linear_params, sigmaDepth) == 16 &&
                   offsetof(ptss_denoise_linear_params, reserved) == 20,
               "ptss_denoise_linear_params is eight 32-bit words");
_Static_assert(sizeof(ptss_reproject_linear_params) == 24 && offsetof(ptss_reproject_linear_params, cosNormal) == 4 &&
                   offsetof(ptss_reproject_linear_params, minCoverage) == 12 && offsetof(ptss_reproject_linear_params, maxHistory) == 16 &&
                   offsetof(ptss_reproject_linear_params, reserved) == 20,
               "ptss_reproject_linear_params is six 32-bit words");
_Static_assert(sizeof(ptss_reproject_linear_info) == 32 && offsetof(ptss_reproject_linear_info, offFilm) == 8 &&
                   offsetof(ptss_reproject_linear_info, noVariance) == 24,
               "ptss_reproject_linear_info is four 64-bit words");
_Static_assert(sizeof(ptss_upsample_linear_params) == 24 && offsetof(ptss_upsample_linear_params, factor) == 4 &&
                   offsetof(ptss_upsample_linear_params, sigmaDepth) == 12 && offsetof(ptss_upsample_linear_params, flags) == 16 &&
                   offsetof(ptss_upsample_linear_params, reserved) == 20,
               "ptss_upsample_linear_params is six 32-bit words");
_Static_assert(sizeof(ptss_upsample_linear_info) == 24 && offsetof(ptss_upsample_linear_info, fallback) == 8 &&
                   offsetof(ptss_upsample_linear_info, empty) == 16,
               "ptss_upsample_linear_info is three 64-bit words");
_Static_assert(sizeof(ptss_tone_params) == 48 && offsetof(ptss_tone_params, curve) == 4 && offsetof(ptss_tone_params, bits) == 12 &&
                   offsetof(ptss_tone_params, white) == 20 && offsetof(ptss_tone_params, filmic) == 24 && offsetof(ptss_tone_params, reserved) == 44,
               "ptss_tone_params is twelve 32-bit words");
_Static_assert(sizeof(ptss_surface_point) == 16 && offsetof(ptss_surface_point, a) == 4 && offsetof(ptss_surface_point, b) == 8 &&
                   offsetof(ptss_surface_point, flags) == 12,
               "ptss_surface_point is one 16-byte row");
_Static_assert(sizeof(ptss_surface_params) == 16 && offsetof(ptss_surface_params, mode) == 4 && offsetof(ptss_surface_params, maxDistance) == 8 &&
                   offsetof(ptss_surface_params, reserved) == 12,
               "ptss_surface_params is four 32-bit words");
_Static_assert(sizeof(ptss_surface_block) == 16 && offsetof(ptss_surface_block, y) == 4 && offsetof(ptss_surface_block, width) == 8 &&
                   offsetof(ptss_surface_block, height) == 12,
               "ptss_surface_block is one 16-byte row");
_Static_assert(sizeof(ptss_chain_result) == 32 && offsetof(ptss_chain_result, steps) == 12 && offsetof(ptss_chain_result, direction) == 16 &&
                   offsetof(ptss_chain_result, pathLength) == 28,
               "ptss_chain_result is two 16-byte rows");
_Static_assert(sizeof(ptss_chain_options) == 16 && offsetof(ptss_chain_options, schedule) == 4 && offsetof(ptss_chain_options, maxWorkgroups) == 8 &&
                   offsetof(ptss_chain_options, reserved) == 12,
               "ptss_chain_options is four 32-bit words");
_Static_assert(sizeof(ptss_lightmap_params) == 40 && offsetof(ptss_lightmap_params, atlasWidth) == 4 && offsetof(ptss_lightmap_params, filter) == 12 &&
                   offsetof(ptss_lightmap_params, flags) == 16 && offsetof(ptss_lightmap_params, firstTriangle) == 20 &&
                   offsetof(ptss_lightmap_params, firstSphere) == 28 && offsetof(ptss_lightmap_params, reserved) == 36,
               "ptss_lightmap_params is ten 32-bit words");
#endif

#ifdef __cplusplus
}
#endif
#endif
