/* ptss.h — C-ABI of libptss.so: the MI355X-native drop-in for the reference's per-frame hot path.
 *
 * The reference has no plugin/FFI layer; its seam is the GPUAnimBitmap frame callback plus the
 * scene vectors. Each entry point below names the reference code it replaces
 * (paths relative to /root/reference/CudaTracer/). INTEGRATION.md shows the host-side glue.
 *
 * Conventions: plain pointers and sizes only; every function returns PTSS_OK (0) or a negative
 * PTSS_E* code (no exit(), unlike CUDA_ERROR_HANDLE, CudaUtils.h:13-21); no exceptions cross the
 * boundary; one host thread per context at a time (the reference is single-threaded, CudaUtils.h:117).
 * There is NO CPU fallback: without a usable HIP device ptss_create fails with PTSS_ENODEVICE.
 */
#ifndef PTSS_H
#define PTSS_H

#include "ptss_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTSS_OK 0
#define PTSS_EINVAL (-1)   /* bad argument */
#define PTSS_EHIP (-2)     /* a HIP runtime call or kernel launch failed; see ptss_last_error_detail */
#define PTSS_ENODEVICE (-3)/* no usable HIP device */
#define PTSS_ENOMEM (-4)   /* host or device allocation failed */
#define PTSS_ERANGE (-5)   /* output buffer too small / index out of range */
#define PTSS_ETIMEOUT (-6) /* a bounded wait on the device (~2 s) expired: a frame lane for a peer lane, or a workgroup of the one-launch
                              frame kernel for its shard; the frame was not traced as specified, the buffers may hold another image */
#define PTSS_VERSION 300   /* what ptss_version() of a matching library returns; bumped whenever a struct below changes */

typedef struct ptss_context ptss_context; /* ≙ ProgramData + RendererData + every cudaMalloc of main() */

typedef struct ptss_render_config {
    unsigned int structSize;     /* sizeof(ptss_render_config) as the CALLER compiled it (ptss_default_config fills it in);
                                    ptss_create refuses any other value, so a binding built against an older header fails
                                    loudly instead of being read past its end */
    int width, height;           /* full frame; the reference's compile-time DIM x DIM (CudaUtils.h:7) */
    unsigned long long seed;     /* curand_init seed; the reference passes clock64() (CudaTracer.cu:28) */
    unsigned int maxIterations;  /* ProgramData::maxIterations, default 15 (CudaTracer.h:39) */
    int device;                  /* HIP device ordinal (reference: cudaChooseDevice, CudaUtils.h:49-57) */
    /* Pixel-tile shard (north_star): this context owns the rows y with
     * (y / bandRows) % tileWorld == tileRank. tileWorld = 1 renders the whole frame. The RNG
     * subsequence is the GLOBAL pixel index, so the image does not depend on the sharding — with ONE exception:
     * the reference stops bouncing once <= 128 rays are alive in the WHOLE frame (CudaTracer.cu:622); a shard cannot
     * know that count without a collective per bounce, so a context with tileWorld > 1 never stops early (and
     * ptss_live_counts reports its own rays down to 0). Sharded and unsharded images are identical whenever more than
     * 128 rays stay alive frame-wide at every bounce that runs (always, at the benchmark sizes); they differ in tiny
     * frames and in frames whose last few rays outlive the guard (tests/test_gpu_tiles.py pins both behaviours). */
    int tileRank, tileWorld, bandRows;
    int syncEachFrame;     /* 1: block on the stop event and record ms each frame, as CudaTracer.cu:639-642 */
    int floatAccumulator;  /* 1: also keep a linear float32 sum of radiance0 per pixel */
    int timeKernels;       /* 1: bracket every bounce kernel with HIP events (bench.py roofline) */
    /* Extension, default 1 = the reference: S independent samples per pixel per
     * ptss_generate_frame call. Sample lane l of global pixel g owns XORWOW subsequence g*S + l; every sample
     * is still tone-mapped on its own before it is summed (CudaTracer.cu:72-92); the display divides by
     * S*(ticks - lastResetTick + 1). Lets one launch carry S times the rays (multi-GPU shards stay busy). 1..64. */
    int samplesPerPass;
    /* 1 = the reference's loops over every primitive. By default scenes with >= 64 finite spheres are traversed through spatially
     * sorted sphere chunks (tests/test_gpu_many_spheres.py), and scenes of 512 .. 2^20 triangles, fewer than 64
     * spheres and |coordinate| <= 2^40 through a two-level hierarchy of triangle leaves and groups (the mesh image, DESIGN.md
     * §3.15; tests/test_gpu_mesh.py) — the same image either way. 1 keeps the every-sphere and every-triangle loops for them too. */
    int everySphereLoop;
    /* Frame lanes: the frame traced as K ray populations on K streams of the device, the tail of one lane's launches
     * overlapping the other lanes' kernels. The image — loop guard included — does not depend on K.
     * 0 = the library's choice: ONE lane, unless lanesFreeRun is set (then 2 for 3*2^17..2^24 rays per pass, e.g. 800x600 ...
     * 3840x2160 at one sample per tick, else 1); 1..4 = that many. */
    int frameLanes;
    /* Stream ordering of a context with more than one lane. 0 (default): STRICT — like a one-lane context the call is
     * ordered on the caller's stream: the lanes of every frame start behind whatever the caller enqueued on its stream before
     * the call, and the stream continues behind the whole frame, so work enqueued between two ptss_generate_frame calls
     * (a copy of dev_pixels, a gather or a zero-fill of the bound accumulator, ...) sees exactly the frames before it. With that
     * fork and join every frame two lanes are no faster than one (measured, profiles/README.md). 1: FREE-RUNNING — the lanes are
     * forked from the caller's stream only on a reset or camera change and run on from frame to frame (this is where lanes
     * gain: +15-18 % at 1080p, one sample per tick); the caller's stream still continues behind each frame, but the NEXT frame's
     * kernels do not wait for anything the caller enqueued after the previous call. Opt in only if, between two calls,
     * nothing touches dev_pixels, the accumulator or the float sums on the device — or call ptss_synchronize() /
     * ptss_request_reset() first. */
    int lanesFreeRun;
    /* One launch per frame, opt-in: a frame small enough for ALL its bounce-0 tiles to be resident on the device
     * at once (up to about 3*2^17 rays per pass on an MI355X: 512x512 or 640x480 at one sample per tick) is traced by ONE kernel
     * whose workgroups carry their shard from bounce to bounce, instead of one launch per bounce each at most one resident
     * round wide: +7 % at 512x512. Same image, same counters. 1 = on where the frame qualifies (one lane, scene in LDS; a frame
     * that does not qualify is traced bounce by bounce all the same); 0 (default) / -1 = off. Opt-in because the kernel's
     * workgroups wait for each other: it must have the device to itself — two such kernels running at once (two contexts on
     * two streams, or two processes sharing the GPU) can each hold slots the other needs; every wait is bounded (~2 s) and an
     * expired one surfaces as PTSS_ETIMEOUT, but the frame is then lost. */
    int oneLaunchFrames;
} ptss_render_config;

/* Fills the reference's defaults: 512x512 (DIM), maxIterations 15, seed 0x5EED, one tile, sync on. */
int ptss_default_config(ptss_render_config* cfg);

/* ≙ main(): cudaMalloc x8, cudaMemcpy x5 of the scene vectors, ProgramData fill, curandSetupKernel
 * (CudaTracer.cu:671-724). Scene arrays are copied; the caller may free them afterwards.
 * Starts with Camera() defaults, usePathTracer = true, resetTicksThisFrame = true (:703,:717). */
int ptss_create(const ptss_scene_desc* scene, const ptss_render_config* cfg, ptss_context** out);

/* ≙ cudaFree x8 + delete data (CudaTracer.cu:731-740). */
int ptss_destroy(ptss_context* ctx);

/* ≙ generateFrame(uchar4* pixels, void* dataBlock, int ticks) (CudaTracer.cu:587-647), the fAnim
 * callback of GPUAnimBitmap (CudaUtils.h:36,154). dev_pixels: DEVICE pointer to this context's
 * local pixels (width * ptss_local_rows, RGBA, row 0 = bottom), owned by the caller, or NULL to
 * skip the display write. ticks: the caller's running counter (starts at 1, CudaUtils.h:146). */
int ptss_generate_frame(ptss_context* ctx, ptss_uchar4* dev_pixels, int ticks);

/* ≙ Key()/moveCamera() effects on ProgramData (CudaTracer.cu:782-785): store camera, set the reset flag. */
int ptss_set_camera(ptss_context* ctx, const ptss_camera* camera);
int ptss_get_camera(const ptss_context* ctx, ptss_camera* out);
/* ≙ resetTicksThisFrame = true (CudaTracer.cu:764,784). */
int ptss_request_reset(ptss_context* ctx);
/* ≙ space bar: usePathTracer toggle + reset (CudaTracer.cu:760-765). 0 = one-bounce ray tracing. */
int ptss_set_mode(ptss_context* ctx, int usePathTracer);
int ptss_set_max_iterations(ptss_context* ctx, unsigned int maxIterations);

/* Plumbing for callers that own device memory / streams (PyTorch, GPUAnimBitmap). */
int ptss_set_stream(ptss_context* ctx, void* hipStream);            /* default: the null stream */
int ptss_bind_accumulator(ptss_context* ctx, uint32_t* dev_uint3);  /* external totalPixelColors, 3 u32 per local pixel */
int ptss_accumulator_devptr(ptss_context* ctx, uint32_t** out);
int ptss_float_accumulator_devptr(ptss_context* ctx, float** out);
int ptss_alloc_pixels(ptss_context* ctx, ptss_uchar4** out_dev);    /* headless stand-in for the GL PBO (CudaUtils.h:72-81) */
int ptss_free_pixels(ptss_context* ctx, ptss_uchar4* dev);
int ptss_local_pixels(const ptss_context* ctx, size_t* out);        /* width * local rows */
int ptss_local_rows(const ptss_context* ctx, int* rows, int cap, int* count); /* global y of each local row */

/* Device -> host copies (synchronising). count = number of ELEMENTS of the destination type. */
int ptss_read_accumulator(ptss_context* ctx, uint32_t* host_uint3, size_t count);       /* 3 * local pixels */
int ptss_read_float_accumulator(ptss_context* ctx, float* host_float3, size_t count);   /* 3 * local pixels */
int ptss_read_pixels(ptss_context* ctx, const ptss_uchar4* dev_pixels, ptss_uchar4* host, size_t count);
int ptss_read_rng_state(ptss_context* ctx, size_t local_pixel, uint32_t* out6);         /* v0..v4, d (sample lane 0) */
int ptss_read_rng_state_lane(ptss_context* ctx, size_t local_pixel, unsigned int lane, uint32_t* out6);
int ptss_synchronize(ptss_context* ctx);

/* ≙ the "Rays per pixel / Time per pass" line (CudaTracer.cu:641-646). */
int ptss_last_pass_ms(ptss_context* ctx, float* out_ms);
int ptss_samples_since_reset(const ptss_context* ctx, int* out);
/* Rays that ENTERED each bounce of the last frame (numRays at CudaTracer.cu:623); returns count in *n. */
int ptss_live_counts(ptss_context* ctx, uint32_t* out, int cap, int* n);
/* Sum over all frames and bounces of rays processed by the bounce kernel (the Mrays numerator). */
int ptss_total_ray_bounces(ptss_context* ctx, unsigned long long* out);
/* HIP-event time of the bounce kernel since the last call (needs cfg.timeKernels): total ms, launches. */
int ptss_bounce_kernel_time(ptss_context* ctx, double* total_ms, unsigned long long* launches);

/* 1 when this context traces a frame with ONE launch (cfg.oneLaunchFrames resolved for the scene image in use). */
int ptss_one_launch_frames(const ptss_context* ctx, int* out);
/* Frame lanes this context runs (cfg.frameLanes resolved). */
int ptss_frame_lanes(const ptss_context* ctx, int* out);
/* How often a lane gave up waiting for a peer lane's live count (a stream that did not run for ~2 s): always 0 in a healthy
 * process; a non-zero value means the loop guard of that frame was decided without the peer. Every synchronising entry
 * point (ptss_synchronize, ptss_read_*, ptss_live_counts, ptss_total_ray_bounces, ptss_bounce_kernel_time, and
 * ptss_generate_frame with syncEachFrame) returns PTSS_ETIMEOUT once when this count has grown since the last check. */
int ptss_guard_timeouts(ptss_context* ctx, unsigned int* out);

/* Which kernel instantiations this context has enqueued since ptss_create, as a bitmask (tests/test_gpu_kernel_coverage.py):
 * every kernel owns a range of bits, PTSS_KERNEL_x .. PTSS_KERNEL_x + PTSS_KERNEL_WIDTH_x - 1 (ptss_types.h, which also says how the
 * instantiations of a kernel are numbered inside its range): PTSS_KERNEL_BOUNCE and PTSS_KERNEL_BOUNCE_MESH for the bounce kernels,
 * PTSS_KERNEL_FRAME for the one-launch frame kernels, PTSS_KERNEL_QUERY (ptss_intersect, ptss_occluded), PTSS_KERNEL_FEATURES
 * (ptss_render_features), PTSS_KERNEL_DENOISE (ptss_denoise), PTSS_KERNEL_UPDATE and PTSS_KERNEL_REFIT (ptss_update_triangles),
 * PTSS_KERNEL_REPROJECT (ptss_reproject), PTSS_KERNEL_FEATURES_MOTION (ptss_render_features_motion) and
 * PTSS_KERNEL_REPROJECT_MOTION (ptss_reproject_motion).
 * Recorded on the host at launch. */
int ptss_launched_kernels(const ptss_context* ctx, unsigned long long* out);

/* The strip words of the latest ptss_generate_frame (csrc/ptstrip.h): one 64-bit word per 64 consecutive local pixels
 * of the context's pixel plane (*count of them: the local pixels rounded up to 256, over 64), bits 0-31 the stored spheres and bits 32-63
 * the stored triangles bounce 0 visits for that strip. *enabled = 1 when that frame's bounce 0 read them; 0 (and every word all ones)
 * when it visited every primitive: an image or camera outside the cull's domain, the one-launch frame kernel, or no frame since the
 * camera or the scene last changed. host_words holds `capacity` words (PTSS_EINVAL when that is fewer than *count, which is still set).
 * Synchronises the context's stream. For tests and diagnostics: the words are a pure function of camera, scene and frame shape
 * (ptss_probe_strip_masks, ptss_host.h, computes the same ones on the host). */
int ptss_read_strip_words(ptss_context* ctx, unsigned long long* host_words, size_t capacity, size_t* count, int* enabled);

/* Which range guards of the shading code the current scene's constants satisfy, decided once at ptss_create / ptss_set_scene
 * (DESIGN.md §3.8): bit 0 every light-power component is +0.0 or has a magnitude in [2^-60, 2^60), bit 1 every index of refraction has,
 * bit 2 every specularExponent is +inf or has |exponent + 1| in [2^-125, 2^126). A set bit lets the kernels divide by / into that
 * constant without testing its range again; a clear bit leaves the guarded code. The images are the same either way. */
int ptss_guard_flags(const ptss_context* ctx, unsigned int* out);

/* Batched ray queries against the context's scene. dev_rays / dev_hits / dev_occluded are DEVICE pointers of n
 * entries on the context's device. ptss_intersect: what the reference's intersectScene loop (CudaTracer.cu:120-141) returns for
 * ray (origin, direction) with `distance` starting at tmax — spheres 0..S-1, then triangles 0..T-1 — bit for bit, for every input
 * (non-unit, zero, infinite and NaN components included). ptss_occluded: dev_occluded[i] = 1 iff some primitive's
 * intersectRay(ray, tmax, surfel, false) accepts (lineOfSight's loop, CudaTracer.cu:434-452, without the bump and the
 * shortening), else 0. Asynchronous on hipStream (NULL: the context's stream). They read the scene image only, never the
 * per-camera rows, and leave no trace in frame state: they may run between frames or on another stream while frames run.
 * n = 0 returns PTSS_OK; a null context or null pointers with n > 0 return PTSS_EINVAL, n >= 2^31 PTSS_ERANGE, without touching
 * the device. ptss_launched_kernels reports the query kernel at PTSS_KERNEL_QUERY + any * 2 + inLds. */
int ptss_intersect(ptss_context* ctx, const ptss_ray_query* dev_rays, ptss_ray_hit* dev_hits, size_t n, void* hipStream);
int ptss_occluded(ptss_context* ctx, const ptss_ray_query* dev_rays, uint32_t* dev_occluded, size_t n, void* hipStream);

/* First-hit feature buffer. dev_features: DEVICE pointer to one entry per local pixel, in the order of dev_pixels
 * and ptss_local_rows. Entry p holds what ptss_intersect returns for ptss_camera_ray(camera, width, height, x, y, 0.5, 0.5) of the
 * context's CURRENT camera with tmax = +inf — normal, distance, materialIdx — and that material's diffuseColor, every field bit for
 * bit; a miss: normal 0, depth +inf, materialIdx -1, albedo = the scene's defaultColor. Asynchronous on hipStream (NULL: the
 * context's stream). Like the queries it reads the scene image only and leaves no trace in frame state; it serves pixel-band shards
 * (tileWorld > 1) for their own pixels. ptss_launched_kernels reports the feature kernel at PTSS_KERNEL_FEATURES + inLds. */
int ptss_render_features(ptss_context* ctx, ptss_pixel_feature* dev_features, void* hipStream);

/* First-hit features AND per-pixel motion across a pose change of the triangles, from ONE trace per pixel.
 * dev_features receives what ptss_render_features writes, bit for bit. dev_triangles_prev: DEVICE pointer to `count` records in the
 * caller's 76-byte layout, the PREVIOUS pose of the triangles with original indices first .. first + count - 1 — in practice the
 * buffer handed to the ptss_update_triangles call before the latest one; only its vertices are read. count = 0: nothing moved
 * (dev_triangles_prev may be NULL). dev_motion (one 16-byte row per local pixel, in the order of dev_features), with d the
 * pixel-centre direction, o the camera position and the hit what ptss_intersect returns for that ray:
 *   a miss:          prevPoint = 0, surface = -1;
 *   a static hit     (a sphere, a triangle outside the range, or one whose previous record ptss_update_triangles would have refused —
 *                    a vertex not finite or beyond 2^40: it never became geometry): prevPoint = fma(d, distance, o), the point
 *                    ptss_reproject evaluates; surface = k for sphere k, PTSS_SURFACE_TRIANGLE | t for triangle t;
 *   a moved triangle t: prevPoint = fma(e2', w2, fma(e1', w1, v0')) with v0', e1' = v1' - v0', e2' = v2' - v0' of record t - first and
 *                    the hit's weights w1, w2 (they go with vertex1 and vertex2, as in the normal interpolation).
 * Every image kind is served (the index is the caller's), and pixel-band shards for their own pixels. Asynchronous on hipStream
 * (NULL: the context's stream); it reads the scene image and the caller's records only and leaves no trace in frame state. The
 * caller orders it behind the ptss_update_triangles whose pose it traces and keeps dev_triangles_prev alive until it has run.
 * Refused without touching the device: a null context or output pointer, a null dev_triangles_prev with count > 0, a misaligned
 * pointer (PTSS_EINVAL); with count > 0, a range that leaves [0, numTriangles) (PTSS_ERANGE). Spheres move only through
 * ptss_set_scene and count as static. ptss_launched_kernels: PTSS_KERNEL_FEATURES_MOTION + inLds. */
int ptss_render_features_motion(ptss_context* ctx, const ptss_triangle* dev_triangles_prev, size_t first, size_t count,
                                ptss_pixel_feature* dev_features, ptss_pixel_motion* dev_motion, void* hipStream);

/* Features BEHIND mirrors and glass. The centre ray of every local pixel is carried through the delta lobes of the
 * surfaces it meets — perfect reflection, refraction; which one is decided from the material alone, csrc/ptspecular.h — for at most
 * maxSteps (0 .. 8) steps, to the first surface that is neither a mirror nor glass. dev_features (the layout and order of
 * ptss_render_features) receives normal, materialIdx and albedo of the LAST surface of that chain, and as depth the float32 sum of the
 * chain's hit distances in chain order; a chain that leaves the scene writes the miss row (normal 0, depth +inf, materialIdx -1,
 * defaultColor). dev_steps (may be NULL): one uint32 per local pixel, the steps taken, 0 .. maxSteps. Every link is what
 * ptss_intersect returns for the ray ptss_probe_specular_step (ptss_host.h) continues with, bit for bit; maxSteps = 0 writes what
 * ptss_render_features writes, bit for bit.
 * The depth is a PATH LENGTH (a virtual depth), not the distance of a point on the centre ray: these features are for ptss_denoise and
 * ptss_denoise_history only. ptss_reproject and ptss_reproject_motion rebuild a world point from the depth along the centre ray and
 * still need the first-hit features of ptss_render_features.
 * Asynchronous on hipStream (NULL: the context's stream). It reads the scene image only and leaves no trace in frame state; it serves
 * pixel-band shards (tileWorld > 1) for their own pixels. Refused with PTSS_EINVAL without touching the device: a null context or
 * dev_features, maxSteps outside 0..8, a dev_features that is not 16-byte aligned or a dev_steps that is not 4-byte aligned.
 * The kernel owns no bit of ptss_launched_kernels, which this call leaves as it is; ptss_specular_feature_launches counts its launches
 * since ptss_create instead: out2[0] with the scene image read in place, out2[1] with the image staged in LDS. */
int ptss_render_features_specular(ptss_context* ctx, int maxSteps, ptss_pixel_feature* dev_features, uint32_t* dev_steps /* may be NULL */,
                                  void* hipStream);
int ptss_specular_feature_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] in place, [1] in LDS */

/* Batched path queries: the path tracer started from the caller's rays, the third member of the query family.
 * ptss_seed_path_rng writes one XORWOW state per entry: dev_rng[i] = the state of curand_init(seed, firstSequence + i, 0) after `skip`
 * (0 .. 64) draws, through the jump table the context's own streams are seeded with. A caller who keeps dev_rng across
 * ptss_trace_paths calls continues the streams: a probe accumulates progressively without any library state.
 * ptss_trace_paths runs ray i as the thread body of the reference's pathTraceKernel (CudaTracer.cu:106-206), called maxIterations
 * (1 .. 64) times or until the ray goes inactive, with stream dev_rng[i]: it starts from radiance0 = 0, radiance1 = 1 and distance
 * +inf — the row's tmax is IGNORED (the struct is ptss_ray_query so that ptss_camera_ray's output can be passed as it is) —, takes the
 * closest hit over spheres then triangles; a miss adds defaultColor * radiance1 and ends the path; a hit adds the emittance, runs
 * shade() when cosI = dot(-d, normal) > 0 (point lights, then area lights, in index order; four draws per area light whether or not
 * it is visible), scatters — except in iteration maxIterations - 1, whose indirect factor is (1, 1, 1) —, applies Beer-Lambert when
 * inside, then updates radiance0 and radiance1 in the reference's order. dev_results[i].radiance = the final radiance0, LINEAR: no
 * tone map and no clamp, NaN and inf stored as they come; .bounces = the iterations the ray entered; dev_rng[i] receives the stream's
 * state afterwards. Fed a frame's own eye rays and streams (ptss_camera_ray with the pixel's two jitter draws; ptss_seed_path_rng(seed,
 * 0, skip = 2) in pixel order) the call reproduces that frame's linear radiance (ptss_read_float_accumulator after the first frame)
 * and final stream states bit for bit — as long as the frame's loop guard never fires: every path runs on its own here, so the
 * reference's "stop once at most 128 rays are alive frame-wide" (CudaTracer.cu:622) does not exist, which is the documented behaviour
 * of a tileWorld > 1 context.
 * Both calls are asynchronous on hipStream (NULL: the context's stream). ptss_trace_paths reads the scene image only, never the
 * per-camera rows, leaves no trace in frame state, may run between frames or beside them on another stream, serves sharded contexts,
 * and is ordered by the caller against ptss_update_triangles, ptss_resort_triangles and ptss_set_scene under their rules. The first
 * ptss_seed_path_rng of a context uploads the jump table (100 KiB, synchronously).
 * Refused without touching the device and without counting: a null context, or a null pointer with n > 0 (PTSS_EINVAL); a pointer that
 * is not aligned — 16 bytes for rays and results, 4 for dev_rng — (PTSS_EINVAL); maxIterations outside 1 .. 64 or skip above 64
 * (PTSS_EINVAL); n >= 2^31, or firstSequence + n above 2^32 (PTSS_ERANGE). n = 0 returns PTSS_OK.
 * Neither kernel owns a bit of ptss_launched_kernels, which these calls leave as it is; ptss_path_launches counts the ptss_trace_paths
 * launches since ptss_create instead: out2[0] with the scene image read in place, out2[1] with the image staged in LDS. */
int ptss_seed_path_rng(ptss_context* ctx, ptss_path_rng* dev_rng, size_t n, unsigned long long seed, unsigned long long firstSequence,
                       unsigned int skip, void* hipStream);
int ptss_trace_paths(ptss_context* ctx, const ptss_ray_query* dev_rays, ptss_path_rng* dev_rng /* in/out */, ptss_path_result* dev_results,
                     size_t n, unsigned int maxIterations, void* hipStream);
int ptss_path_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] scene read in place, [1] staged in LDS */

/* ptss_trace_paths with a choice of schedule. ptss_default_path_options: structSize, PTSS_PATHS_LANE_PER_RAY, 0, 0.
 * PTSS_PATHS_LANE_PER_RAY: the call IS ptss_trace_paths (the same launch, counted in ptss_path_launches).
 * PTSS_PATHS_REFILL: a lane whose path has ended takes the next unclaimed ray of the batch from a device-side queue, so a wave no longer
 * runs dead lanes until the longest of its 64 paths has ended. Every output byte, results and streams, is what ptss_trace_paths writes
 * for the same inputs, for every input and every maxWorkgroups. It pays on small scenes with long paths (DESIGN.md §3.27 has the
 * measurements); the default stays LANE_PER_RAY. maxWorkgroups caps the grid (0: as many workgroups as the device holds at once); a
 * small cap leaves part of the device to frames running beside the query.
 * ORDERING: the queue's head is one device word of the context, set on hipStream in front of the kernel. The PTSS_PATHS_REFILL calls of
 * one context must therefore be ordered among themselves by the caller — the same stream, or an event or a synchronise between two
 * streams (the rule of ptss_denoise's planes and ptss_resort_triangles' scratch). Plain ptss_trace_paths calls, queries, feature passes
 * and frames may run beside a refill call on other streams. The first refill call of a context allocates the word (hipMalloc).
 * Refused with PTSS_EINVAL / PTSS_ERANGE without touching the device and without counting: everything ptss_trace_paths refuses, a null
 * options, a wrong structSize, an unknown schedule, a negative maxWorkgroups, a non-zero reserved. n = 0 returns PTSS_OK, nothing launched.
 * Refill launches are not counted in ptss_path_launches and own no bit of ptss_launched_kernels. ptss_path_refill_stats, since
 * ptss_create: out5[0] refill launches with the scene image read in place, [1] staged in LDS (host counts); [2] wave iterations (the
 * iterations the waves ran), [3] lane iterations (the live lanes summed over them = the sum of .bounces), [4] dequeues (device counts:
 * the call synchronises with the stream of the latest refill call). [3] / (64 [2]) is the lane occupancy. */
int ptss_default_path_options(ptss_path_options* options);
int ptss_trace_paths_opt(ptss_context* ctx, const ptss_ray_query* dev_rays, ptss_path_rng* dev_rng /* in/out */, ptss_path_result* dev_results,
                         size_t n, unsigned int maxIterations, const ptss_path_options* options, void* hipStream);
int ptss_path_refill_stats(ptss_context* ctx, unsigned long long* out5);

/* The film of a path query: eye rays made on the device, samples accumulated as a frame accumulates them, features
 * of arbitrary rays. A film is film->width x film->height pixels of its own (independent of the context's frame), pixel
 * p = (x, y) = (p % width, p / width), row 0 at the bottom.
 *
 * ptss_generate_rays: dev_rays[i] = the eye ray of film pixel p = dev_index ? dev_index[i] : firstPixel + i, made from stream dev_rng[i],
 * which is stored back advanced by the model's draws (uniforms of (0, 1], curand_uniform's). csrc/ptcamera.h fixes every operation and
 * its order; its host build (ptss_probe_film_rays, ptss_host.h) is the specification and the device agrees with it byte for byte.
 * With s = -2 tan(fov / 2), aspect = H / W, invW = 1 / W, invH = 1 / H evaluated once on the host, X = x + jx, Y = y + jy and
 * start = (((X invW) - 0.5) s, ((Y invH) - 0.5) s aspect, 1) zNear:
 *   PTSS_FILM_PINHOLE    draws jx, jy (computeEyeRaysKernel's order). origin = position, direction = normalize(rotate(rotation, start)):
 *                        ptss_camera_ray(camera, width, height, x, y, jx, jy), bit for bit.
 *   PTSS_FILM_THIN_LENS  draws jx, jy, u1, u2. Focus point f = start * (focusDistance / |start.z|) (camera space, on the plane
 *                        |z| = focusDistance); lens point l = lensRadius sqrt(u1) (cos 2 pi u2, sin 2 pi u2, 0);
 *                        origin = position + rotate(rotation, l), direction = normalize(rotate(rotation, f - l)). At lensRadius = 0 the
 *                        rays are a pinhole's up to rounding, not bit for bit.
 *   PTSS_FILM_EQUIRECT   draws jx, jy. lon = ((X invW) - 0.5) 2 pi, lat = ((Y invH) - 0.5) pi, camera-space direction
 *                        (sin lon cos lat, sin lat, -cos lon cos lat), rotated and normalised; origin = position. The film's centre looks
 *                        along rotate(rotation, (0, 0, -1)), where the centre ray of the reference's pinhole cameras (zNear < 0) looks, and
 *                        +x, +y have the pinhole's senses. fieldOfView and zNear are not read.
 * jitter = 0: no draw is made and no stream is read or written (dev_rng must still be given): jx = jy = 0.5 and the lens point is the
 * lens centre. Every ray has
 * tmax = +inf, pad = 0. An index entry >= width * height writes no ray, leaves its stream as it is and is counted.
 *
 * ptss_accumulate_paths: for ray i, pixel p as above, the three channels of dev_results[i].radiance go through the frame's own 8-bit tone map
 * (writeToPixelsKernel, CudaTracer.cu:72-85, in the table form a frame uses, with the context's thresholds; NaN gives 0, +inf 255) and
 * are added to dev_film[p].r, .g, .b; .samples grows by 1. Then, for every pixel touched, with inv = 1.f / (float)samples:
 * dev_pixels[p] = {(unsigned char)(r * inv + 0.5f), .. g, .. b, 255} (may be NULL) and dev_history[p] = {(float)r * inv, .. g, .. b,
 * (float)samples} (may be NULL): the display pixel of a frame and the entry ptss_denoise_history, ptss_reproject and ptss_upsample take.
 * Without an index every ray has a pixel of its own: one kernel, a plain read-modify-write. With an index several rays may share a
 * pixel: the sums are integer atomics, order-free and exact, and the touched pixels are resolved by a second launch behind the first.
 * Index entries >= filmPixels are dropped and counted. The caller zero-fills a new film; samples must stay below 2^24 (exact as a float).
 * A pinhole film of the context's size, fed ptss_seed_path_rng(seed, 0, skip = 0) streams and run generate -> ptss_trace_paths ->
 * accumulate once per frame, reproduces the frame loop's accumulator, display pixels and stream states bit for bit, frame after frame,
 * under ptss_trace_paths' condition (the frame's loop guard never fires).
 *
 * ptss_ray_features: dev_features[i] = what ptss_render_features documents, for ray i: ptss_intersect's normal, distance and materialIdx
 * with tmax = +inf (the row's tmax is ignored), that material's diffuseColor; the same miss row. Of jitter = 0 rays it is the feature
 * buffer of a film.
 *
 * All three are asynchronous on hipStream (NULL: the context's stream), read the scene image at most, leave no trace in frame state and
 * serve sharded contexts. Refused without touching the device and without counting: a null context, a null required pointer with n > 0,
 * a wrong structSize, an unknown kind, a jitter other than 0 or 1, a film size that is not positive, a thin lens with lensRadius < 0,
 * focusDistance <= 0 or either not finite, a pointer that is not aligned — 16 bytes for rays, results, film, features and history, 4 for
 * streams, indices and pixels — (PTSS_EINVAL); n >= 2^31, width * height (filmPixels) >= 2^31, or, without an index, firstPixel + n
 * above the film's pixels (PTSS_ERANGE). n = 0 returns PTSS_OK.
 * No kernel here owns a bit of ptss_launched_kernels, which these calls leave as it is. ptss_film_launches: the calls of each kind that
 * launched since ptss_create. ptss_film_rejected: the index entries dropped since ptss_create; it synchronises with the latest call that
 * took an index. */
int ptss_generate_rays(ptss_context* ctx, const ptss_film_camera* film, size_t firstPixel, const uint32_t* dev_index /* may be NULL */, size_t n,
                       ptss_path_rng* dev_rng /* in/out */, ptss_ray_query* dev_rays, void* hipStream);
int ptss_accumulate_paths(ptss_context* ctx, const ptss_path_result* dev_results, const uint32_t* dev_index /* may be NULL */, size_t firstPixel,
                          size_t n, ptss_film_entry* dev_film, size_t filmPixels, ptss_uchar4* dev_pixels /* may be NULL */,
                          ptss_history_entry* dev_history /* may be NULL */, void* hipStream);
int ptss_ray_features(ptss_context* ctx, const ptss_ray_query* dev_rays, ptss_pixel_feature* dev_features, size_t n, void* hipStream);
int ptss_film_launches(const ptss_context* ctx, unsigned long long* out3); /* [0] generate, [1] accumulate, [2] features */
int ptss_film_rejected(ptss_context* ctx, unsigned long long* out);

/* Adaptive film sampling: a film that also keeps the second moment of its samples, and a plan that turns film and
 * moments into the next round's index on the device. One round is
 *     ptss_generate_rays(index) -> ptss_trace_paths -> ptss_accumulate_paths_stats(index) -> ptss_plan_samples -> the next index,
 * with no host round trip. Ray slot i keeps stream dev_rng[i] whatever pixel the index gives it: streams belong to slots, not to pixels.
 * Choosing sample counts from the samples themselves biases the estimate (a pixel whose first samples happen to agree is left early);
 * that is a known property of the scheme and is not corrected here.
 *
 * dev_moments: one unsigned long long per film pixel, 8-byte aligned, zero for a new film: the sum, over the samples accumulated into the
 * pixel, of qr^2 + qg^2 + qb^2, where q* are the three tone-mapped bytes ptss_accumulate_paths adds to the film entry (at most 195,075
 * per sample: no overflow below 2^24 samples).
 *
 * ptss_accumulate_paths_stats: ptss_accumulate_paths' arguments, refusals and bytes — dev_film, dev_pixels and dev_history come out
 * exactly as that call writes them, dropped index entries are counted in ptss_film_rejected — plus dev_moments[p] += the ray's squared
 * bytes; dev_moments null or not 8-byte aligned: PTSS_EINVAL. Without an index: one kernel, a plain read-modify-write of the 16-byte
 * entry and the 8-byte moment. With an index: the lanes of a wave that hold one pixel side by side (all of them, for a plan's sorted
 * index) are summed on chip and the run's first lane alone issues the atomics, four 32-bit and one 64-bit; duplicates that are not
 * neighbours meet in the atomics, so the sums are exact for every index. The touched pixels are resolved by a second launch.
 *
 * ptss_plan_samples: dev_index[0 .. n) = a budget of exactly n rays spread over the film's pixels in proportion to an integer weight.
 *   weight (csrc/ptadaptive.h; N = samples, S = the sums, Q = the moment; unsigned 64-bit wrapping arithmetic):
 *     N < minSamples: 2^19 (unsampled: it outranks every measured pixel). N >= maxSamples: 0 (capped). Otherwise D = max(N Q - |S|^2, 0),
 *     se = sqrt((float)D) / ((float)N sqrt((float)N)) — the standard error of the pixel's mean on the 0..255 scale, every operation
 *     correctly rounded f32 — and w = se > threshold ? (uint32_t)min(se * 1024.f, 524287.f) : 0.
 *   dev_cdf[p] = w_0 + .. + w_p for p < filmPixels (at most 2^50); the entries from filmPixels up to ptss_plan_cdf_entries(filmPixels)
 *     are the call's workspace, so the call keeps no state.
 *   total = dev_cdf[filmPixels - 1] > 0: t_i = floor((i total + total / 2) / n) and dev_index[i] = the smallest p with dev_cdf[p] > t_i.
 *   total = 0 (every pixel converged or capped): the same rule with every weight 1, dev_index[i] = (i filmPixels + filmPixels / 2) / n.
 *   The index is non-decreasing, never names a pixel of weight 0 while total > 0, and names pixel p count_p times with
 *   |count_p total - n w_p| < total. dev_info (may be NULL) is written by the device.
 * The host build of csrc/ptadaptive.h (ptss_probe_plan_samples) is the specification; the device agrees with it byte for byte, also
 * for moments that do not belong to the film.
 * Refused without touching the device and without counting: a null context, params or required pointer, a wrong structSize,
 * minSamples = 0, maxSamples outside [1, 2^23] or below minSamples, a threshold that is negative or not finite, a pointer that is not
 * aligned — 16 bytes for the film, 8 for moments, cdf and info, 4 for the index — (PTSS_EINVAL); filmPixels = 0 or >= 2^31, n >= 2^31
 * (PTSS_ERANGE). n = 0 returns PTSS_OK and launches nothing.
 *
 * Both calls are asynchronous on hipStream (NULL: the context's stream), leave no trace in frame state, own no bit of
 * ptss_launched_kernels and serve sharded contexts. ptss_adaptive_launches: the calls of each kind that launched since ptss_create
 * (ptss_film_launches does not count them). ptss_default_plan_params: minSamples 8, maxSamples 2^23, threshold 0.5 — design choices,
 * not measurements. */
int ptss_accumulate_paths_stats(ptss_context* ctx, const ptss_path_result* dev_results, const uint32_t* dev_index /* may be NULL */,
                                size_t firstPixel, size_t n, ptss_film_entry* dev_film, unsigned long long* dev_moments, size_t filmPixels,
                                ptss_uchar4* dev_pixels /* may be NULL */, ptss_history_entry* dev_history /* may be NULL */, void* hipStream);
int ptss_default_plan_params(ptss_plan_params* params);
int ptss_plan_cdf_entries(size_t filmPixels, size_t* entries); /* >= filmPixels */
int ptss_plan_samples(ptss_context* ctx, const ptss_film_entry* dev_film, const unsigned long long* dev_moments, size_t filmPixels,
                      const ptss_plan_params* params, size_t n, unsigned long long* dev_cdf, uint32_t* dev_index /* n entries out */,
                      ptss_plan_info* dev_info /* may be NULL */, void* hipStream);
int ptss_adaptive_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] stats accumulates, [1] plans */

/* The linear film: ptss_trace_paths' radiance accumulated as it is — not tone-mapped sample by sample — for probes,
 * light-map texels, panoramas and every use whose exposure is chosen afterwards. A pixel holds 64-bit unsigned fixed-point sums
 * (ptss_linear_entry), so the film is exact and the same bytes for every order of the samples, for every index, duplicates included, and
 * for every split of a batch into calls. csrc/ptlinear.h has the arithmetic; its host build (ptss_probe_accumulate_linear,
 * ptss_probe_resolve_linear) is the specification and the device agrees with it byte for byte.
 *
 * ptss_accumulate_paths_linear: for ray i, pixel p as in ptss_accumulate_paths, each channel x of dev_results[i].radiance becomes
 *   q = (u64) round-to-nearest-even(clamp'(x) * 2^scaleLog2), clamp': NaN -> 0, x < 0 (-inf and -0 included) -> 0, x > clampMax (+inf
 *   included) -> clampMax,
 * and is added to dev_film[p].r, .g, .b; .samples grows by 1, and .clamped by 1 when a channel was NaN or above clampMax (negative
 * channels do not count). q <= 2^40, so the sums stay below 2^63 while samples < 2^23. Without an index: one kernel, a plain
 * read-modify-write of the 32-byte entry. With an index: the lanes of a wave that hold one pixel side by side are summed on chip and
 * the run's first lane alone issues four 64-bit integer atomics (r, g, b, samples | clamped << 32). Index entries >= filmPixels are
 * dropped and counted in ptss_film_rejected. The caller zero-fills a new film. Nothing is resolved by this call.
 *
 * ptss_resolve_linear: for pixels firstPixel .. firstPixel + count of dev_film (the caller guarantees they exist), with N = samples:
 *   N = 0: dev_linear[p] = (0, 0, 0, 0), dev_pixels[p] = (0, 0, 0, 255), dev_history[p] = (0, 0, 0, 0). Otherwise, per channel,
 *   m = (sum + N / 2) / N in unsigned 64-bit integers, mean = (float)m * 2^-scaleLog2 (round to nearest even, then an exact multiply),
 *   e = mean * exposure; dev_linear[p] = {mean_r, mean_g, mean_b, (float)N} (unexposed), dev_pixels[p] = the frame's 8-bit tone map of e
 *   (the context's thresholds) with alpha 255 — the tone map of the mean, not the mean of tone maps —, dev_history[p] =
 *   {255 pow(clamp(e, 0, 1), 1 / 2.2) per channel, (float)N}: the entry ptss_denoise_history, ptss_reproject and ptss_upsample take.
 * Each of the three outputs may be NULL; all three NULL is PTSS_OK with nothing launched. One streaming kernel.
 *
 * Both calls are asynchronous on hipStream (NULL: the context's stream), leave no trace in frame state, own no bit of
 * ptss_launched_kernels and serve sharded contexts. Refused without touching the device and without counting: everything
 * ptss_accumulate_paths refuses; null params, a wrong structSize, scaleLog2 outside 0 .. 32, a clampMax that is not finite and positive
 * or has clampMax * 2^scaleLog2 > 2^40, an exposure that is negative or not finite, a non-zero reserved, a pointer that is not aligned
 * — 16 bytes for results, film, linear and history, 4 for index and pixels — (PTSS_EINVAL, also with n = 0 or count = 0 for the
 * parameters); the ranges ptss_accumulate_paths refuses, firstPixel + count >= 2^31 (PTSS_ERANGE). n = 0 and count = 0 return PTSS_OK.
 * ptss_linear_launches: the calls of each kind that launched since ptss_create. ptss_default_linear_params: scaleLog2 20, clampMax
 * 65536, exposure 1 — design choices, not measurements. A caller who wants a sampling plan on this film keeps its moments
 * with ptss_accumulate_paths_linear_stats and plans with ptss_plan_samples_linear (below). */
int ptss_default_linear_params(ptss_linear_params* params);
int ptss_accumulate_paths_linear(ptss_context* ctx, const ptss_path_result* dev_results, const uint32_t* dev_index /* may be NULL */,
                                 size_t firstPixel, size_t n, ptss_linear_entry* dev_film, size_t filmPixels, const ptss_linear_params* params,
                                 void* hipStream);
int ptss_resolve_linear(ptss_context* ctx, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                        ptss_history_entry* dev_linear /* may be NULL */, ptss_uchar4* dev_pixels /* may be NULL */,
                        ptss_history_entry* dev_history /* may be NULL */, void* hipStream);
int ptss_linear_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] accumulates, [1] resolves */

/* Adaptive sampling on the linear film: the film also keeps the first and second moment of its samples' luminance,
 * exactly, and the plan spends the next round by the relative standard error of a pixel's mean luminance — a quantity that does not
 * depend on the exposure chosen afterwards. csrc/ptlinstats.h has the arithmetic; its host build (ptss_probe_accumulate_linear_stats,
 * ptss_probe_plan_samples_linear) is the specification and the device agrees with it byte for byte.
 *
 * ptss_accumulate_paths_linear_stats: ptss_accumulate_paths_linear's arguments, refusals and film bytes, and for every ray that reaches
 * pixel p, with q_r, q_g, q_b that call's fixed-point channels: y = (54 q_r + 183 q_g + 19 q_b + 128) >> 8 (<= 2^40; the meter's
 * luminance), dev_moments[p].sumY += y, .sqLo += y^2 & (2^40 - 1), .sqHi += y^2 >> 40, .samples += 1. All sums are unsigned 64-bit
 * integers, below 2^64 while samples < 2^23 and wrapping beyond; they do not depend on the order of the samples, on the index or on the
 * split of a batch into calls. dev_film may be NULL: moments only (a filtered film keeps them by home pixel beside ptss_splat_paths).
 * Without an index: one kernel, a plain read-modify-write of the rows. With an index: runs of equal pixels inside a wave are summed on
 * chip and the run's first lane issues four 64-bit atomics for the moment row and four for the film entry. The caller zero-fills new
 * moments.
 *
 * ptss_plan_samples_linear: ptss_plan_samples over those moments. N = samples, Sy = sumY, Q = sqHi * 2^40 + sqLo: N < minSamples weighs
 * 2^19, N >= maxSamples 0; otherwise D = max(N Q - Sy^2, 0) in 128-bit integers, r = sqrt(D) as f32 (through a 64-bit mantissa with a
 * sticky bit when D >= 2^64), seY = r / (N sqrt N), meanY = Sy / N, rel = seY / (meanY + floor * 2^scaleLog2), every step correctly
 * rounded f32, and the weight is rel > threshold ? min(rel * 2^18, 2^19 - 1) : 0. Running sum, targets, search, the uniform fallback,
 * dev_cdf (ptss_plan_cdf_entries words), dev_index and dev_info are ptss_plan_samples'. Four launches, no host round trip.
 *
 * Both calls are asynchronous on hipStream (NULL: the context's stream), leave no trace in frame state, own no bit of
 * ptss_launched_kernels and serve sharded contexts; ptss_linear_launches and ptss_adaptive_launches do not count them. Refused without
 * touching the device and without counting: everything ptss_accumulate_paths_linear and ptss_plan_samples refuse about the arguments
 * they share; null or misaligned moments (16 bytes), null plan params, a wrong structSize, minSamples 0, maxSamples outside
 * [minSamples, 2^23], a threshold that is negative or not finite, a floor that is not finite, has floor * 2^scaleLog2 < 1 or exceeds
 * clampMax, a non-zero reserved (PTSS_EINVAL). n = 0 returns PTSS_OK with nothing launched. ptss_default_linear_plan_params: minSamples
 * 8, maxSamples 2^23, threshold 0.02, floor 1/64 — design choices, not measurements. ptss_linear_stats_launches: the calls of each kind
 * that launched since ptss_create. */
int ptss_default_linear_plan_params(ptss_linear_plan_params* params);
int ptss_accumulate_paths_linear_stats(ptss_context* ctx, const ptss_path_result* dev_results, const uint32_t* dev_index /* may be NULL */,
                                       size_t firstPixel, size_t n, ptss_linear_entry* dev_film /* may be NULL: moments only */,
                                       ptss_linear_moment* dev_moments, size_t filmPixels, const ptss_linear_params* params, void* hipStream);
int ptss_plan_samples_linear(ptss_context* ctx, const ptss_linear_moment* dev_moments, size_t filmPixels, const ptss_linear_params* params,
                             const ptss_linear_plan_params* plan, size_t n, unsigned long long* dev_cdf, uint32_t* dev_index,
                             ptss_plan_info* dev_info /* may be NULL */, void* hipStream);
int ptss_linear_stats_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] accumulates, [1] plans */

/* The filtered linear film: the linear film's fixed-point samples, spread over the pixels around the sample's position
 * by a box, a tent or a Gaussian pixel filter (ptss_splat_filter) whose weights are integers. Every contribution is an integer, so a
 * film (ptss_splat_entry, zero-filled by the caller) is exact and the same bytes for every order of the samples, every split of a batch
 * into calls and both kernel forms. csrc/ptsplat.h has the arithmetic; its host build (ptss_probe_splat_paths, ptss_probe_resolve_splat)
 * is the specification and the device agrees with it byte for byte.
 *
 * ptss_generate_rays_positions: ptss_generate_rays — the same rays and streams — and dev_positions[i] = (x + jx, y + jy), where sample i
 * lies on the film in pixels (the pixel's centre with jitter = 0). An index entry >= width * height writes no ray and no stream, is
 * counted in ptss_film_rejected, and gets the position (NaN, NaN), which every splat drops. dev_positions: required, 8-byte aligned.
 * It counts in ptss_film_launches()[0].
 *
 * A sample at (X, Y) and pixel (i, j): d = X - (i + 0.5), the per-axis profile f(d) in float32 — box: 1 for -R <= d < R; tent:
 * max(0, 1 - |d| / R); Gaussian: max(0, exp(-alpha d^2) - exp(-alpha R^2)) for |d| < R — wq = (uint32_t)(f * 65536 + 0.5) per axis, the
 * tap's weight W = (wqx * wqy + 32768) >> 16, and the entry of pixel (i, j) gains (q * W + 32768) >> 16 per channel, q the linear film's
 * fixed-point sample (ptss_linear_params: scaleLog2, clampMax), and W in weight. Taps outside the film and taps with W = 0 add nothing.
 *
 * ptss_splat_paths: any positions in any order, integer atomics. A sample with a coordinate that is not finite or outside
 * [-R, width + R] (resp. height) is dropped and counted.
 * ptss_splat_paths_homed: the caller states that sample i was aimed at pixel firstPixel + i (ptss_generate_rays_positions without an
 * index); a sample whose position is outside that pixel's closed square [hx, hx + 1] x [hy, hy + 1] (NaN included) is dropped and
 * counted. One thread per output pixel gathers its taps; no atomics, one plain read-modify-write per pixel: two calls on one film must
 * be ordered by the caller. The film's bytes equal ptss_splat_paths' on the same samples.
 * ptss_resolve_splat: for pixels firstPixel .. firstPixel + count, Wt = weight: Wt = 0 gives ptss_resolve_linear's N = 0 row; otherwise
 * per channel m = floor((S * 2^16 + Wt / 2) / Wt) exactly, mean = (float)m * 2^-scaleLog2, and the outputs of ptss_resolve_linear from
 * that mean, with (float)Wt * 2^-16 as the sample weight. With the box at radius 0.5 the film resolves to ptss_resolve_linear's bytes.
 *
 * All calls are asynchronous on hipStream (NULL: the context's), leave no trace in frame state, own no bit of ptss_launched_kernels and
 * serve sharded contexts. Refused without touching the device and without counting (PTSS_EINVAL): a null ctx, filter, params or
 * required buffer, a wrong structSize, an unknown kind, a radius outside [0.5, 2], a Gaussian's alpha that is not finite and positive,
 * a non-zero reserved, whatever ptss_accumulate_paths_linear refuses about params, a pointer that is not aligned (16 bytes for
 * results, film, linear and history, 8 for positions, 4 for pixels); (PTSS_ERANGE): width or height outside [1, 2^22], width * height
 * or n >= 2^31, firstPixel + n beyond the film. n = 0 and count = 0 return PTSS_OK with nothing launched.
 * ptss_splat_stats: [0] scatter launches, [1] homed launches, [2] resolves (counted on the host), [3] samples dropped, [4] samples kept
 * with a clamped channel (counted on the device: the call synchronises with the stream of the latest splat). ptss_default_splat_filter:
 * tent, radius 1, alpha 2 — design choices, not measurements. */
int ptss_default_splat_filter(ptss_splat_filter* filter);
int ptss_generate_rays_positions(ptss_context* ctx, const ptss_film_camera* film, size_t firstPixel, const uint32_t* dev_index /* may be NULL */,
                                 size_t n, ptss_path_rng* dev_rng, ptss_ray_query* dev_rays, ptss_film_position* dev_positions, void* hipStream);
int ptss_splat_paths(ptss_context* ctx, const ptss_path_result* dev_results, const ptss_film_position* dev_positions, size_t n,
                     ptss_splat_entry* dev_film, int width, int height, const ptss_splat_filter* filter, const ptss_linear_params* params,
                     void* hipStream);
int ptss_splat_paths_homed(ptss_context* ctx, const ptss_path_result* dev_results, const ptss_film_position* dev_positions, size_t firstPixel,
                           size_t n, ptss_splat_entry* dev_film, int width, int height, const ptss_splat_filter* filter,
                           const ptss_linear_params* params, void* hipStream);
int ptss_resolve_splat(ptss_context* ctx, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                       ptss_history_entry* dev_linear /* may be NULL */, ptss_uchar4* dev_pixels /* may be NULL */,
                       ptss_history_entry* dev_history /* may be NULL */, void* hipStream);
int ptss_splat_stats(ptss_context* ctx, unsigned long long* out5);

/* Metering a linear or a filtered linear film on the device: a luminance histogram of the film's pixel means, the
 * exposure it asks for, with temporal adaptation, kept in device memory, and the two resolves taking their exposure from there — the
 * loop generate, trace, accumulate, meter, resolve never returns to the host. csrc/ptmeter.h has the arithmetic; its host build
 * (ptss_probe_meter_bin, ptss_probe_meter_linear, ptss_probe_meter_splat, ptss_probe_meter_exposure) is the specification and the device
 * agrees with it byte for byte.
 *
 * ptss_meter_linear / ptss_meter_splat: for pixels firstPixel .. firstPixel + count of dev_film (the caller guarantees they exist), a
 * pixel with samples = 0 (weight = 0) is not metered; otherwise per channel m = the integer mean of the resolve — (sum + N / 2) / N, or
 * the filtered film's floor((S * 2^16 + Wt / 2) / Wt) — Y = (54 m_r + 183 m_g + 19 m_b + 128) >> 8, and dev_histogram[bin] gains 1:
 * bin 0 for Y = 0, else 1 + 8 e + sub with e = floor(log2 Y) and sub the three bits below Y's leading one (Y shifted up where e < 3).
 * A film the library filled has Y <= 2^40, bin <= 321; anything from 2^41 on counts in bin 328. dev_histogram: PTSS_METER_BINS
 * 32-bit counts the caller has zero-filled; the counts carry across calls (tiles, shards and rounds may meter into one histogram) and
 * wrap like any unsigned integer. Integer counts: the same bytes for every split into calls and every launch shape.
 *
 * ptss_meter_exposure: one update of *dev_state from dev_histogram (read, not cleared). With T = the counts of bins 1 .., lo = T *
 * lowPermille / 1000 and hi = T - T * highPermille / 1000, the ranks [lo, hi) of the non-black pixels in order of their bins are
 * averaged: sumLog = the sum over those ranks of the bin centre 2 (bin - 1) + 1 (in 1/16 stop), C = hi - lo, meanLog2 = sumLog / (C * 16)
 * - scaleLog2, target = clamp(key * exp(-meanLog2 * ln 2), minExposure, maxExposure); a new state (updates = 0) takes exposure = target,
 * any other exposure = clamp(fma(target - exposure, rate, exposure), minExposure, maxExposure). T = 0: target = exposure = the
 * previous exposure, 1 for a new state. updates grows by one, saturating. params: the film's ptss_linear_params (scaleLog2 is read).
 *
 * ptss_resolve_linear_metered / ptss_resolve_splat_metered: ptss_resolve_linear / ptss_resolve_splat with the exposure
 * dev_state->exposure * params->exposure (one float32 multiply; params->exposure compensates, default 1). No address depends on the
 * state: a state the caller filled with garbage gives garbage pixels, never a fault.
 *
 * All of them are asynchronous on hipStream (NULL: the context's), leave no trace in frame state, own no bit of ptss_launched_kernels
 * and serve sharded contexts like the film calls. Refused without touching the device and without counting (PTSS_EINVAL): a null ctx,
 * params or meter params, a wrong structSize, whatever ptss_resolve_linear refuses about params, a key that is not finite and positive,
 * permilles above 999 together, a rate outside [0, 1], exposure bounds that are negative, not finite or min > max, a non-zero reserved, a
 * null film, histogram or state, a pointer that is not aligned — 16 bytes for film, linear and history, 8 for the state, 4 for the
 * histogram and pixels; (PTSS_ERANGE): firstPixel + count >= 2^31. count = 0 returns PTSS_OK with nothing launched.
 * ptss_meter_launches: the calls of each kind that launched since ptss_create. ptss_default_meter_params: key 0.18, lowPermille 100,
 * highPermille 20, rate 1, minExposure 2^-16, maxExposure 2^16 — design choices, not measurements. */
int ptss_default_meter_params(ptss_meter_params* params);
int ptss_meter_linear(ptss_context* ctx, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, uint32_t* dev_histogram,
                      void* hipStream);
int ptss_meter_splat(ptss_context* ctx, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, uint32_t* dev_histogram,
                     void* hipStream);
int ptss_meter_exposure(ptss_context* ctx, const uint32_t* dev_histogram, const ptss_linear_params* params, const ptss_meter_params* meter,
                        ptss_meter_state* dev_state /* in/out */, void* hipStream);
int ptss_resolve_linear_metered(ptss_context* ctx, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count,
                                const ptss_linear_params* params, const ptss_meter_state* dev_state,
                                ptss_history_entry* dev_linear /* may be NULL */, ptss_uchar4* dev_pixels /* may be NULL */,
                                ptss_history_entry* dev_history /* may be NULL */, void* hipStream);
int ptss_resolve_splat_metered(ptss_context* ctx, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count,
                               const ptss_linear_params* params, const ptss_meter_state* dev_state,
                               ptss_history_entry* dev_linear /* may be NULL */, ptss_uchar4* dev_pixels /* may be NULL */,
                               ptss_history_entry* dev_history /* may be NULL */, void* hipStream);
int ptss_meter_launches(const ptss_context* ctx, unsigned long long* out3); /* [0] histograms, [1] exposure updates, [2] metered resolves */

/* Glare for the two linear films: highlights that bleed, taken between the film and the tone map, where the energy
 * above display white still exists. csrc/ptglare.h has the arithmetic; its host build (ptss_probe_glare_build,
 * ptss_probe_resolve_glare) is the specification and the device equals it byte for byte. Everything in front of the resolve's float steps
 * is unsigned 64-bit integer work, so a pyramid is the same bytes whatever kernels built it.
 *
 * ptss_glare_layout: the levels of a pyramid over a width x height film, out[k - 1] for level k = 1 .. levels: (w + 1) / 2 x (h + 1) / 2
 * of the level below, level 0 being the film; the levels lie one behind the other, *entries ptss_glare_entry in all.
 *
 * ptss_glare_build: the whole film. Per pixel and channel m = the integer mean of the resolve (0 for a pixel without samples), t =
 * glare->threshold in the film's fixed point, the source b = m > t ? m - t : 0. d_k(i, j) = (the 4 x 4 texels 2i-1 .. 2i+2 x 2j-1 .. 2j+2
 * of level k - 1, weights (1, 3, 3, 1) per axis, coordinates clamped, + 32) >> 6; then from the coarsest level u_L = d_L, u_k = d_k +
 * up(u_{k+1}), up at x = 2i taking 3 a[i] + a[i-1], at x = 2i + 1 taking 3 a[i] + a[i+1], the axes multiplied, (sum + 8) >> 4. Afterwards
 * dev_pyramid holds u_1 .. u_L. One launch for the film, one per large level and direction, and one for all the small levels together.
 *
 * ptss_resolve_linear_glare / ptss_resolve_splat_glare: ptss_resolve_linear / ptss_resolve_splat of pixels firstPixel .. firstPixel +
 * count with g = (up(u_1) + L / 2) / L, s = (uint32_t)(strength * 65536 + 0.5) and m' = (m * k + g * s + 32768) >> 16 shown in place of m:
 * k = 65536 (PTSS_GLARE_ADD) or 65536 - s (PTSS_GLARE_MIX). The weight of linear and history stays the pixel's own; a pixel without
 * samples that receives no glare is the plain resolve's empty row, so strength = 0 gives the plain resolve's bytes. dev_state: NULL, or
 * a meter's state: the exposure is state->exposure * params->exposure. glare must be what the pyramid was built with (levels above all).
 *
 * Refused before the device is touched, nothing counted. PTSS_EINVAL: a null ctx, film, pyramid, params or glare, a wrong structSize,
 * whatever ptss_resolve_linear refuses about params, levels outside [1, 8], an unknown mode or film kind, a strength outside [0, 1], a
 * threshold that is negative, not finite or with threshold * 2^scaleLog2 > 2^40, a non-zero reserved, a film, pyramid, linear or history
 * pointer that is not 16-byte aligned, a state that is not 8-byte, pixels that are not 4-byte aligned. PTSS_ERANGE: width or height
 * outside [1, 2^22], width * height >= 2^31, firstPixel + count beyond the film. count = 0 returns PTSS_OK.
 * ptss_default_glare_params: levels 6, PTSS_GLARE_MIX, threshold 0, strength 0.1 (design choices, not measurements). */
int ptss_default_glare_params(ptss_glare_params* params);
int ptss_glare_layout(int width, int height, int levels, ptss_glare_level out[8], size_t* entries);
int ptss_glare_build(ptss_context* ctx, const void* dev_film, int filmKind /* PTSS_GLARE_FILM_LINEAR | PTSS_GLARE_FILM_SPLAT */, int width,
                     int height, const ptss_linear_params* params, const ptss_glare_params* glare, ptss_glare_entry* dev_pyramid,
                     void* hipStream);
int ptss_resolve_linear_glare(ptss_context* ctx, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count,
                              const ptss_linear_params* params, int width, int height, const ptss_glare_params* glare,
                              const ptss_glare_entry* dev_pyramid, const ptss_meter_state* dev_state /* may be NULL */,
                              ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream);
int ptss_resolve_splat_glare(ptss_context* ctx, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count,
                             const ptss_linear_params* params, int width, int height, const ptss_glare_params* glare,
                             const ptss_glare_entry* dev_pyramid, const ptss_meter_state* dev_state /* may be NULL */,
                             ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream);
int ptss_glare_launches(const ptss_context* ctx, unsigned long long* out3); /* [0] builds, [1] kernels launched inside them, [2] glare resolves */

/* Denoising the two linear films in linear light: an edge-avoiding A-trous filter between the accumulation and the
 * meter, the glare and the resolve, whose luminance tolerance is each pixel's own measured error — the standard error of its mean
 * luminance, from the exact moments ptss_accumulate_paths_linear_stats keeps — and whose result is a linear film again, so
 * ptss_meter_linear, ptss_glare_build (PTSS_GLARE_FILM_LINEAR) and every ptss_resolve_linear* take it as they are. csrc/ptlindn.h has
 * the arithmetic; its host build (ptss_probe_denoise_linear) is the specification and the device equals it byte for byte.
 *
 * ptss_denoise_linear: the whole film. dev_film: width * height entries, ptss_linear_entry or (PTSS_FILM_SPLAT) ptss_splat_entry;
 * dev_moments: the film's moment rows (on a filtered film they are kept by home pixel and each row's own count applies); dev_features:
 * what ptss_render_features, ptss_render_features_specular or ptss_ray_features wrote for the film's pixels; dev_workspace:
 * ptss_denoise_linear_workspace bytes (52 per pixel), the caller's, free again when the call's work on the stream is done; dev_out:
 * width * height ptss_linear_entry, not the film itself. A pixel without samples (or weight) has no colour: no pass reads it and its
 * output row is zero. Every other pixel's output row is {m' K, m' K, m' K, samples = K, clamped}, m' the filtered mean rounded to the
 * film's fixed point and K the entry's samples (a filtered film: its weight rounded to samples, at least 1, clamped = 0): the integer
 * mean every consumer takes of it is m' exactly. levels = 0 copies the means (the output's resolve, meter and glare bytes are the
 * input's). The moments are not changed and keep describing the unfiltered samples (ptss_plan_samples_linear goes on reading them).
 * Asynchronous on hipStream (NULL: the context's); no frame state, serves sharded contexts; two calls sharing a workspace are ordered
 * by the caller.
 *
 * Refused before the device is touched, nothing counted. PTSS_EINVAL: a null ctx or required pointer, a wrong structSize, an unknown
 * film kind, levels outside [0, 6], a sigma that is not finite and positive, a non-zero reserved, whatever ptss_resolve_linear refuses
 * about params, a pointer that is not 16-byte aligned, dev_out equal to dev_film, dev_out or dev_film inside the workspace.
 * PTSS_ERANGE: width or height outside [1, 2^22], width * height >= 2^31.
 * ptss_default_denoise_linear_params: levels 5, sigmaLuminance 3, sigmaNormal 0.1, sigmaDepth 4 (design choices, not measurements).
 * ptss_debug_denoise_linear_form: tests and measurements only. 0 (the default): every pass runs the kernel form measured faster at its
 * spacing; 1: taps from global memory at every spacing; 2: tile and halo staged in LDS wherever that kernel exists; 4 + mask (4 .. 11):
 * staged at pass k (spacing 2^k, k = 0 .. 2) where bit k of the mask is set. Same bytes whatever the form. */
int ptss_default_denoise_linear_params(ptss_denoise_linear_params* params);
int ptss_denoise_linear_workspace(int width, int height, size_t* bytes);
int ptss_denoise_linear(ptss_context* ctx, const void* dev_film, int filmKind /* PTSS_FILM_LINEAR | PTSS_FILM_SPLAT */, int width, int height,
                        const ptss_linear_moment* dev_moments, const ptss_pixel_feature* dev_features, const ptss_linear_params* params,
                        const ptss_denoise_linear_params* denoise, void* dev_workspace, ptss_linear_entry* dev_out, void* hipStream);
int ptss_denoise_linear_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] calls that launched, [1] kernels inside them */
int ptss_debug_denoise_linear_form(ptss_context* ctx, int form);

/* Carrying the two linear films across a camera move: the previous pose's film SEEDS the new pose's film once. For
 * each pixel of the `now` film the call looks the previous film up through the first-hit features (four bilinear taps, a tap counting
 * only where material, normal and depth agree and the previous entry is not empty) and writes {m' K, m' K, m' K, K}: the reprojected
 * mean m' at the film's fixed point times an integer history count K <= maxHistory, with a moment row whose standard error is the
 * reprojected per-sample variance over K. From there the film is an ordinary film: ptss_accumulate_paths_linear*, ptss_splat_paths*
 * add to it, ptss_plan_samples_linear, ptss_denoise_linear, the meters, ptss_glare_build and every linear resolve take it as it is, and
 * the history fades by itself as samples arrive. A pixel without history (disoccluded, off the previous film) is an all-zero row: the
 * plan ranks it "unsampled". csrc/ptlinrp.h has the arithmetic; its host build (ptss_probe_reproject_linear) is the specification
 * and the device equals it byte for byte.
 *
 * now, prev: the two poses' film cameras; they may differ in kind and size, prev->width x prev->height being the size of
 * dev_features_prev, dev_film_prev and dev_moments_prev. `jitter` of both is not read: the centre ray is always used, and
 * dev_features_now / dev_features_prev are ptss_ray_features of exactly those rays (ptss_generate_rays with jitter = 0).
 * dev_motion_now (may be NULL): where each hit point was in the previous pose; valid only when the `now` film is the context's own
 * pinhole camera at the context's size, because that is where ptss_render_features_motion writes rows — the call cannot check more
 * than the pointer. dev_film_prev / dev_film_out: ptss_linear_entry or (PTSS_FILM_SPLAT) ptss_splat_entry, both the same kind;
 * dev_film_out has now->width * now->height entries, all written. dev_moments_prev (may be NULL) and dev_moments_out are given
 * together or not at all. dev_info (may be NULL): four counters the call ADDS to; the caller zero-fills.
 * Asynchronous on hipStream (NULL: the context's); no frame state, no bit of ptss_launched_kernels, serves sharded contexts.
 *
 * Refused with PTSS_EINVAL before the device is touched, nothing written or counted: a null ctx or required pointer, a wrong
 * structSize, a parameter outside its range, a camera ptss_generate_rays refuses, a side above 2^22 or width * height >= 2^31, whatever
 * ptss_resolve_linear refuses about `film`, an unknown film kind, moments given on one side only, a film, moment or feature pointer
 * that is not 16-byte aligned (dev_info: 8), an output range that overlaps the previous film or moments or the other output. */
int ptss_default_reproject_linear_params(ptss_reproject_linear_params* params);
int ptss_reproject_linear(ptss_context* ctx, const ptss_film_camera* now, const ptss_pixel_feature* dev_features_now,
                          const ptss_pixel_motion* dev_motion_now /* may be NULL */, const ptss_film_camera* prev,
                          const ptss_pixel_feature* dev_features_prev, const void* dev_film_prev,
                          int filmKind /* PTSS_FILM_LINEAR | PTSS_FILM_SPLAT */, const ptss_linear_moment* dev_moments_prev /* may be NULL */,
                          const ptss_linear_params* film, const ptss_reproject_linear_params* params, void* dev_film_out,
                          ptss_linear_moment* dev_moments_out /* NULL exactly when dev_moments_prev is */,
                          ptss_reproject_linear_info* dev_info /* may be NULL */, void* hipStream);
int ptss_reproject_linear_launches(const ptss_context* ctx, unsigned long long* out); /* calls that launched */

/* Upsampling the two linear films in linear light: a linear or a filtered linear film of width x height becomes a
 * LINEAR film of factor * width x factor * height, between ptss_denoise_linear and the meter, the glare build and the resolves, which
 * take the result exactly as it is — the glare pyramid is built at the large size, the exposure can change afterwards, and edges are
 * interpolated in linear light, in front of the tone map. Per hi pixel the four lo pixels around its centre (ptss_upsample's taps and
 * bilinear weights) count where they are inside the film, hold samples and have the hi pixel's material, weighted by the normal and
 * depth terms of ptss_upsample; the weighted mean of their means, written around the nearest counted one and clamped to their hull,
 * is rounded to the film's fixed point as m' and the row is {m' K, m' K, m' K, samples = K, clamped = 0}, K the nearest counted tap's
 * count: every consumer's integer mean of it is m' exactly. A channel in which all counted taps agree keeps their integer mean itself.
 * No tap counted: the nearest lo pixel's own means and count, or an all-zero row where that pixel is empty. csrc/ptlinup.h has the
 * arithmetic; its host build (ptss_probe_upsample_linear) is the specification and the device equals it byte for byte.
 *
 * dev_film_lo: ptss_linear_entry or (PTSS_FILM_SPLAT) ptss_splat_entry, width * height of them; dev_film_hi: factor^2 * width * height
 * ptss_linear_entry, all written. dev_features_lo / dev_features_hi: ptss_render_features / ptss_render_features_scaled of the same
 * camera, or ptss_ray_features of the centre rays (jitter = 0) of the same film camera at width x height and at factor * width x
 * factor * height (thin-lens and equirect films). params->flags & PTSS_UPSAMPLE_LINEAR_WRAP_X: an equirect film — tap columns and
 * the depth slope's left and right neighbours wrap at the seam. dev_info (may be NULL): three counters the call ADDS to; the caller
 * zero-fills; they sum to the large film's pixels. Asynchronous on hipStream (NULL: the context's); no frame state, no bit of
 * ptss_launched_kernels; the sizes are the caller's, so it serves sharded contexts. No moments are written for the large film: the
 * plan and the denoiser work at the small size.
 *
 * Refused before the device is touched, nothing written or counted. PTSS_EINVAL: a null ctx or required pointer, a wrong structSize,
 * a factor outside 1..4, a sigma that is not finite and positive, an unknown flag, a non-zero reserved, an unknown film kind, whatever
 * ptss_resolve_linear refuses about `film`, a film or feature pointer that is not 16-byte aligned (dev_info: 8), an output range that
 * overlaps the input film. PTSS_ERANGE: width or height outside [1, 2^22], factor * width or factor * height above 2^22,
 * factor^2 * width * height >= 2^31.
 * ptss_debug_upsample_linear_form (tests and measurements): 0 the form measured faster at each factor, 1 every tap from global
 * memory, 2 the lo pixels of a tile divided once and staged in LDS. The bytes are the same whatever the form. */
int ptss_default_upsample_linear_params(ptss_upsample_linear_params* params); /* factor 2, sigmaNormal 0.1, sigmaDepth 4, flags 0 */
int ptss_upsample_linear(ptss_context* ctx, const void* dev_film_lo, int filmKind /* PTSS_FILM_LINEAR | PTSS_FILM_SPLAT */, int width, int height,
                         const ptss_pixel_feature* dev_features_lo, const ptss_pixel_feature* dev_features_hi, const ptss_linear_params* film,
                         const ptss_upsample_linear_params* params, ptss_linear_entry* dev_film_hi,
                         ptss_upsample_linear_info* dev_info /* may be NULL */, void* hipStream);
int ptss_upsample_linear_launches(const ptss_context* ctx, unsigned long long* out); /* calls that launched */
int ptss_debug_upsample_linear_form(ptss_context* ctx, int form);

/* Tone curves for the two linear films: a shoulder instead of the hard clip at display white, the sRGB transfer
 * function, 10 bits. The last step of generate -> trace -> accumulate -> denoise -> reproject -> upsample -> meter -> glare -> resolve.
 * csrc/pttone.h has the arithmetic; its host build (ptss_probe_tone_*) is the specification and the device equals it byte for byte. A
 * quantised curve is a step function of its input, so it is fully described by its thresholds: whatever the curve costs in float
 * operations, the pixel is a search in a table, and THE TABLE IS THE SPECIFICATION OF THE PIXEL: the level of x is the number of k in
 * 1 .. K (K = 2^bits - 1) with x >= T[k]; NaN and negatives give 0.
 *
 * ptss_default_tone_params: PTSS_TONE_FILMIC, PTSS_TRANSFER_SRGB, 8 bits, no flags, white 4, filmic 2.51, 0.03, 2.43, 0.59, 0.14 (design
 * choices, not measurements). ptss_tone_table_floats: the floats of a table, 2^bits + 4 (0 for other bits).
 *
 * ptss_tone_build: the table of `tone` on the device, by one kernel of one thread per threshold and 31 bisection steps of the literal
 * level; nothing returns to the host. T[0] = -inf, T[1 .. K], T[K + 1] = NaN, T[K + 2] = 0 — or 1 where the thresholds came out of order,
 * which the bisections' shared midpoints rule out (csrc/pttone.h) and which a caller can read back —, T[K + 3] = T[K + 4] = NaN. dev_table: 16-byte aligned. The bytes
 * are ptss_probe_tone_build's.
 *
 * ptss_resolve_toned: the six linear resolves behind one entry point, shown through the table. filmKind: the film is ptss_linear_entry
 * or ptss_splat_entry. dev_state: NULL or a meter's state (the exposure is state->exposure * params->exposure). glare with dev_pyramid:
 * both NULL, or the parameters and the pyramid of ptss_glare_build for this film (width and height are read only then): the glare
 * resolves' m'. Channel input x_c = mean_c * exposure, or with PTSS_TONE_LUMINANCE x_c scaled by curve(Y) / Y of the exposed luminance Y,
 * the table being that of the clamp. dev_linear: the unexposed means and the weight, as every linear resolve writes them; dev_pixels: one
 * 32-bit word per pixel, r | g << 8 | b << 16 | 255 << 24 at 8 bits, r | g << 10 | b << 20 | 3 << 30 at 10; dev_history: 255 * the literal
 * display value of x_c and the weight, on the denoiser's 0 .. 255 scale at either depth. A pixel without samples or weight gives the
 * empty row (zeros, the alpha bits set). Each output may be NULL. tone must be what dev_table was built from. PTSS_TONE_CLAMP with
 * PTSS_TRANSFER_GAMMA22 at 8 bits without flags writes the bytes of the plain, metered and glare resolves.
 * Asynchronous on hipStream (NULL: the context's), no frame state, any shard. Nothing to write (count == 0 or all three outputs NULL) is
 * PTSS_OK without a launch. Refused before the device is touched, nothing counted: whatever the sibling resolves refuse, and PTSS_EINVAL
 * for an unknown film kind, a null or misaligned table, a tone structSize, curve, transfer, flag, bits, white, filmic[] or reserved
 * outside what ptss_types.h states, a pyramid without glare parameters.
 * ptss_debug_tone_form (tests and measurements): 0 the shipped lookup, 1 the table staged in LDS and a branch-free binary search, 2 a
 * first guess from the hardware log2 / exp2 settled by exact comparisons against the table in global memory. The bytes are the same. */
int ptss_default_tone_params(ptss_tone_params* params);
size_t ptss_tone_table_floats(int bits);
int ptss_tone_build(ptss_context* ctx, const ptss_tone_params* tone, float* dev_table, void* hipStream);
int ptss_resolve_toned(ptss_context* ctx, const void* dev_film, int filmKind /* PTSS_FILM_LINEAR | PTSS_FILM_SPLAT */, size_t firstPixel, size_t count,
                       const ptss_linear_params* params, const ptss_tone_params* tone, const float* dev_table,
                       const ptss_meter_state* dev_state /* may be NULL */, int width, int height, const ptss_glare_params* glare /* may be NULL */,
                       const ptss_glare_entry* dev_pyramid /* NULL with glare NULL */, ptss_history_entry* dev_linear, uint32_t* dev_pixels,
                       ptss_history_entry* dev_history, void* hipStream);
int ptss_tone_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] table builds, [1] toned resolves */
int ptss_debug_tone_form(ptss_context* ctx, int form);

/* Light maps and probes on the scene's own surfaces: rays that leave from surface points, made on the device from
 * the scene image, and the gutter fill of a baked film. With them the chain generate -> trace -> accumulate -> plan -> meter -> resolve
 * is a baker: the film is indexed by texel number, the index of a round is the texels of its rays. csrc/ptsurface.h has the arithmetic;
 * its host build (ptss_probe_surface_rays, ptss_probe_dilate_linear) is the specification and the device equals it byte for byte.
 *
 * ptss_generate_rays_surface: ray i leaves from point p = dev_index ? dev_index[i] : firstPoint + i of dev_points[0 .. numPoints), with
 * stream dev_rng[i], which is stored back advanced by the mode's draws (PTSS_SURFACE_NORMAL: none — the stream is neither read nor
 * written; PTSS_SURFACE_COSINE: two). Several rays may share a point. direction: unit length; origin: the point bumped along its
 * normal as scatter() bumps a Lambert ray; tmax = params->maxDistance; pad = 0. dev_surfels[i], when given, is the ptss_ray_hit a ray
 * arriving at the point would report: point, distance 0, the unit normal on the side the flags name, materialIdx, kind, primitive,
 * w1 = a and w2 = b (0 for spheres). The geometry is read from the scene image in use (ptss_update_triangles, ptss_resort_triangles and
 * ptss_set_scene are seen; the caller orders the calls on their streams as those calls ask).
 * An entry is REJECTED — no row written, the stream left as it is, counted (ptss_surface_rejected, which synchronises with the stream
 * of the latest call) — when its index is at or above numPoints, its surface is negative or names a primitive the scene does not hold,
 * a and b are outside the primitive (ptss_types.h), or a reserved flag bit is set.
 *
 * ptss_dilate_linear: one gutter-fill pass over a width x height linear film into dev_out, which must not be dev_film: a texel with
 * samples is copied; an empty one receives the field-by-field integer sum of its up to eight neighbours that hold samples — their
 * sample-weighted mean, an ordinary film row — or stays all zero. Repeat the pass for wider gutters.
 *
 * Both are asynchronous on hipStream (NULL: the context's), read the scene image at most, leave no frame state, serve any shard and own
 * no bit of ptss_launched_kernels. n = 0 returns PTSS_OK. Refused before the device is touched, nothing counted: PTSS_EINVAL a null
 * context, a null required pointer, a wrong structSize, an unknown mode, a non-zero reserved, a maxDistance that is not positive, a
 * pointer that is not aligned (16 bytes for points, rays, surfels and films, 4 for streams and indices), dev_out == dev_film;
 * PTSS_ERANGE n >= 2^31, numPoints >= 2^31, width or height below 1 or width * height >= 2^31, firstPoint + n beyond numPoints without
 * an index.
 * ptss_debug_dilate_linear_form (tests and measurements): 0 the shipped form, 1 the nine rows from global memory, 2 a 32 x 8 tile with
 * a ring of one staged in LDS. The bytes are the same. */
int ptss_generate_rays_surface(ptss_context* ctx, const ptss_surface_params* params, const ptss_surface_point* dev_points, size_t numPoints,
                               size_t firstPoint, const uint32_t* dev_index /* may be NULL */, size_t n, ptss_path_rng* dev_rng /* in/out */,
                               ptss_ray_query* dev_rays, ptss_ray_hit* dev_surfels /* may be NULL */, void* hipStream);
int ptss_dilate_linear(ptss_context* ctx, const ptss_linear_entry* dev_film, int width, int height, ptss_linear_entry* dev_out, void* hipStream);
int ptss_surface_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] generate, [1] dilate calls that launched */
int ptss_surface_rejected(ptss_context* ctx, unsigned long long* out);
int ptss_debug_dilate_linear_form(ptss_context* ctx, int form);

/* Reading a baked light map back: hits in, ordinary linear film rows out — one closest-hit query per pixel and a
 * four-tap lookup instead of a path-traced round. dev_hits are whatever the caller has: ptss_intersect of ptss_generate_rays' centre
 * rays for a camera view, the hits of reflection rays, ptss_generate_rays_surface's surfels. dev_blocksTri / dev_blocksSph are
 * ptss_surface_atlas_blocks' tables (ptss_host.h) on the device: row k of the triangles belongs to the caller's triangle
 * params->firstTriangle + k, k < numTriangleBlocks, the spheres alike; dev_map is the baked film of atlasWidth x atlasHeight entries,
 * before or after ptss_dilate_linear. csrc/ptlightmap.h has the arithmetic and its head comment is the specification; its host build
 * (ptss_probe_lookup_lightmap) and the device agree byte for byte.
 *
 * Per hit: the block of its primitive; the place in it (a triangle's w1, w2; a sphere's longitude and latitude from the hit's normal);
 * four taps with integer weights in 1/65536 (PTSS_LIGHTMAP_NEAREST: one), columns clamped on a triangle block and wrapped on a sphere
 * block, rows clamped — no tap leaves its block; the weighted mean m' of the integer means of the taps that hold samples, exact;
 * PTSS_LIGHTMAP_MODULATE: times the hit's diffuseColor in 1/65536 (the radiance a Lambert surface sends out: the baker's cosine-
 * weighted mean of the incoming radiance is E / pi); PTSS_LIGHTMAP_EMISSION: plus the hit's emmitance at the film's fixed point.
 * dev_out[i] = {m'_r, m'_g, m'_b, samples = 1, clamped = 0}, which every consumer of a linear film takes (the meter, the glare build,
 * ptss_denoise_linear, ptss_upsample_linear, every resolve); all zero for a hit with a block but no tap that holds samples (EMPTY),
 * without a block (a miss, a primitive outside the tables, a row with width == 0: NO BLOCK), or REJECTED: a kind outside 0..2, a w1, w2
 * or normal that is not finite, a block row that leaves the atlas (x, y, width or height negative, height 0, x + width > atlasWidth,
 * y + height > atlasHeight, width > 8192, height > 4096), or, with either flag, a materialIdx the scene image does not hold. Block
 * rows and hits are device memory and never trusted: no address is formed from a rejected one. All n rows are written.
 * dev_info (may be NULL): four uint32 counts ADDED to — filtered, empty, no block, rejected; they add up to n.
 *
 * Asynchronous on hipStream (NULL: the context's); reads the scene image only for materials; leaves no frame state; owns no bit of
 * ptss_launched_kernels; counted by ptss_lightmap_launches. n = 0 returns PTSS_OK. Refused before the device is touched, nothing
 * counted: PTSS_EINVAL a null context, a null required pointer (a block table may be NULL with a count of 0), a wrong structSize of
 * either params, an unknown filter or flag, a non-zero reserved, film parameters ptss_accumulate_paths_linear refuses, a pointer that
 * is not aligned (16 bytes for blocks, map, hits and out, 4 for info), dev_out overlapping dev_map; PTSS_ERANGE n >= 2^31, an atlas
 * side below 1 or atlasWidth * atlasHeight >= 2^31, a negative first or count.
 * ptss_default_lightmap_params: a 1 x 1 atlas, bilinear, no flags, empty tables. ptss_debug_lightmap_form (tests and measurements):
 * 0 the shipped form, 1 one lane per hit, 2 four lanes per hit. The bytes are the same. */
int ptss_default_lightmap_params(ptss_lightmap_params* params);
int ptss_lookup_lightmap(ptss_context* ctx, const ptss_lightmap_params* params, const ptss_linear_params* film,
                         const ptss_surface_block* dev_blocksTri /* may be NULL with 0 */, const ptss_surface_block* dev_blocksSph /* may be NULL with 0 */,
                         const ptss_linear_entry* dev_map, const ptss_ray_hit* dev_hits, size_t n, ptss_linear_entry* dev_out /* n rows, all written */,
                         uint32_t* dev_info /* may be NULL: 4 counts, added to */, void* hipStream);
int ptss_lightmap_launches(const ptss_context* ctx, unsigned long long* out);
int ptss_debug_lightmap_form(ptss_context* ctx, int form);

/* Ray queries that follow mirrors and glass: the fourth member of the query family. ptss_intersect for n caller rays,
 * each carried through the delta lobes of what it meets — perfect reflection, refraction; which one is decided from the material alone,
 * csrc/ptspecular.h, the chain of ptss_render_features_specular — for at most maxSteps links (0 .. 8). The first link's query runs
 * with the ray's own tmax, later links with +inf. The chain ends at a material the chain does not follow (diffuse, glossy,
 * Cook-Torrance, total internal reflection without a specular lobe), a miss, a continued direction that is not finite, or maxSteps.
 * dev_hits[i]: the ptss_ray_hit ptss_intersect writes for the LAST link's ray, the miss row included; maxSteps = 0 writes
 * ptss_intersect's bytes. dev_chain[i] (may be NULL): what the chain did on the way (ptss_types.h) — the throughput, the product of
 * the followed links' factors (ptsp::linkFactor: the followed lobe's probability in the reference's scatter times its weight), the
 * steps, the last ray's direction and the path length. The host composition — ptss_intersect, ptss_probe_specular_link
 * (ptss_host.h), ptss_intersect, .. — gives the same bytes.
 * options (NULL: the defaults, ptss_default_chain_options: structSize, PTSS_CHAIN_LANE_PER_RAY, 0, 0) picks the schedule.
 * PTSS_CHAIN_REFILL hands the next unclaimed ray of the batch to a lane whose chain has ended (ptss_trace_paths_opt's schedule, with a
 * queue head of its own: chain calls and path queries do not disturb each other); maxWorkgroups caps its grid (0: the resident
 * workgroups). Every output byte is the same for both schedules and every grid. ORDERING: ptss_trace_paths_opt's rule — the
 * PTSS_CHAIN_REFILL calls of one context must be ordered among themselves by the caller (one stream, or an event between streams).
 * Asynchronous on hipStream (NULL: the context's); reads the scene image only — the live one, after ptss_update_triangles and
 * ptss_resort_triangles —; leaves no frame state; owns no bit of ptss_launched_kernels; ptss_chain_launches counts since ptss_create:
 * out2[0] launches with one lane per ray, out2[1] with the refill schedule. n = 0 returns PTSS_OK. Refused before the device is touched,
 * nothing counted: PTSS_EINVAL a null context, null rays or hits with n > 0, a wrong structSize, an unknown schedule, a non-zero
 * reserved, a negative maxWorkgroups, a pointer that is not 16-byte aligned, outputs that overlap the rays or each other; PTSS_ERANGE
 * maxSteps outside 0 .. 8, n >= 2^31. */
int ptss_default_chain_options(ptss_chain_options* options);
int ptss_intersect_chain(ptss_context* ctx, const ptss_ray_query* dev_rays, size_t n, int maxSteps /* 0..8 */,
                         const ptss_chain_options* options /* NULL: defaults */, ptss_ray_hit* dev_hits,
                         ptss_chain_result* dev_chain /* may be NULL */, void* hipStream);
int ptss_chain_launches(const ptss_context* ctx, unsigned long long* out2); /* [0] lane per ray, [1] refill */

/* ptss_lookup_lightmap for hits seen through a chain: the same arguments, checks, verdicts and counts, plus dev_chain,
 * n rows of ptss_chain_result (16-byte aligned, required, device memory and never trusted). A FILTERED row is tinted after SHADE:
 * per channel m' = (m' t + 32768) >> 16 with t = clamp((int)(throughput * 65536 + 0.5f), 0, 65536) — a throughput that is not a number
 * or negative gives 0, a throughput ABOVE 1 IS CLAMPED TO 1. A throughput of exactly (1, 1, 1) gives ptss_lookup_lightmap's bytes.
 * Also refused (PTSS_EINVAL): dev_out overlapping dev_chain or dev_hits. Counted by ptss_lightmap_chain_launches, not by
 * ptss_lightmap_launches. The host build is ptss_probe_lookup_lightmap_chain. */
int ptss_lookup_lightmap_chain(ptss_context* ctx, const ptss_lightmap_params* params, const ptss_linear_params* film,
                               const ptss_surface_block* dev_blocksTri /* may be NULL with 0 */,
                               const ptss_surface_block* dev_blocksSph /* may be NULL with 0 */, const ptss_linear_entry* dev_map,
                               const ptss_ray_hit* dev_hits, const ptss_chain_result* dev_chain, size_t n,
                               ptss_linear_entry* dev_out /* n rows, all written */, uint32_t* dev_info /* may be NULL: 4 counts, added to */,
                               void* hipStream);
int ptss_lightmap_chain_launches(const ptss_context* ctx, unsigned long long* out);

/* First-hit features of the context's CURRENT camera for a frame of factor * width x factor * height, factor 1 .. 4 (DESIGN.md
 * §3.22): what ptss_upsample is guided by. The entry of hi-res pixel (X, Y) holds what ptss_intersect returns for
 * ptss_camera_ray(camera, factor * width, factor * height, X, Y, 0.5, 0.5) with tmax = +inf, albedo and the miss row as in
 * ptss_render_features — byte for byte what ptss_render_features of a context created at the larger size writes; factor = 1 writes
 * what ptss_render_features writes. dev_features_hi: factor^2 * local pixels entries, hi-res rows in the order of the local rows
 * (ptss_local_rows), `factor` hi-res rows per local row: a pixel-band shard (tileWorld > 1) gets the hi-res rows that cover its
 * own rows. The kernel is ptss_render_features' with the larger frame's shape and eye constants: ptss_launched_kernels reports it
 * at PTSS_KERNEL_FEATURES + inLds. Asynchronous on hipStream (NULL: the context's stream); it reads the scene image only and leaves
 * no trace in frame state. Refused without touching the device: a null context or pointer, a factor outside 1 .. 4, a pointer that
 * is not 16-byte aligned (PTSS_EINVAL); factor^2 * local pixels >= 2^31 (PTSS_ERANGE). */
int ptss_render_features_scaled(ptss_context* ctx, int factor, ptss_pixel_feature* dev_features_hi, void* hipStream);

/* factor 2, sigmaNormal 0.1, sigmaDepth 4 (the denoiser's tolerances: design choices, not measurements). */
int ptss_default_upsample_params(ptss_upsample_params* p);

/* Guided upsampling: an image of the context's size rebuilt at params->factor times that size, its edges taken
 * from the features of the larger frame, which are exact, and not from the noisy colour. dev_lo: any display-scale RGBA image of
 * the context's size — the frame's dev_pixels, or the output of ptss_denoise / ptss_denoise_history. dev_features_lo:
 * ptss_render_features (or _specular) of the same camera; dev_features_hi: ptss_render_features_scaled at params->factor. For every
 * hi-res pixel the four lo-res pixels around its centre are weighted bilinearly, and by material (a hard stop), normal and depth
 * against the hi-res pixel's own feature; the result is their normalised sum, clamped to the taps that counted. A hi-res pixel none
 * of whose taps counts (a surface the small frame did not see) takes the nearest lo-res pixel's colour, with weight 0.
 * dev_out_hi (factor^2 * width * height pixels, row 0 = bottom) receives (unsigned char)(v + 0.5f) per channel, alpha 255;
 * dev_out_hi_float (may be NULL) the floats before that conversion and, as weight, the sum of the taps' weights. factor = 1 copies
 * dev_lo with alpha 255. Asynchronous on hipStream (NULL: the context's stream); the caller orders it behind whatever wrote its
 * inputs. It reads its arguments only and leaves no trace in frame state. PTSS_EINVAL without touching the device and without
 * counting: a null context or required pointer, a wrong structSize, a factor outside 1 .. 4, a sigma that is not finite and
 * positive, a misaligned pointer (4 B for the pixels, 16 B for features and floats), dev_out_hi == dev_lo, a sharded context
 * (tileWorld > 1: a band of rows has no neighbours); PTSS_ERANGE likewise for factor^2 * pixels >= 2^31 or factor * height > 524,280 rows (the launch grid). The kernel owns no bit of ptss_launched_kernels, which this call leaves as
 * it is; ptss_upsample_launches counts its launches since ptss_create instead. */
int ptss_upsample(ptss_context* ctx, const ptss_uchar4* dev_lo, const ptss_pixel_feature* dev_features_lo,
                  const ptss_pixel_feature* dev_features_hi, const ptss_upsample_params* params, ptss_uchar4* dev_out_hi,
                  ptss_history_entry* dev_out_hi_float /* may be NULL */, void* hipStream);
int ptss_upsample_launches(const ptss_context* ctx, unsigned long long* out);

/* levels 5, sigmaColor 64, sigmaNormal 0.1, sigmaDepth 4 (the values behind the figures of DESIGN.md §3.17). */
int ptss_default_denoise_params(ptss_denoise_params* p);

/* Edge-avoiding A-trous filter of the accumulated image. Input: the context's integer accumulator (the bound one
 * if ptss_bind_accumulator was used) times the inverseTicks of the last frame's display value — the tone-mapped mean on the 0..255
 * scale —, then params->levels passes of the 5x5 B3-spline kernel at tap spacing 2^i, each tap weighted by material (a hard stop),
 * normal, depth and colour of dev_features (ptss_render_features of the same camera). Output: (unsigned char)(v + 0.5f) per channel,
 * alpha 255, into dev_out (local pixels; may be the frame's own dev_pixels). levels = 0 writes the frame's display pixels exactly.
 * The accumulator, the float sums, the RNG records and the counters are only read or not touched: frames rendered afterwards are
 * the frames rendered without it. Scratch (two colour planes of 16 B per pixel) is allocated by the first call with levels >= 2
 * and freed by ptss_destroy. Asynchronous on hipStream (NULL: the context's stream); the caller orders it behind the frames whose
 * accumulator it reads. The planes belong to the context: the denoise calls of ONE context (and ptss_read_denoise_plane) must be
 * ordered among themselves — the same stream, or an event or a synchronise between two streams. A wrong structSize, a null pointer or levels outside 0..6 return PTSS_EINVAL without touching the device; so does a
 * sharded context (tileWorld > 1): a band of rows has no neighbours to filter with. ptss_launched_kernels: PTSS_KERNEL_DENOISE. */
int ptss_denoise(ptss_context* ctx, const ptss_pixel_feature* dev_features, const ptss_denoise_params* params, ptss_uchar4* dev_out,
                 void* hipStream);

/* Device -> host copy (synchronising on the stream of that call) of the filtered floats the latest ptss_denoise of this context
 * left in its scratch: the colour plane its last NON-final pass wrote, i.e. the result of level levels - 2 (levels >= 2; the final
 * pass writes bytes only), 3 floats per local pixel on the 0..255 scale. count = 3 * local pixels; *level (may be NULL) receives
 * that level's index. PTSS_EINVAL when the latest call ran fewer than two levels (or there was none). With k + 1 levels it returns
 * what a k-level call converts to bytes: how the tests compare the device's floats with ptss_probe_denoise's. */
int ptss_read_denoise_plane(ptss_context* ctx, float* host_float3, size_t count, int* level);

/* cosNormal 0.9, depthTolerance 0.02, maxHistory 64, minCoverage 0.25 (design choices, not measurements). */
int ptss_default_reproject_params(ptss_reproject_params* p);

/* Reprojected history: carries an image across a camera move of a STATIC scene. For every pixel of the current
 * frame: its colour c (the context's accumulator times the inverseTicks of the last frame's display value, ptss_denoise's input) and
 * the samples per pixel n behind it (frames since the reset times samplesPerPass; 0 before the first frame); the world point its
 * centre ray hits (dev_features_now: ptss_render_features of the context's CURRENT camera) projected into prev_camera; the four
 * bilinear taps of dev_history_prev there, each counted only if the previous frame saw the same surface (same material, normals
 * within cosNormal, previous depth within depthTolerance of the point's distance from prev_camera — otherwise the point was hidden
 * then); out = the mean of c and the taps' colour h weighted n : w, w = the taps' weight capped at maxHistory (0 when the counting
 * taps cover less than minCoverage), weight = n + w. A pixel without usable history gets (c, n) exactly. dev_history_prev = NULL
 * means "no history": out = (c, n) for every pixel, prev_camera and dev_features_prev are ignored (and may be NULL). Moving geometry
 * is out of scope HERE: after ptss_set_scene pass NULL; after ptss_update_triangles pass NULL or use ptss_reproject_motion.
 * dev_history_out (one entry per pixel, 16-byte aligned) must not be dev_history_prev. Asynchronous on hipStream (NULL: the
 * context's stream); like ptss_denoise it only reads the accumulator and leaves no trace in frame state. PTSS_EINVAL without
 * touching the device: a null context or required pointer, a wrong structSize, cosNormal outside [-1, 1], depthTolerance or
 * maxHistory negative or not finite, minCoverage outside [0, 1], equal history pointers, a sharded context (tileWorld > 1).
 * ptss_launched_kernels: PTSS_KERNEL_REPROJECT. */
int ptss_reproject(ptss_context* ctx, const ptss_pixel_feature* dev_features_now, const ptss_camera* prev_camera,
                   const ptss_pixel_feature* dev_features_prev, const ptss_history_entry* dev_history_prev,
                   const ptss_reproject_params* params, ptss_history_entry* dev_history_out, void* hipStream);

/* ptss_reproject across a pose change of the triangles: everything as above, except that the world point of a
 * pixel whose centre ray hits is dev_motion_now[p].prevPoint (ptss_render_features_motion of the CURRENT camera and pose) — where
 * that surface point was when dev_history_prev was made — instead of the hit point itself: v = prevPoint - prev_camera's position,
 * r = |v|. Misses, every tap test (material, normal, depth against r, finite history, coverage), the clamp, the weights, the
 * argument checks and the dev_history_prev = NULL shortcut are ptss_reproject's; dev_motion_now (16-byte aligned) is required.
 * With motion rows of count = 0 the result is ptss_reproject's, bit for bit.
 * A limit: the normal test compares the CURRENT normal with the previous frame's normal at the tap, so a surface that turns by
 * more than acos(cosNormal) between two frames loses its history — the safe direction. Lighting that changed because geometry
 * moved is carried over as it was; maxHistory bounds how long that lag lasts. ptss_launched_kernels: PTSS_KERNEL_REPROJECT_MOTION. */
int ptss_reproject_motion(ptss_context* ctx, const ptss_pixel_feature* dev_features_now, const ptss_pixel_motion* dev_motion_now,
                          const ptss_camera* prev_camera, const ptss_pixel_feature* dev_features_prev,
                          const ptss_history_entry* dev_history_prev, const ptss_reproject_params* params,
                          ptss_history_entry* dev_history_out, void* hipStream);

/* ptss_denoise with the colours of dev_history (a ptss_reproject output) as input instead of the accumulator: the same passes, the
 * same kernels, the same scratch and ordering rules; levels = 0 converts the history's colours to bytes. It updates what
 * ptss_read_denoise_plane returns. */
int ptss_denoise_history(ptss_context* ctx, const ptss_history_entry* dev_history, const ptss_pixel_feature* dev_features,
                         const ptss_denoise_params* params, ptss_uchar4* dev_out, void* hipStream);

/* Leaves of the triangle hierarchy of the scene image in use (16 triangles each), 0 when that image walks
 * every triangle. */
int ptss_triangle_leaves(const ptss_context* ctx, int* out);

/* ---- Updating the scene of a live context ----
 * ptss_set_scene: replaces the WHOLE scene (host path). The scene is validated and its new image(s) are packed and uploaded
 * before the old ones are freed: on any error, allocation failure included, the context keeps its old scene untouched. The image
 * kind may change (plain / edge-classed, mesh, many-sphere) in either direction. The call waits for the work this context has
 * enqueued on its stream and on its lanes, then sets the reset flag and marks the camera rows stale. Pools, random streams,
 * camera, mode, maxIterations, cumulative counters (ptss_total_ray_bounces, ptss_launched_kernels, ptss_update_rejected), a bound
 * accumulator and the denoise planes are kept: afterwards the context behaves as a fresh ptss_create(scene, cfg) would, except
 * for the state of its random streams (ptss_reseed) and those counters. Scene arrays are copied, as by ptss_create. */
int ptss_set_scene(ptss_context* ctx, const ptss_scene_desc* scene);

/* ptss_update_triangles: new vertex data that is ALREADY ON THE DEVICE (device path, no host round trip). dev_triangles: DEVICE
 * pointer to `count` records in the caller's 76-byte layout; they replace the vertices and normals of the triangles with original
 * indices first .. first + count - 1. materialIdx of the records is ignored: the number of triangles, their materials and their
 * stored order do not change. A mesh image has every leaf and group bound refitted around the new vertices, exactly as
 * conservatively as a freshly packed image's (csrc/ptmesh.h), but keeps the kd order of the pose the scene was packed in: a
 * strongly deformed mesh culls worse and renders the same image; ptss_set_scene rebuilds the order. A context with two images
 * (many spheres) has both updated. Asynchronous on hipStream (NULL: the context's stream, i.e. behind the frames already
 * enqueued); the caller orders the call against frames and queries that read the scene, under the rules of ptss_denoise. The host
 * side of the call marks the camera rows stale and requests a reset.
 * A record with a vertex that is not finite or lies beyond |coordinate| <= 2^40 is NOT written — the triangle keeps its old
 * geometry — and a device counter grows (ptss_update_rejected): the image never leaves the range its kernels were proven for.
 * Normals are copied as given, whatever their bits.
 * Refused without touching the device: a null context or a null pointer with count > 0 (PTSS_EINVAL); a range that leaves
 * [0, numTriangles) (PTSS_ERANGE); an edge-classed image (T <= 255: PTSS_EINVAL — its storage order depends on the edges; use
 * ptss_set_scene). count = 0 returns PTSS_OK. ptss_launched_kernels: PTSS_KERNEL_UPDATE (the update), PTSS_KERNEL_REFIT (the refit, mesh images only). */
int ptss_update_triangles(ptss_context* ctx, const ptss_triangle* dev_triangles, size_t first, size_t count, void* hipStream);
/* Records ptss_update_triangles has refused since ptss_create (synchronises on the stream of the latest update). */
int ptss_update_rejected(ptss_context* ctx, unsigned long long* out);

/* ptss_resort_triangles: the kd order of a live mesh image rebuilt ON THE DEVICE from the vertices the image holds now (DESIGN.md
 * §3.23) — the other half of an animation loop: ptss_update_triangles refits the bounds but keeps the order of the pose the scene
 * was packed in. Afterwards every leaf (16 consecutive stored positions) holds the triangles a fresh pack of the current pose would
 * put there (csrc/ptorder.h restates the packer's rule level by level; ptss_probe_kd_order is the same code on the host), a
 * triangle's material and original index travel with it, the area lights name their triangles' new positions, and every bound is
 * refitted. A triangle whose record ptss_update_triangles refused is sorted by the vertices it kept. The image keeps its address
 * and layout; images render the same, only the culling changes. No host round trip and no wait: asynchronous on hipStream (NULL: the
 * context's stream); the caller orders it against frames, queries and feature passes that read the scene, under the rules of
 * ptss_update_triangles — in an animation loop it sits behind the update and before the next frame. The host side marks the camera
 * rows stale; it requests NO reset (the scene is the same scene: accumulation continues) and ptss_read_triangle_bounds /
 * ptss_read_triangle_positions synchronise with its stream.
 * Scratch: about 178 bytes per triangle (8 gathered rows 128, two 8-byte key arrays, segment 8, centroid codes 12, three index arrays
 * 12, extents 1.5) plus the radix sort's temporary, one device allocation made by the first call that launches, replaced if
 * ptss_set_scene brings another number of triangles, freed by ptss_destroy. It is allocated before anything is launched: PTSS_ENOMEM leaves the
 * image untouched. Every call of a context works in that one scratch: two calls on different streams are ordered against each
 * other by the caller as well.
 * Measured on one MI355X: 0.49 / 1.1 / 4.7 ms at 5,134 / 81,934 / 1,046,542 triangles, against 1.2 / 21 / 514 ms for
 * ptss_set_scene of the same pose — below it at every size measured, so no crossover is known down to 5,134 triangles.
 * Images without a kd order — plain, edge-classed, many-sphere, and every image of an everySphereLoop context: PTSS_OK, nothing
 * launched, nothing counted. A null context: PTSS_EINVAL. ptss_launched_kernels gains PTSS_KERNEL_REFIT (the refit that ran); the
 * sort's own kernels take no bit: ptss_resort_launches counts the calls that launched since ptss_create. */
int ptss_resort_triangles(ptss_context* ctx, void* hipStream);
int ptss_resort_launches(const ptss_context* ctx, unsigned long long* out);

/* Re-runs the random-stream set-up (curandSetupKernel, CudaTracer.cu:22-29) with `seed` and requests a reset: afterwards the
 * streams are those of a context created with cfg.seed = seed, so frame N of an animation need not depend on what was rendered
 * before it. Waits for the context's outstanding frames first; returns once the streams are seeded. */
int ptss_reseed(ptss_context* ctx, unsigned long long seed);

/* Device -> host copies (synchronising) of the mesh image in use, for tests and tools; PTSS_EINVAL when that image is not a mesh
 * image. Bounds: 12 floats each (csrc/ptmesh.h), the leaves first, then the groups; count = 12 * (leaves + groups), leaves =
 * ptss_triangle_leaves, groups = ceil(leaves / 16). Positions: the stored position of each original triangle index; count =
 * the scene's triangle count. */
int ptss_read_triangle_bounds(ptss_context* ctx, float* host, size_t count);
int ptss_read_triangle_positions(ptss_context* ctx, int* host, size_t count);

/* Diagnostic builds only (-DPTSS_DIAG=<bits>, csrc/ptss_diag.h, tools/build_variants.py): the eight counter words of that
 * build (sphere candidates per lane, scatter blocks, chunk culling, shadow-segment pairs, queue lengths); all zero in the
 * shipped library, which carries no counter. */
int ptss_debug_counters(ptss_context* ctx, unsigned long long* out8);

const char* ptss_error_string(int code);
const char* ptss_last_error_detail(void);
int ptss_version(void);

#ifdef __cplusplus
}
#endif
#endif
