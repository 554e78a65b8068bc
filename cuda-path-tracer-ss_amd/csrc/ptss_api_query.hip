// ptss_api_query.hip — the queries along caller-supplied rays and the first-hit feature renders: ptss_intersect, ptss_occluded,
// ptss_intersect_chain, the path queries (ptss_seed_path_rng .. ptss_path_launches), ptss_ray_features and ptss_render_features*.
// They run on the caller's stream and touch no frame state: of the context they read the device number, the default stream,
// images[0] (exact for every ray, so the camera's range plays no part), gridCap, numCUs and the default colour — the feature renders
// the current camera and tile map as well — and write only their own counters and scratch (ptss_context.h, second block) and, where
// the launch is one the frames count too, the context's kernel count.
#include <vector>

#include "ptss_context.h"
#include "ptspecular.h"
#include "ptlinrp.h"
#include "ptupsample.h"

extern "C" {

static int rayQuery(ptss_context* c, bool any, const ptss_ray_query* rays, void* out, size_t n, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (n == 0) return PTSS_OK;
    if (!rays || !out) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (((uintptr_t)rays | (uintptr_t)out) & (any ? 3u : 15u) || (uintptr_t)rays & 15u)
        return fail(PTSS_EINVAL, "rays and hits must be 16-byte aligned, verdicts 4-byte aligned");
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchQuery(st, any, im->dBlob, im->layout, im->inLds, rays, out, (uint32_t)n, c->gridCap * ptss::kShards,
                              &c->launchedKernels));
    return PTSS_OK;
}

int ptss_intersect(ptss_context* c, const ptss_ray_query* dev_rays, ptss_ray_hit* dev_hits, size_t n, void* hipStream) {
    return rayQuery(c, false, dev_rays, dev_hits, n, hipStream);
}

int ptss_occluded(ptss_context* c, const ptss_ray_query* dev_rays, uint32_t* dev_occluded, size_t n, void* hipStream) {
    return rayQuery(c, true, dev_rays, dev_occluded, n, hipStream);
}

// ptss_render_features: the context's CURRENT camera
int ptss_render_features(ptss_context* c, ptss_pixel_feature* dev_features, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features) return fail(PTSS_EINVAL, "dev_features is null");
    if ((uintptr_t)dev_features & 15u) return fail(PTSS_EINVAL, "dev_features must be 16-byte aligned");
    if (c->numPixels == 0) return PTSS_OK;   // a rank whose tile is empty
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchFeatures(st, im->dBlob, im->layout, im->inLds, c->tile, eyeParams(c), defaultColorOf(c), dev_features, c->numPixels,
                                 c->gridCap * ptss::kShards, &c->launchedKernels));
    return PTSS_OK;
}

// ptss_render_features_motion: the same launch shape; the previous records are the caller's, read in place
int ptss_render_features_motion(ptss_context* c, const ptss_triangle* dev_triangles_prev, size_t first, size_t count,
                                ptss_pixel_feature* dev_features, ptss_pixel_motion* dev_motion, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features || !dev_motion) return fail(PTSS_EINVAL, "dev_features or dev_motion is null");
    if (count > 0 && !dev_triangles_prev) return fail(PTSS_EINVAL, "dev_triangles_prev is null with count > 0");
    if (((uintptr_t)dev_features | (uintptr_t)dev_motion) & 15u) return fail(PTSS_EINVAL, "dev_features and dev_motion must be 16-byte aligned");
    if ((uintptr_t)dev_triangles_prev & 3u) return fail(PTSS_EINVAL, "dev_triangles_prev must be 4-byte aligned");
    if (count > 0) {
        const size_t T = (size_t)c->images[0].layout.numTriangles;
        if (first >= T || count > T - first) return fail(PTSS_ERANGE, "first .. first + count - 1 leaves the scene's triangles");
    }
    if (c->numPixels == 0) return PTSS_OK;   // a rank whose tile is empty
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchFeaturesMotion(st, im->dBlob, im->layout, im->inLds, c->tile, eyeParams(c), defaultColorOf(c), dev_features, c->numPixels,
                                       c->gridCap * ptss::kShards, dev_triangles_prev, count ? (uint32_t)first : 0u, (uint32_t)count, dev_motion,
                                       &c->launchedKernels));
    return PTSS_OK;
}

// ptss_render_features_specular: ptss_render_features' image, camera and grid; the chain of csrc/ptspecular.h behind the first hit
int ptss_render_features_specular(ptss_context* c, int maxSteps, ptss_pixel_feature* dev_features, uint32_t* dev_steps, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features) return fail(PTSS_EINVAL, "dev_features is null");
    if (maxSteps < 0 || maxSteps > ptsp::kMaxSteps) return fail(PTSS_EINVAL, "maxSteps must be in [0, 8]");
    if (((uintptr_t)dev_features & 15u) || ((uintptr_t)dev_steps & 3u))
        return fail(PTSS_EINVAL, "dev_features must be 16-byte aligned, dev_steps 4-byte aligned");
    if (c->numPixels == 0) return PTSS_OK;   // a rank whose tile is empty
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchFeaturesSpecular(st, im->dBlob, im->layout, im->inLds, c->tile, eyeParams(c), defaultColorOf(c), dev_features, dev_steps,
                                         c->numPixels, maxSteps, c->gridCap * ptss::kShards, c->specularFeatureLaunches));
    return PTSS_OK;
}

int ptss_specular_feature_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::specularFeatureLaunches, out2); }

// ptss_intersect_chain: the chain of csrc/ptspecular.h behind every hit (ptss_chain.hip)
int ptss_default_chain_options(ptss_chain_options* o) {
    if (!o) return fail(PTSS_EINVAL, "options is null");
    o->structSize = (unsigned int)sizeof(ptss_chain_options);
    o->schedule = PTSS_CHAIN_LANE_PER_RAY;
    o->maxWorkgroups = 0;
    o->reserved = 0;
    return PTSS_OK;
}

int ptss_intersect_chain(ptss_context* c, const ptss_ray_query* dev_rays, size_t n, int maxSteps, const ptss_chain_options* options,
                         ptss_ray_hit* dev_hits, ptss_chain_result* dev_chain, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (options) {
        if (options->structSize != sizeof(ptss_chain_options)) return fail(PTSS_EINVAL, "options->structSize is not sizeof(ptss_chain_options)");
        if (options->schedule != PTSS_CHAIN_LANE_PER_RAY && options->schedule != PTSS_CHAIN_REFILL) return fail(PTSS_EINVAL, "unknown schedule");
        if (options->maxWorkgroups < 0) return fail(PTSS_EINVAL, "maxWorkgroups must not be negative");
        if (options->reserved != 0) return fail(PTSS_EINVAL, "reserved must be 0");
    }
    if (maxSteps < 0 || maxSteps > ptsp::kMaxSteps) return fail(PTSS_ERANGE, "maxSteps must be in [0, 8]");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (!dev_rays || !dev_hits) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if (((uintptr_t)dev_rays | (uintptr_t)dev_hits | (uintptr_t)dev_chain) & 15u) return fail(PTSS_EINVAL, "rays, hits and chain must be 16-byte aligned");
    if (ptlrp::rangesOverlap(dev_hits, 48 * n, dev_rays, 32 * n)) return fail(PTSS_EINVAL, "dev_hits overlaps dev_rays");
    if (dev_chain && (ptlrp::rangesOverlap(dev_chain, 32 * n, dev_rays, 32 * n) || ptlrp::rangesOverlap(dev_chain, 32 * n, dev_hits, 48 * n)))
        return fail(PTSS_EINVAL, "dev_chain overlaps dev_rays or dev_hits");
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    if (!(options && options->schedule == PTSS_CHAIN_REFILL)) {
        HIP_TRY(ptss::launchChain(st, im->dBlob, im->layout, im->inLds, dev_rays, dev_hits, dev_chain, (uint32_t)n, maxSteps, c->gridCap * ptss::kShards,
                                  &c->chainLaunches[0]));
        return PTSS_OK;
    }
    if (!c->dChainHead) HIP_TRY(hipMalloc(&c->dChainHead, 2 * sizeof(uint32_t)));   // (set in front of every kernel: nothing to clear)
    HIP_TRY(ptss::launchChainRefill(st, im->dBlob, im->layout, im->inLds, dev_rays, dev_hits, dev_chain, (uint32_t)n, maxSteps, options->maxWorkgroups,
                                    c->numCUs, c->dChainHead, &c->chainLaunches[1]));
    return PTSS_OK;
}

int ptss_chain_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::chainLaunches, out2); }

// ptss_seed_path_rng: the streams of a path query, seeded as the context's own are (seedStreams). The jump table stays on the device
// from the first call on, so that later calls are asynchronous.
int ptss_seed_path_rng(ptss_context* c, ptss_path_rng* dev_rng, size_t n, unsigned long long seed, unsigned long long firstSequence,
                       unsigned int skip, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (skip > 64u) return fail(PTSS_EINVAL, "skip must be in [0, 64]");
    if (n == 0) return PTSS_OK;
    if (!dev_rng) return fail(PTSS_EINVAL, "dev_rng is null with n > 0");
    if ((uintptr_t)dev_rng & 3u) return fail(PTSS_EINVAL, "dev_rng must be 4-byte aligned");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (firstSequence > (1ull << 32) || firstSequence + n > (1ull << 32)) return fail(PTSS_ERANGE, "firstSequence + n must not exceed 2^32");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (!c->dPathJumpTable) {
        std::vector<uint32_t> table(ptrng::kJumpTableWords);
        ptrng::build_subsequence_table(table.data());
        uint32_t* dTable = nullptr;
        HIP_TRY(hipMalloc(&dTable, table.size() * sizeof(uint32_t)));
        const hipError_t e = hipMemcpy(dTable, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(dTable);
            return fail(PTSS_EHIP, "upload of the jump table", e);
        }
        c->dPathJumpTable = dTable;
    }
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchPathRngSeed(st, dev_rng, (uint32_t)n, seed, (uint32_t)firstSequence, skip, c->dPathJumpTable));
    return PTSS_OK;
}

// ptss_trace_paths / ptss_trace_paths_opt, with the scene's guard flags and default colour. options == nullptr: ptss_trace_paths itself
static int tracePaths(ptss_context* c, const ptss_ray_query* dev_rays, ptss_path_rng* dev_rng, ptss_path_result* dev_results, size_t n,
                      unsigned int maxIterations, const ptss_path_options* options, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (maxIterations < 1u || maxIterations > (unsigned)ptss::kMaxBounces) return fail(PTSS_EINVAL, "maxIterations must be in [1, 64]");
    const bool refill = options && options->schedule == PTSS_PATHS_REFILL;
    if (n == 0) return PTSS_OK;
    if (!dev_rays || !dev_rng || !dev_results) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if ((((uintptr_t)dev_rays | (uintptr_t)dev_results) & 15u) || ((uintptr_t)dev_rng & 3u))
        return fail(PTSS_EINVAL, "rays and results must be 16-byte aligned, dev_rng 4-byte aligned");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    if (!refill) {
        HIP_TRY(ptss::launchPathQuery(st, im->dBlob, im->layout, im->inLds, dev_rays, dev_rng, dev_results, (uint32_t)n, (int)maxIterations, defaultColorOf(c),
                                      im->guardFlags, c->gridCap * ptss::kShards, c->pathLaunches));
        return PTSS_OK;
    }
    if (!c->dPathRefill) {   // the head and the counters: zero from here on, in stream order with this and every later refill call
        unsigned long long* d = nullptr;
        HIP_TRY(hipMalloc(&d, ptss::kPathRefillWords * sizeof(unsigned long long)));
        const hipError_t e = hipMemsetAsync(d, 0, ptss::kPathRefillWords * sizeof(unsigned long long), st);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(PTSS_EHIP, "clearing the refill counters", e);
        }
        c->dPathRefill = d;
    }
    c->lastRefill.note(st);
    HIP_TRY(ptss::launchPathRefill(st, im->dBlob, im->layout, im->inLds, dev_rays, dev_rng, dev_results, (uint32_t)n, (int)maxIterations, defaultColorOf(c),
                                   im->guardFlags, options->maxWorkgroups, c->numCUs, c->dPathRefill, c->refillLaunches));
    return PTSS_OK;
}

int ptss_trace_paths(ptss_context* c, const ptss_ray_query* dev_rays, ptss_path_rng* dev_rng, ptss_path_result* dev_results, size_t n,
                     unsigned int maxIterations, void* hipStream) {
    return tracePaths(c, dev_rays, dev_rng, dev_results, n, maxIterations, nullptr, hipStream);
}

int ptss_default_path_options(ptss_path_options* o) {
    if (!o) return fail(PTSS_EINVAL, "options is null");
    o->structSize = (unsigned int)sizeof(ptss_path_options);
    o->schedule = PTSS_PATHS_LANE_PER_RAY;
    o->maxWorkgroups = 0;
    o->reserved = 0;
    return PTSS_OK;
}

int ptss_trace_paths_opt(ptss_context* c, const ptss_ray_query* dev_rays, ptss_path_rng* dev_rng, ptss_path_result* dev_results, size_t n,
                         unsigned int maxIterations, const ptss_path_options* options, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!options) return fail(PTSS_EINVAL, "options is null");
    if (options->structSize != sizeof(ptss_path_options)) return fail(PTSS_EINVAL, "options->structSize is not sizeof(ptss_path_options)");
    if (options->schedule != PTSS_PATHS_LANE_PER_RAY && options->schedule != PTSS_PATHS_REFILL) return fail(PTSS_EINVAL, "unknown schedule");
    if (options->maxWorkgroups < 0) return fail(PTSS_EINVAL, "maxWorkgroups must not be negative");
    if (options->reserved != 0) return fail(PTSS_EINVAL, "reserved must be 0");
    return tracePaths(c, dev_rays, dev_rng, dev_results, n, maxIterations, options, hipStream);
}

// [0], [1]: host counts; [2..4]: the device counters, behind everything the latest refill call's stream holds
int ptss_path_refill_stats(ptss_context* c, unsigned long long* out5) {
    RC_TRY(readLaunches(c, &ptss_context::refillLaunches, out5));
    out5[2] = out5[3] = out5[4] = 0;
    return c->dPathRefill ? readBehind(c, c->lastRefill, c->dPathRefill + 1, 3, out5 + 2) : PTSS_OK;
}

int ptss_path_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::pathLaunches, out2); }

int ptss_ray_features(ptss_context* c, const ptss_ray_query* dev_rays, ptss_pixel_feature* dev_features, size_t n, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (n == 0) return PTSS_OK;
    if (!dev_rays || !dev_features) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if (((uintptr_t)dev_rays | (uintptr_t)dev_features) & 15u) return fail(PTSS_EINVAL, "rays and features must be 16-byte aligned");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchRayFeatures(st, im->dBlob, im->layout, im->inLds, dev_rays, defaultColorOf(c), dev_features, (uint32_t)n, c->gridCap * ptss::kShards,
                                    &c->filmLaunches[2]));
    return PTSS_OK;
}

// ptss_render_features_scaled: ptss_render_features' launch for the frame of factor * width x factor * height — the tile map and the eye
// constants a context of that size would hold (ptss_create, eyeParams), so the entries are that context's, byte for byte
int ptss_render_features_scaled(ptss_context* c, int factor, ptss_pixel_feature* dev_features_hi, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features_hi) return fail(PTSS_EINVAL, "dev_features_hi is null");
    if (factor < 1 || factor > ptup::kMaxFactor) return fail(PTSS_EINVAL, "factor must be in [1, 4]");
    if ((uintptr_t)dev_features_hi & 15u) return fail(PTSS_EINVAL, "dev_features_hi must be 16-byte aligned");
    const unsigned long long n = (unsigned long long)(factor * factor) * c->numPixels;
    if (!fits31(n)) return fail(PTSS_ERANGE, "factor^2 * local pixels must stay below 2^31");
    if (n == 0) return PTSS_OK;   // a rank whose tile is empty
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const int fW = factor * c->tile.width, fH = factor * c->tile.height;
    const ptss::TileMap tile{fW, fH, factor * c->tile.localRows, c->tile.rank, c->tile.world, factor * c->tile.bandRows};
    const ptss::EyeParams eye{c->camera, -2 * ptm::tan(c->camera.fieldOfView * 0.5f), (float)fH / (float)fW, 1.0f / fW, 1.0f / fH};
    HIP_TRY(ptss::launchFeatures(st, im->dBlob, im->layout, im->inLds, tile, eye, defaultColorOf(c), dev_features_hi, (uint32_t)n,
                                 c->gridCap * ptss::kShards, &c->launchedKernels));
    return PTSS_OK;
}

}  // extern "C"
