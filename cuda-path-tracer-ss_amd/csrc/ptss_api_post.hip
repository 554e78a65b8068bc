// ptss_api_post.hip — the display-referred passes: ptss_denoise, ptss_denoise_history, ptss_upsample, ptss_reproject,
// ptss_reproject_motion and ptss_read_denoise_plane, with their defaults and getters. They run on the caller's stream and READ the
// context's own accumulator, camera, tile map and tick counts; what they write is their own (ptss_context.h, second block) and the
// context's kernel count.
#include <string>
#include <vector>

#include "ptss_context.h"
#include "ptupsample.h"
#include "ptreproject.h"

extern "C" {

int ptss_default_upsample_params(ptss_upsample_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(*p);
    p->factor = 2;
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.0f;
    return PTSS_OK;
}

// ptss_upsample: one launch over the hi-res frame; it reads its arguments only
int ptss_upsample(ptss_context* c, const ptss_uchar4* dev_lo, const ptss_pixel_feature* dev_features_lo, const ptss_pixel_feature* dev_features_hi,
                  const ptss_upsample_params* params, ptss_uchar4* dev_out_hi, ptss_history_entry* dev_out_hi_float, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_lo || !dev_features_lo || !dev_features_hi || !dev_out_hi) return fail(PTSS_EINVAL, "null argument");
    if (const char* why = ptup::paramsError(params)) return fail(PTSS_EINVAL, why);
    if (((uintptr_t)dev_lo | (uintptr_t)dev_out_hi) & 3u) return fail(PTSS_EINVAL, "dev_lo and dev_out_hi must be 4-byte aligned");
    if (((uintptr_t)dev_features_lo | (uintptr_t)dev_features_hi | (uintptr_t)dev_out_hi_float) & 15u)
        return fail(PTSS_EINVAL, "features and dev_out_hi_float must be 16-byte aligned");
    if (static_cast<const void*>(dev_out_hi) == static_cast<const void*>(dev_lo))
        return fail(PTSS_EINVAL, "dev_out_hi must not be dev_lo: a pixel's taps are other pixels' inputs");
    if (c->tile.world > 1)
        return fail(PTSS_EINVAL, "ptss_upsample needs the whole frame: this context is a pixel-band shard (tileWorld > 1), whose bands of rows "
                                 "have no neighbours to interpolate with");
    const int factor = params->factor;
    if (!fits31((unsigned long long)(factor * factor) * c->numPixels))
        return fail(PTSS_ERANGE, "factor^2 * pixels must stay below 2^31");
    if ((long long)factor * c->tile.height > ptup::kMaxHiRows) return fail(PTSS_ERANGE, "factor * height must not exceed 524,280 rows");
    if (c->numPixels == 0) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchUpsample(st, dev_lo, dev_features_lo, dev_features_hi, dev_out_hi, dev_out_hi_float, c->tile.width, c->tile.height, factor,
                                 ptup::levelOf(*params), &c->upsampleLaunches));
    return PTSS_OK;
}

int ptss_upsample_launches(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::upsampleLaunches, out); }

int ptss_default_denoise_params(ptss_denoise_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(*p);
    p->levels = 5;
    p->sigmaColor = 64.0f;
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.0f;
    return PTSS_OK;
}

// ptss_denoise / ptss_denoise_history: the passes over the context's integer accumulator (fromAccumulator) or over `input`, a plane of
// float4 colours
static int denoisePasses(ptss_context* c, const char* what, const void* input, bool fromAccumulator, const ptss_pixel_feature* dev_features,
                         const ptss_denoise_params* params, ptss_uchar4* dev_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features || !params || !dev_out || (!fromAccumulator && !input)) return fail(PTSS_EINVAL, "null argument");
    if (params->structSize != (unsigned int)sizeof(ptss_denoise_params))
        return fail(PTSS_EINVAL, "params->structSize is not this library's sizeof(ptss_denoise_params): start from ptss_default_denoise_params");
    if (params->levels < 0 || params->levels > PTSS_DENOISE_MAX_LEVELS) return fail(PTSS_EINVAL, "levels must be in [0, 6]");
    if (!(params->sigmaColor > 0.0f) || !(params->sigmaNormal > 0.0f) || !(params->sigmaDepth >= 0.0f))
        return fail(PTSS_EINVAL, "sigmaColor and sigmaNormal must be positive, sigmaDepth not negative");
    if (((uintptr_t)dev_features & 15u) || ((uintptr_t)dev_out & 3u)) return fail(PTSS_EINVAL, "dev_features must be 16-byte aligned, dev_out 4-byte aligned");
    if (!fromAccumulator && ((uintptr_t)input & 15u)) return fail(PTSS_EINVAL, "dev_history must be 16-byte aligned");
    if (c->tile.world > 1)
        return fail(PTSS_EINVAL, (std::string(what) + " needs the whole frame: this context is a pixel-band shard (tileWorld > 1), whose bands of "
                                                       "rows have no neighbours to filter with").c_str());
    if (fromAccumulator) input = c->dAccum;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const int levels = params->levels;
    if (levels >= 2)
        for (float4*& plane : c->dDenoise)
            if (!plane) {
                RC_TRY(createCheck(hipMalloc(&plane, (size_t)c->numPixels * sizeof(float4)), "ptss_denoise: colour planes"));
            }
    // the display value's scale: displayKernel's / finishPath's inverseTicks of the last frame (frameBuffers)
    const float inverseTicks = 1.f / (float)((int)c->samples * (c->lastTicks - c->lastResetTick + 1));
    const int width = c->tile.width, height = c->tile.height;
    c->denoiseLastPlane = levels >= 2 ? (levels - 2) & 1 : -1;
    c->denoiseLastLevel = levels - 2;
    c->denoiseStream = st;
    for (int i = 0; i < (levels > 0 ? levels : 1); ++i) {
        const bool first = i == 0, last = i + 1 >= levels;
        const void* src = first ? input : c->dDenoise[(i - 1) & 1];
        void* dst = last ? static_cast<void*>(dev_out) : c->dDenoise[i & 1];
        HIP_TRY(ptss::launchDenoise(st, first && fromAccumulator, last, src, dst, dev_features, width, height, ptdn::levelOf(*params, i), inverseTicks,
                                    &c->launchedKernels));
    }
    return PTSS_OK;
}

int ptss_denoise(ptss_context* c, const ptss_pixel_feature* dev_features, const ptss_denoise_params* params, ptss_uchar4* dev_out,
                 void* hipStream) {
    return denoisePasses(c, "ptss_denoise", nullptr, true, dev_features, params, dev_out, hipStream);
}

// the same passes over the colours of a history: an entry is laid out as a colour-plane entry, so every pass is a denoiseKernel<false, *>
int ptss_denoise_history(ptss_context* c, const ptss_history_entry* dev_history, const ptss_pixel_feature* dev_features,
                         const ptss_denoise_params* params, ptss_uchar4* dev_out, void* hipStream) {
    return denoisePasses(c, "ptss_denoise_history", dev_history, false, dev_features, params, dev_out, hipStream);
}

int ptss_default_reproject_params(ptss_reproject_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(*p);
    p->cosNormal = 0.9f;
    p->depthTolerance = 0.02f;
    p->maxHistory = 64.0f;
    p->minCoverage = 0.25f;
    return PTSS_OK;
}

// ptss_reproject / ptss_reproject_motion: one set of checks, one launch; motion: the point of a hit comes from dev_motion_now
static int reprojectCall(ptss_context* c, const char* what, bool motion, const ptss_pixel_feature* dev_features_now,
                         const ptss_pixel_motion* dev_motion_now, const ptss_camera* prev_camera, const ptss_pixel_feature* dev_features_prev,
                         const ptss_history_entry* dev_history_prev, const ptss_reproject_params* params, ptss_history_entry* dev_history_out,
                         void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features_now || !dev_history_out || (motion && !dev_motion_now)) return fail(PTSS_EINVAL, "null argument");
    if (dev_history_prev && (!prev_camera || !dev_features_prev)) return fail(PTSS_EINVAL, "a history needs its camera and its features");
    if (const char* why = ptrp::paramsError(params)) return fail(PTSS_EINVAL, why);
    if (static_cast<const void*>(dev_history_out) == static_cast<const void*>(dev_history_prev))
        return fail(PTSS_EINVAL, "dev_history_out must not be dev_history_prev: a pixel's taps are other pixels' entries");
    if (((uintptr_t)dev_features_now | (uintptr_t)dev_features_prev | (uintptr_t)dev_history_prev | (uintptr_t)dev_history_out |
         (uintptr_t)dev_motion_now) & 15u)
        return fail(PTSS_EINVAL, "features, motion rows and histories must be 16-byte aligned");
    if (c->tile.world > 1)
        return fail(PTSS_EINVAL, (std::string(what) + " needs the whole frame: this context is a pixel-band shard (tileWorld > 1)").c_str());
    if (c->numPixels == 0) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    // c and n of the accumulator as it stands: the last frame's display scale (ptss_denoise's input), nothing before the first frame
    const int perPixel = (int)c->samples * (c->lastTicks - c->lastResetTick + 1);
    const float inverseTicks = 1.f / (float)perPixel;
    const float n = c->frameIndex == 0 ? 0.0f : (float)perPixel;
    const int width = c->tile.width, height = c->tile.height;
    const ptrp::View now = ptrp::viewOf(c->camera, width, height);
    const ptrp::View prev = dev_history_prev ? ptrp::viewOf(*prev_camera, width, height) : now;
    if (motion)
        HIP_TRY(ptss::launchReprojectMotion(st, c->dAccum, dev_features_now, dev_motion_now, dev_features_prev, dev_history_prev, dev_history_out,
                                            width, height, now, prev, ptrp::paramsOf(*params), inverseTicks, n, &c->launchedKernels));
    else
        HIP_TRY(ptss::launchReproject(st, c->dAccum, dev_features_now, dev_features_prev, dev_history_prev, dev_history_out, width, height, now, prev,
                                      ptrp::paramsOf(*params), inverseTicks, n, &c->launchedKernels));
    return PTSS_OK;
}

int ptss_reproject(ptss_context* c, const ptss_pixel_feature* dev_features_now, const ptss_camera* prev_camera,
                   const ptss_pixel_feature* dev_features_prev, const ptss_history_entry* dev_history_prev,
                   const ptss_reproject_params* params, ptss_history_entry* dev_history_out, void* hipStream) {
    return reprojectCall(c, "ptss_reproject", false, dev_features_now, nullptr, prev_camera, dev_features_prev, dev_history_prev, params,
                         dev_history_out, hipStream);
}

int ptss_reproject_motion(ptss_context* c, const ptss_pixel_feature* dev_features_now, const ptss_pixel_motion* dev_motion_now,
                          const ptss_camera* prev_camera, const ptss_pixel_feature* dev_features_prev,
                          const ptss_history_entry* dev_history_prev, const ptss_reproject_params* params,
                          ptss_history_entry* dev_history_out, void* hipStream) {
    return reprojectCall(c, "ptss_reproject_motion", true, dev_features_now, dev_motion_now, prev_camera, dev_features_prev, dev_history_prev,
                         params, dev_history_out, hipStream);
}

int ptss_read_denoise_plane(ptss_context* c, float* host_float3, size_t count, int* level) {
    if (!c || !host_float3) return fail(PTSS_EINVAL, "null argument");
    if (c->denoiseLastPlane < 0) return fail(PTSS_EINVAL, "no colour plane: the latest ptss_denoise of this context ran fewer than two levels");
    if (count != (size_t)3 * c->numPixels) return fail(PTSS_ERANGE, "count must be 3 * local pixels");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->denoiseStream));
    std::vector<float4> plane(c->numPixels);
    HIP_TRY(hipMemcpy(plane.data(), c->dDenoise[c->denoiseLastPlane], plane.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < plane.size(); ++p) {
        host_float3[3 * p] = plane[p].x;
        host_float3[3 * p + 1] = plane[p].y;
        host_float3[3 * p + 2] = plane[p].z;
    }
    if (level) *level = c->denoiseLastLevel;
    return PTSS_OK;
}

}  // extern "C"
