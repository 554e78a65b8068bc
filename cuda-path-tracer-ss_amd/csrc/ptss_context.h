// ptss_context.h — what the C-ABI translation units (ptss_api*.hip) share: the context behind include/ptss.h, how a call
// reports a refusal, and the few bodies more than one of those files states. Included by them only: no kernel file and
// nothing under host/ sees a ptss_context.
#pragma once
#include <string.h>

#include <utility>
#include <vector>

#include "ptss.h"
#include "ptss_device.h"

// The one function of the layer that crosses translation units: it writes the thread's text behind ptss_last_error_detail,
// which ptss_api.hip defines (hidden: the dynamic symbol table holds the ptss_* entry points only).
__attribute__((visibility("hidden"))) int fail(int code, const char* what, hipError_t e = hipSuccess);

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return fail(PTSS_EHIP, #expr, _e); \
    } while (0)

#define RC_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)   // a step that reports a PTSS_* code

// an allocation's failure: PTSS_ENOMEM when the device ran out of memory, PTSS_EHIP for any other HIP error
static inline int createCheck(hipError_t e, const char* what) {
    return e == hipSuccess ? PTSS_OK : fail(e == hipErrorOutOfMemory ? PTSS_ENOMEM : PTSS_EHIP, what, e);
}

struct __attribute__((visibility("hidden"))) EventPair {   // (hidden with what is instantiated over it: it was file-local before the layer had a header)
    hipEvent_t a, b;
};

// One ray population of the frame with its own pools, counters and stream (ptss_device.h, "frame lanes"). A context
// has 1..kMaxLanes of them; with one lane the caller's stream is used and nothing below differs from a single population.
struct Lane {
    hipStream_t stream = nullptr;            // own stream (contexts with several lanes only)
    float* dPool[2] = {nullptr, nullptr};
    uint32_t* dCounts[2] = {nullptr, nullptr};   // alternate per frame (flushKernel arms the other one)
    uint32_t* dShardCount0 = nullptr;
    uint32_t* dLastCounts = nullptr;         // counts of the frame before (flushKernel's copy)
    uint32_t* dDone = nullptr;               // done[countIndex(b, s)]: workgroups of shard s that ended a bounce-b kernel, all frames (never reset)
    uint32_t doneTarget[ptss::kMaxBounces + 1] = {};  // what done[b][*] add up to once everything launched so far has ended
                                             // (stored by this lane's bounce-b kernel as it starts: bounce b - 1 has then finished)
    hipEvent_t evDone[2] = {nullptr, nullptr};   // end of this lane's frame, by frame parity (several lanes only)
    uint32_t regionCap = 0;                  // slots per shard region of this lane's pools
    int maxBlocks = 0;                       // one 256-ray tile per workgroup over this lane's share of the frame
    // live-count hints: counts[] of a recent frame, read back asynchronously, size the next frames' grids
    uint32_t hint[ptss::kMaxBounces + 1] = {0};  // per bounce: the fullest shard's live count
    bool haveHint = false;
    uint32_t* hCounts = nullptr;  // pinned, 4 slots x kCountWords
    hipEvent_t hintEvent[4] = {nullptr, nullptr, nullptr, nullptr};
    bool hintPending[4] = {false, false, false, false};
};

// One packed scene (ptpack.h packScene) on the device, with how the frames use it.
struct SceneImage {
    float4* dBlob = nullptr;
    ptss::SceneLayout layout{};
    bool inLds = true;       // staged in LDS (true) or read through scalar loads (false)
    bool oneLaunch = false;  // the frame is traced by ONE launch (frameKernel)
    uint32_t guardFlags = 0; // range guards the scene's constants satisfy (ptpack.h sceneGuardFlags); the same for both images of a scene
};

// The words of ptss_context::dTotal, 64 bits each, zero from ptss_create on.
enum TotalWord : int {
    kLaneTotalsWord = 0,                            // kMaxLanes words: ray-bounce totals, one per lane
    kRejectedWord = ptss::kMaxLanes,                // records ptss_update_triangles rejected
    kFilmRejectedWord = ptss::kMaxLanes + 1,        // index entries the film calls dropped
    kSplatCountersWord = ptss::kMaxLanes + 2,       // two words: samples the splat calls dropped, samples they clamped
    kSurfaceRejectedWord = ptss::kMaxLanes + 4,     // entries ptss_generate_rays_surface dropped
                                                    // (+ 5 .. + 7: unused)
    kGuardTimeoutsWord = ptss::kMaxLanes + 8,       // its low 32 bits: guard timeouts (must stay 0; FrameBuffers::guardTimeouts)
    kTotalWords = ptss::kMaxLanes + 8 + 1
};

// The stream of the latest call that may have counted into a device word, for the read-back that has to wait for it (readBehind).
struct LastStream {
    hipStream_t stream = nullptr;
    bool set = false;
    void note(hipStream_t st) {
        stream = st;
        set = true;
    }
    hipError_t synchronize() const { return set ? hipStreamSynchronize(stream) : hipSuccess; }
};

struct ptss_context {
    // ---- frame state: what ptss_api.hip's driver, read-backs and scene updates work on. Of it, the calls on the caller's stream
    // (ptss_api_query.hip, ptss_api_film.hip) read only cfg.device, stream, images[0], gridCap, numCUs, defaultColor and dTotal ----
    ptss_render_config cfg{};
    hipStream_t stream = nullptr;
    ptss::TileMap tile{};
    // images[0]: the scene image the context was made for; images[1] (sphere acceleration on, else empty): the plain image,
    // for cameras outside the chunked image's range. The frames use images[active].
    SceneImage images[2];
    int active = 0;
    const SceneImage& image() const { return images[active]; }
    std::vector<Lane> lanes;
    hipEvent_t evFork = nullptr;            // several lanes: the caller's stream has reached this frame
    int countParity = 0;                    // which of a lane's two count buffers the next frame uses
    uint32_t* dRngHome = nullptr;
    unsigned long long* dTotal = nullptr;   // kTotalWords device counters (TotalWord)
    uint32_t* dAccumOwned = nullptr;
    uint32_t* dAccum = nullptr;  // owned or bound
    float* dFsum = nullptr;
    uint32_t* dStaged = nullptr;  // S > 1: per-stream sample words of the current pass. Free-running lanes: TWO buffers, by frame parity —
                                  // the lanes of frame N + 1 already park samples while displayKernel of frame N (on the caller's stream,
                                  // behind the join) still adds up frame N's; a lane starts frame N + 2 only behind displayKernel of frame N
    bool stagedTwice = false;
    hipEvent_t evDisplay[2] = {nullptr, nullptr};   // displayKernel of the last frame of each parity has run (stagedTwice only)
    uint32_t capacity = 0, numPixels = 0;  // capacity: stride of the per-pixel planes (rngHome)
    uint32_t samples = 1;                    // cfg.samplesPerPass (sample lanes per pixel)
    bool cameraDirty = true;           // primary-ray precomputes must be refreshed (camera-origin rows and strip words)
    unsigned long long* dStrips = nullptr;   // capacity / 64 strip words (csrc/ptstrip.h), rewritten together with the camera-origin rows
    bool stripsOn = false;                   // the current image and camera are ones bounce 0 culls on: dStrips holds their words
    bool stripsRead = false;                 // the latest frame's bounce 0 read them (ptss_read_strip_words)
    float defaultColor[3] = {0, 0, 0};
    // ProgramData (CudaTracer.h:32-42)
    ptss_camera camera{};
    int lastResetTick = 0, lastTicks = 0;
    unsigned maxIterations = 15;
    bool resetTicksThisFrame = true;
    bool usePathTracer = true;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    float lastMs = 0.0f;
    int gridCap = 0;             // workgroups per shard at most = 16 resident rounds of this scene's bounce kernel (0 = uncapped)
    int numCUs = 0;              // hipDeviceProp_t::multiProcessorCount of cfg.device (sceneState's launch caps)
    unsigned frameIndex = 0;
    // bounce-kernel timing (cfg.timeKernels): every launch is bracketed by two events on ITS stream; a finished pair becomes
    // an interval [start, end) in ms since evEpoch. ptss_bounce_kernel_time reports the UNION of the intervals: with one lane
    // that is the sum of the launch durations, with several lanes (whose kernels overlap in time) the time during which at
    // least one bounce kernel was running — the figure a launch-time roofline needs.
    std::vector<EventPair> evFree, evBusy;
    std::vector<std::pair<double, double>> kernelSpans;
    hipEvent_t evEpoch = nullptr;
    unsigned int timeoutsSeen = 0;   // ptss_guard_timeouts value already reported as PTSS_ETIMEOUT
    unsigned long long launchedKernels = 0;   // frame, ray-query, feature, display-pass and scene-update kernels enqueued since ptss_create
    LastStream lastUpdate;                    // the latest ptss_update_triangles or ptss_resort_triangles (read-backs of the image, kRejectedWord)
    ptss::ResortScratch resortScratch;        // ptss_resort_triangles' device scratch, allocated by its first launching call
    unsigned long long resortLaunches = 0;    // ptss_resort_triangles calls that launched

    // ---- what the calls outside the frame driver keep for themselves: launch counters (the ptss_*_launches getters), debug forms
    // (the ptss_debug_*_form setters), last streams, and device scratch allocated by the first call that needs it ----
    // ptss_api_query.hip
    unsigned long long specularFeatureLaunches[2] = {0, 0};   // ptss_render_features_specular launches: [0] in place, [1] in LDS
    unsigned long long chainLaunches[2] = {0, 0};             // ptss_intersect_chain launches: [0] one lane per ray, [1] refill
    uint32_t* dChainHead = nullptr;                           // the refill schedule's queue head (ptss_device.h launchChainRefill)
    unsigned long long pathLaunches[2] = {0, 0};              // ptss_trace_paths launches: [0] in place, [1] in LDS
    uint32_t* dPathJumpTable = nullptr;                       // ptss_seed_path_rng's 2^67 jump table
    unsigned long long refillLaunches[2] = {0, 0};            // ptss_trace_paths_opt launches with PTSS_PATHS_REFILL: [0] in place, [1] in LDS
    unsigned long long* dPathRefill = nullptr;                // their queue head and counters (ptss_device.h launchPathRefill)
    LastStream lastRefill;                                    // the latest of them (ptss_path_refill_stats)
    // ptss_api_film.hip
    unsigned long long filmLaunches[3] = {0, 0, 0};           // ptss_generate_rays, ptss_accumulate_paths, ptss_ray_features calls that launched
    LastStream lastFilmIndex;                                 // the latest film call with an index (kFilmRejectedWord)
    unsigned long long adaptiveLaunches[2] = {0, 0};          // ptss_accumulate_paths_stats, ptss_plan_samples calls that launched
    unsigned long long linearLaunches[2] = {0, 0};            // ptss_accumulate_paths_linear, ptss_resolve_linear calls that launched
    unsigned long long linStatsLaunches[2] = {0, 0};          // ptss_accumulate_paths_linear_stats, ptss_plan_samples_linear calls that launched
    unsigned long long splatLaunches[3] = {0, 0, 0};          // ptss_splat_paths, ptss_splat_paths_homed, ptss_resolve_splat calls that launched
    LastStream lastSplat;                                     // the latest splat (kSplatCountersWord)
    unsigned long long meterLaunches[3] = {0, 0, 0};          // meter histograms, ptss_meter_exposure, metered resolves that launched
    unsigned long long glareLaunches[3] = {0, 0, 0};          // glare builds, the kernels they launched, glare resolves that launched
    unsigned long long toneLaunches[2] = {0, 0};              // ptss_tone_build, ptss_resolve_toned calls that launched
    int toneForm = 0;                                         // 0 the shipped lookup, 1 staged in LDS, 2 guess and settle
    unsigned long long linDenoiseLaunches[2] = {0, 0};        // ptss_denoise_linear calls that launched, the kernels inside them
    int linDenoiseForm = 0;                                   // 0 the measured table, 1 unstaged, 2 staged, 4 + mask
    unsigned long long linReprojectLaunches = 0;              // ptss_reproject_linear calls that launched
    unsigned long long linUpsampleLaunches = 0;               // ptss_upsample_linear calls that launched
    int linUpsampleForm = 0;                                  // 0 the measured table, 1 global memory, 2 staged
    unsigned long long surfaceLaunches[2] = {0, 0};           // ptss_generate_rays_surface, ptss_dilate_linear calls that launched
    LastStream lastSurface;                                   // the latest ptss_generate_rays_surface (kSurfaceRejectedWord)
    int dilateForm = 0;                                       // 0 the shipped form, 1 global memory, 2 staged
    unsigned long long lightmapLaunches = 0;                  // ptss_lookup_lightmap calls that launched
    unsigned long long lightmapChainLaunches = 0;             // ptss_lookup_lightmap_chain calls that launched
    int lightmapForm = 0;                                     // 0 the shipped form, 1 one lane per hit, 2 four lanes per hit
    // ptss_api_post.hip
    unsigned long long upsampleLaunches = 0;    // ptss_upsample launches
    float4* dDenoise[2] = {nullptr, nullptr};   // ptss_denoise's ping-pong colour planes (levels >= 2)
    int denoiseLastPlane = -1;                  // the plane the last non-final pass of the latest ptss_denoise wrote (-1: none), and its
    int denoiseLastLevel = -1;                  // level; on denoiseStream (ptss_read_denoise_plane)
    hipStream_t denoiseStream = nullptr;
};

// the calls on the caller's stream: counts and indices travel as 32-bit words, and a null stream is the context's
static inline bool fits31(unsigned long long v) { return v < (1ull << 31); }
static inline hipStream_t streamOf(const ptss_context* c, void* hipStream) { return hipStream ? static_cast<hipStream_t>(hipStream) : c->stream; }

static inline const float* quantTableOf(const SceneImage& im) { return reinterpret_cast<const float*>(im.dBlob + im.layout.offQuant); }

// The image those calls read — images[0], exact for every ray, so the camera's range plays no part — or nullptr behind their refusal.
static inline const SceneImage* sceneImageOf(const ptss_context* c) {
    if (c->images[0].dBlob) return &c->images[0];
    fail(PTSS_EINVAL, "context has no scene image");
    return nullptr;
}

static inline ptss_vec3 defaultColorOf(const ptss_context* c) { return ptss_vec3{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]}; }

static inline ptss::EyeParams eyeParams(const ptss_context* c) {   // {camera, s (CudaTracer.cu:334), aspect, invW, invH}
    return {c->camera, -2 * ptm::tan(c->camera.fieldOfView * 0.5f), (float)c->tile.height / (float)c->tile.width, 1.0f / c->tile.width,
            1.0f / c->tile.height, nullptr};
}

// A ptss_*_launches getter: the null checks, then the counter as wide as its member is.
template <size_t K>
static inline int readLaunches(const ptss_context* c, unsigned long long (ptss_context::*counter)[K], unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    memcpy(out, c->*counter, sizeof(c->*counter));
    return PTSS_OK;
}
static inline int readLaunches(const ptss_context* c, unsigned long long ptss_context::*counter, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->*counter;
    return PTSS_OK;
}

// A ptss_debug_*_form setter: `accepted` has bit f set for every form f the call takes.
static inline int setForm(ptss_context* c, int ptss_context::*form, int value, unsigned accepted, const char* refusal) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (value < 0 || value > 31 || !(accepted >> value & 1u)) return fail(PTSS_EINVAL, refusal);
    c->*form = value;
    return PTSS_OK;
}

// k device words at `src`, behind everything the stream of `last` holds.
static inline int readBehind(ptss_context* c, const LastStream& last, const unsigned long long* src, int k, unsigned long long* out) {
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(last.synchronize());
    HIP_TRY(hipMemcpy(out, src, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PTSS_OK;
}
