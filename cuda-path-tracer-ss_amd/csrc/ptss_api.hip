// ptss_api.hip — context management and the frame driver behind include/ptss.h.
//
// ptss_generate_frame is the reference's generateFrame (CudaTracer/CudaTracer.cu:587-647) with the
// host taken out of the inner loop: the per-bounce live-ray count stays on the device
// (FrameBuffers::counts), every bounce kernel is launched unconditionally and applies the
// reference's `numRays > 128` guard itself, so a frame is one uninterrupted stream of launches
// with at most one event wait at the end (cfg.syncEachFrame, the reference's :639-642).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "ptss.h"
#include "ptss_device.h"
#include <algorithm>
#include "ptdenoise.h"
#include "ptupsample.h"
#include "ptreproject.h"
#include "ptspecular.h"
#include "ptpack.h"
#include "ptstrip.h"
#include "ptcamera.h"
#include "ptadaptive.h"
#include "ptlinear.h"
#include "ptlinstats.h"
#include "ptsplat.h"
#include "ptmeter.h"
#include "ptglare.h"
#include "pttone.h"
#include "ptlindn.h"
#include "ptlinrp.h"
#include "ptlinup.h"
#include "ptsurface.h"
#include "ptlightmap.h"

using namespace ptv;
using ptpack::cameraInRange;
static_assert(sizeof(ptpack::Row) == sizeof(float4) && alignof(ptpack::Row) == alignof(float4), "a packed row is uploaded as a float4");

#if PTSS_DIAG
namespace ptss { hipError_t readDiagCounters(unsigned long long* out8); }
#endif
namespace {

thread_local std::string g_detail;

int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf, sizeof(buf), "%s", what);
    g_detail = buf;
    return code;
}

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return fail(PTSS_EHIP, #expr, _e); \
    } while (0)

#define RC_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)   // a step that reports a PTSS_* code

struct EventPair {
    hipEvent_t a, b;
};

}  // namespace

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

struct ptss_context {
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
    unsigned long long* dTotal = nullptr;   // [0 .. kMaxLanes) ray-bounce totals per lane, [kMaxLanes]: records ptss_update_triangles
                                            // rejected (kRejectedWord), [kMaxLanes + 1]: index entries the film calls dropped (kFilmRejectedWord),
                                            // [kMaxLanes + 2], [+ 3]: samples the splat calls dropped and clamped (kSplatCountersWord),
                                            // [kMaxLanes + 4]: entries ptss_generate_rays_surface dropped (kSurfaceRejectedWord),
                                            // [kMaxLanes + 5 .. +8) unused, then one word: guard timeouts (must stay 0)
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
    int lastResetTick = 0;
    int lastTicks = 0;
    unsigned maxIterations = 15;
    bool resetTicksThisFrame = true;
    bool usePathTracer = true;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    float lastMs = 0.0f;
    int gridCap = 0;             // workgroups per shard at most = 16 resident rounds of this scene's bounce kernel (0 = uncapped)
    unsigned frameIndex = 0;
    // bounce-kernel timing (cfg.timeKernels): every launch is bracketed by two events on ITS stream; a finished pair becomes
    // an interval [start, end) in ms since evEpoch. ptss_bounce_kernel_time reports the UNION of the intervals: with one lane
    // that is the sum of the launch durations, with several lanes (whose kernels overlap in time) the time during which at
    // least one bounce kernel was running — the figure a launch-time roofline needs.
    std::vector<EventPair> evFree, evBusy;
    std::vector<std::pair<double, double>> kernelSpans;
    hipEvent_t evEpoch = nullptr;
    unsigned int timeoutsSeen = 0;   // ptss_guard_timeouts value already reported as PTSS_ETIMEOUT
    unsigned long long launchedKernels = 0;   // bounce / frame kernel instantiations enqueued since ptss_create (ptss_launched_kernels)
    unsigned long long specularFeatureLaunches[2] = {0, 0};   // ptss_render_features_specular launches: [0] in place, [1] in LDS
    unsigned long long upsampleLaunches = 0;                  // ptss_upsample launches
    unsigned long long pathLaunches[2] = {0, 0};              // ptss_trace_paths launches: [0] in place, [1] in LDS
    uint32_t* dPathJumpTable = nullptr;                       // ptss_seed_path_rng's 2^67 jump table, uploaded by its first launching call
    unsigned long long refillLaunches[2] = {0, 0};            // ptss_trace_paths_opt launches with PTSS_PATHS_REFILL: [0] in place, [1] in LDS
    unsigned long long* dPathRefill = nullptr;                // their queue head and counters (ptss_device.h launchPathRefill), allocated by the first
    hipStream_t refillStream = nullptr;                       // the stream of the latest of them (ptss_path_refill_stats synchronises on it)
    unsigned long long filmLaunches[3] = {0, 0, 0};           // ptss_generate_rays, ptss_accumulate_paths, ptss_ray_features calls that launched
    hipStream_t filmStream = nullptr;                         // the stream of the latest film call with an index (ptss_film_rejected synchronises on it)
    bool filmIndexed = false;
    unsigned long long adaptiveLaunches[2] = {0, 0};          // ptss_accumulate_paths_stats, ptss_plan_samples calls that launched
    unsigned long long linearLaunches[2] = {0, 0};            // ptss_accumulate_paths_linear, ptss_resolve_linear calls that launched
    unsigned long long linStatsLaunches[2] = {0, 0};          // ptss_accumulate_paths_linear_stats, ptss_plan_samples_linear calls that launched
    unsigned long long splatLaunches[3] = {0, 0, 0};          // ptss_splat_paths, ptss_splat_paths_homed, ptss_resolve_splat calls that launched
    unsigned long long meterLaunches[3] = {0, 0, 0};          // meter histograms, ptss_meter_exposure, metered resolves that launched
    unsigned long long glareLaunches[3] = {0, 0, 0};          // glare builds, the kernels they launched, glare resolves that launched
    unsigned long long linDenoiseLaunches[2] = {0, 0};        // ptss_denoise_linear calls that launched, the kernels inside them
    unsigned long long linReprojectLaunches = 0;              // ptss_reproject_linear calls that launched
    unsigned long long linUpsampleLaunches = 0;               // ptss_upsample_linear calls that launched
    int linUpsampleForm = 0;                                  // ptss_debug_upsample_linear_form: 0 the measured table, 1 global memory, 2 staged
    unsigned long long toneLaunches[2] = {0, 0};              // ptss_tone_build, ptss_resolve_toned calls that launched
    unsigned long long surfaceLaunches[2] = {0, 0};           // ptss_generate_rays_surface, ptss_dilate_linear calls that launched
    hipStream_t surfaceStream = nullptr;                      // the stream of the latest ptss_generate_rays_surface (ptss_surface_rejected synchronises on it)
    bool surfaceCounted = false;
    int dilateForm = 0;                                       // ptss_debug_dilate_linear_form: 0 the shipped form, 1 global memory, 2 staged
    unsigned long long lightmapLaunches = 0;                  // ptss_lookup_lightmap calls that launched
    unsigned long long lightmapChainLaunches = 0;             // ptss_lookup_lightmap_chain calls that launched
    unsigned long long chainLaunches[2] = {0, 0};             // ptss_intersect_chain launches: [0] one lane per ray, [1] refill
    uint32_t* dChainHead = nullptr;                           // the refill schedule's queue head (ptss_device.h launchChainRefill), allocated by its first call
    int lightmapForm = 0;                                     // ptss_debug_lightmap_form: 0 the shipped form, 1 one lane per hit, 2 four lanes per hit
    int toneForm = 0;                                         // ptss_debug_tone_form: 0 the shipped lookup, 1 staged in LDS, 2 guess and settle
    int linDenoiseForm = 0;                                   // ptss_debug_denoise_linear_form: 0 the measured table, 1 unstaged, 2 staged, 4 + mask
    hipStream_t splatStream = nullptr;                        // the stream of the latest splat (ptss_splat_stats synchronises on it)
    bool splatCounted = false;
    float4* dDenoise[2] = {nullptr, nullptr};   // ptss_denoise's ping-pong colour planes, allocated by its first call with levels >= 2
    int denoiseLastPlane = -1;                  // the plane the last non-final pass of the latest ptss_denoise wrote (-1: none), and its
    int denoiseLastLevel = -1;                  // level; on denoiseStream (ptss_read_denoise_plane)
    hipStream_t denoiseStream = nullptr;
    int numCUs = 0;                             // hipDeviceProp_t::multiProcessorCount of cfg.device (sceneState's launch caps)
    hipStream_t updateStream = nullptr;         // the stream of the latest ptss_update_triangles (its read-backs synchronise on it)
    bool updated = false;                       // (ptss_resort_triangles records its stream here as well)
    ptss::ResortScratch resortScratch;          // ptss_resort_triangles' device scratch, allocated by its first launching call
    unsigned long long resortLaunches = 0;      // ptss_resort_triangles calls that launched
};
constexpr int kTotalWords = ptss::kMaxLanes + 8 + 1;
constexpr int kRejectedWord = ptss::kMaxLanes;
constexpr int kFilmRejectedWord = ptss::kMaxLanes + 1;
constexpr int kSurfaceRejectedWord = ptss::kMaxLanes + 4;   // entries ptss_generate_rays_surface dropped
constexpr int kSplatCountersWord = ptss::kMaxLanes + 2;   // two words: samples the splat calls dropped, samples they clamped

namespace {

// the checks of a scene description (ptpack.h), as a PTSS_* code
int validateScene(const ptss_scene_desc& s) {
    const char* what = ptpack::validateScene(s);
    return what ? fail(PTSS_EINVAL, what) : PTSS_OK;
}

// rows of the frame this context owns: bands of cfg.bandRows rows, dealt round-robin to the tileWorld ranks
int localRows(const ptss_render_config& cfg) {
    int rows = 0;
    for (int y = 0; y < cfg.height; ++y)
        if ((y / cfg.bandRows) % cfg.tileWorld == cfg.tileRank) ++rows;
    return rows;
}

// ptss_create's failures: PTSS_ENOMEM when the device ran out of memory, PTSS_EHIP for any other HIP error
int createCheck(hipError_t e, const char* what) { return e == hipSuccess ? PTSS_OK : fail(e == hipErrorOutOfMemory ? PTSS_ENOMEM : PTSS_EHIP, what, e); }
#define ALLOC_TRY(expr) RC_TRY(createCheck((expr), #expr))
template <class T>
hipError_t mallocZeroed(T** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? hipMemset(*p, 0, bytes) : e;
}

// ---- the scene-dependent part of a context (ptss_create and ptss_set_scene) ------------------------------------------------------
// Which images the scene gets, their blobs on the device, how the frames read each of them, and the launch caps that follow.
// Everything else a context owns — pools, random streams, accumulator, counters — does not depend on the scene.
struct SceneState {
    SceneImage images[2];
    int gridCap = 0;
    float defaultColor[3] = {0, 0, 0};
};
void releaseSceneState(SceneState& st) {
    for (SceneImage& im : st.images) {
        (void)hipFree(im.dBlob);
        im = SceneImage{};
    }
}
// Fills `st` (empty on entry) or leaves nothing allocated. numLanes, maxBlocks0: the context's lanes and lane 0's widest grid.
int buildSceneState(const ptss_scene_desc& scene, const ptss_render_config& cfg, int numLanes, int maxBlocks0, int numCUs, SceneState& st) {
    std::vector<ptpack::PackedImage> packed;   // which images the scene gets, and their rows: ptpack.h
    try {
        packed = ptpack::packImages(scene, cfg.everySphereLoop != 0);
    } catch (const std::bad_alloc&) {
        return fail(PTSS_ENOMEM, "scene image (host)");
    }
    const int numImages = (int)packed.size();
    for (int i = 0; i < numImages; ++i) {
        SceneImage& im = st.images[i];
        im.layout = packed[(size_t)i].layout;
        im.inLds = packed[(size_t)i].inLds;
        im.guardFlags = ptpack::sceneGuardFlags(scene);
        const std::vector<ptpack::Row>& blob = packed[(size_t)i].blob;
        hipError_t e = hipMalloc(&im.dBlob, blob.size() * sizeof(float4));
        if (e == hipSuccess) e = hipMemcpy(im.dBlob, blob.data(), blob.size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            releaseSceneState(st);
            return createCheck(e, "scene image (device)");
        }
    }
    st.defaultColor[0] = scene.defaultColor.x;
    st.defaultColor[1] = scene.defaultColor.y;
    st.defaultColor[2] = scene.defaultColor.z;
    // Launches wider than 16 resident rounds stop growing: a workgroup then walks several tiles and stages the scene
    // into LDS once for all of them. One round = CUs x workgroups per CU of THIS scene's bounce kernel (LDS image and
    // register budget decide: 7 for the 38-primitive scenes, 3-4 for the many-sphere image), so 16 rounds =
    // CUs x perCU workgroups per shard (kShards = 16 shards). Measured on the mixed scene (256 x 7 = 1,792 per shard):
    // 448: -4.6 %, 896: -1.3 %, 1,280-3,584: equal, uncapped: -2 % (profiles/README.md).
    const SceneImage& primary = st.images[0];   // (not recomputed when the frames switch to images[1])
    const int perCU = ptss::bounceOccupancyBlocksPerCU(primary.layout, primary.inLds, primary.layout.sphereBounded != 0);
    st.gridCap = numCUs * (perCU > 0 ? perCU : 4) * 16 / ptss::kShards;
    // One launch per frame (ptss_kernels.hip frameKernel): only when every workgroup of the frame's grid is resident at once —
    // its workgroups wait for each other — i.e. bounce-0 tiles <= CUs x resident workgroups per CU of THAT kernel with this
    // scene's LDS image. The occupancy API over-reports by one workgroup per CU for kernels of more than 96 SGPRs
    // (MI355X_MICROARCH.md, "Residency and cooperative launch"): one is kept in reserve. One lane, scene staged in LDS.
    // A bounded image runs the bounded or the unbounded frame kernel, as the camera is in range or not: both must fit.
    auto qualifies = [&](const SceneImage& im) {
        if (cfg.oneLaunchFrames <= 0 || numLanes != 1 || !im.inLds) return false;   // opt-in (include/ptss.h)
        if (ptss::meshImage(im.layout)) return false;   // the mesh image has no frame kernel
        int perCU = ptss::frameOccupancyBlocksPerCU(im.layout, false);
        if (im.layout.sphereBounded) perCU = std::min(perCU, ptss::frameOccupancyBlocksPerCU(im.layout, true));
        const int resident = perCU - 1;
        return resident >= 1 && maxBlocks0 <= numCUs * resident;
    };
    for (int i = 0; i < numImages; ++i) st.images[i].oneLaunch = qualifies(st.images[i]);
#ifdef PTSS_TUNING_KNOBS   // measurement builds only (tools/build_variants.py "knobs"); the shipped library reads no environment
    if (const char* e = getenv("PTSS_SCENE_PATH")) {
        if (!strcmp(e, "scalar"))
            for (int i = 0; i < numImages; ++i) st.images[i].inLds = false;
    }
    if (const char* e = getenv("PTSS_GRID_CAP")) st.gridCap = atoi(e);
#endif
    return PTSS_OK;
}
void adoptSceneState(ptss_context* c, const SceneState& st) {
    for (int i = 0; i < 2; ++i) c->images[i] = st.images[i];
    c->gridCap = st.gridCap;
    for (int k = 0; k < 3; ++k) c->defaultColor[k] = st.defaultColor[k];
    c->active = 0;
}

// A lane's device resources (ptss_create). releaseLane frees whatever of them exists: ptss_destroy, also after a failed create.
int allocLane(Lane& ln, const uint32_t (&shardCount0)[ptss::kShards], bool ownStream) {
    const size_t poolBytes = (size_t)ptss::kRayPlanes * ln.regionCap * ptss::kShards * sizeof(float);
    for (float*& pool : ln.dPool) ALLOC_TRY(hipMalloc(&pool, poolBytes));
    for (uint32_t*& counts : ln.dCounts) ALLOC_TRY(mallocZeroed(&counts, ptss::kCountWords * sizeof(uint32_t)));
    ALLOC_TRY(mallocZeroed(&ln.dLastCounts, ptss::kCountWords * sizeof(uint32_t)));
    for (int s = 0; s < ptss::kShards; ++s)  // arm bounce 0 of the first frame (flushKernel arms every later one)
        ALLOC_TRY(hipMemcpy(ln.dCounts[0] + ptss::countIndex(0, s), &shardCount0[s], sizeof(uint32_t), hipMemcpyHostToDevice));
    ALLOC_TRY(hipMalloc(&ln.dShardCount0, sizeof(shardCount0)));
    ALLOC_TRY(hipMemcpy(ln.dShardCount0, shardCount0, sizeof(shardCount0), hipMemcpyHostToDevice));
    ALLOC_TRY(mallocZeroed(&ln.dDone, (ptss::kCountWords + ptss::kCountStride) * sizeof(uint32_t)));  // + the finished-frames counter
    if (ownStream) {
        ALLOC_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        for (hipEvent_t& ev : ln.evDone) ALLOC_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    ALLOC_TRY(hipHostMalloc(&ln.hCounts, 4 * ptss::kCountWords * sizeof(uint32_t), hipHostMallocDefault));
    for (hipEvent_t& ev : ln.hintEvent) ALLOC_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return PTSS_OK;
}
#undef ALLOC_TRY

// curandSetupKernel (CudaTracer.cu:722-724): per-pixel subsequence via the 2^67 jump table, on stream st; returns once it has run
// (ptss_create, ptss_reseed)
hipError_t seedStreams(ptss_context* c, unsigned long long seed, hipStream_t st) {
    std::vector<uint32_t> table(ptrng::kJumpTableWords);
    ptrng::build_subsequence_table(table.data());
    uint32_t* dTable = nullptr;
    hipError_t e = hipMalloc(&dTable, table.size() * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    e = hipMemcpy(dTable, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && c->numPixels > 0) e = ptss::launchRngInit(st, c->dRngHome, c->capacity, c->samples, c->tile, seed, dTable);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dTable);
    return e;
}

// everything this context has enqueued on its own streams has run (ptss_set_scene, ptss_reseed)
int quiesce(ptss_context* c) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Lane& ln : c->lanes)
        if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
    return PTSS_OK;
}

void releaseLane(Lane& ln) {
    for (hipEvent_t ev : ln.hintEvent)
        if (ev) (void)hipEventDestroy(ev);
    if (ln.hCounts) (void)hipHostFree(ln.hCounts);
    (void)hipFree(ln.dDone);
    for (hipEvent_t ev : ln.evDone)
        if (ev) (void)hipEventDestroy(ev);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
    for (float* pool : ln.dPool) (void)hipFree(pool);
    for (uint32_t* counts : ln.dCounts) (void)hipFree(counts);
    (void)hipFree(ln.dShardCount0);
    (void)hipFree(ln.dLastCounts);
}

ptss::FrameBuffers frameBuffers(const ptss_context* c, int laneIdx, ptss_uchar4* pixels, int sample) {
    const Lane& ln = c->lanes[(size_t)laneIdx];
    ptss::FrameBuffers fb{};
    fb.pool[0] = ln.dPool[0];
    fb.pool[1] = ln.dPool[1];
    fb.rngHome = c->dRngHome;
    fb.counts = ln.dCounts[c->countParity];
    fb.countsNext = ln.dCounts[1 - c->countParity];
    fb.shardCount0 = ln.dShardCount0;
    fb.lastCounts = ln.dLastCounts;
    fb.totalRayBounces = c->dTotal + laneIdx;
    fb.guardTimeouts = reinterpret_cast<uint32_t*>(c->dTotal + ptss::kMaxLanes + 8);
    fb.accum = c->dAccum;
    fb.fsum = c->dFsum;
    fb.staged = c->dStaged ? c->dStaged + (c->stagedTwice ? (size_t)(c->frameIndex & 1u) * c->capacity * c->samples : 0) : nullptr;
    fb.quantTable = reinterpret_cast<const float*>(c->image().dBlob + c->image().layout.offQuant);
    fb.pixels = pixels;
    fb.regionCap = ln.regionCap;
    fb.numPixels = c->numPixels;
    fb.plane = c->capacity;
    fb.samples = c->samples;
    fb.firstTiles = c->samples * (c->capacity / ptss::kBlock);
    // The reference stops bouncing once <= 128 rays are live IN THE WHOLE FRAME (CudaTracer.cu:622). A
    // shard of a multi-GPU frame cannot know the frame-wide count without a collective per bounce, so a context with
    // tileWorld > 1 never stops early; the two agree whenever the frame-wide count stays above 128. (The lanes of ONE
    // context do know each other's counts: the guard is exact for any number of lanes.)
    fb.minLive = c->tile.world > 1 ? 0u : ptss::kMinLiveRays;
    fb.inverseTicks = 1.f / (float)((int)c->samples * (sample + 1));  // CudaTracer.cu:94 (S = 1: 1.f / (ticks + 1))
    fb.defaultColor[0] = c->defaultColor[0];
    fb.defaultColor[1] = c->defaultColor[1];
    fb.defaultColor[2] = c->defaultColor[2];
    fb.guardFlags = c->image().guardFlags;
    fb.laneIndex = (uint32_t)laneIdx;
    fb.laneCount = (uint32_t)c->lanes.size();
    fb.frameRays = c->numPixels * c->samples;
    fb.numPeers = fb.laneCount - 1;
    fb.myDone = ln.dDone;
    fb.myFrameDone = ln.dDone + ptss::kCountWords;
    fb.frameSeq = c->frameIndex;
    fb.joinsFrame = (laneIdx + 1 == (int)c->lanes.size()) ? 1u : 0u;
    uint32_t p = 0;
    for (size_t k = 0; k < c->lanes.size(); ++k) {
        if ((int)k == laneIdx) continue;
        fb.peerCounts[p] = c->lanes[k].dCounts[c->countParity];
        fb.peerDone[p] = c->lanes[k].dDone;
        fb.peerFrameDone[p] = c->lanes[k].dDone + ptss::kCountWords;
        ++p;
    }
    return fb;
}

void drainKernelEvents(ptss_context* c, bool wait) {
    size_t k = 0;
    for (size_t i = 0; i < c->evBusy.size(); ++i) {
        EventPair p = c->evBusy[i];
        hipError_t q = wait ? hipEventSynchronize(p.b) : hipEventQuery(p.b);
        if (q == hipSuccess) {
            float start = 0, ms = 0;   // start since the epoch (coarse at large values), duration from the pair itself (exact)
            if (hipEventElapsedTime(&start, c->evEpoch, p.a) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess)
            {
                if (c->kernelSpans.size() >= (1u << 20)) c->kernelSpans.clear();   // nobody is asking (ptss_bounce_kernel_time empties it)
                c->kernelSpans.emplace_back((double)start, (double)start + (double)ms);
            }
            c->evFree.push_back(p);
        } else {
            c->evBusy[k++] = p;
        }
    }
    c->evBusy.resize(k);
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is not an error
}

// Frame lanes: did a lane give up waiting for a peer since the last check (FrameBuffers::guardTimeouts)? Called by the
// entry points that have just synchronised; one 4-byte read-back, and only in contexts with more than one lane.
int checkLaneTimeouts(ptss_context* c) {
    if (c->lanes.size() < 2 && !c->images[0].oneLaunch && !c->images[1].oneLaunch) return PTSS_OK;   // only kernels that wait for others can time out
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, c->dTotal + ptss::kMaxLanes + 8, sizeof(v), hipMemcpyDeviceToHost));
    if (v != c->timeoutsSeen) {
        c->timeoutsSeen = v;
        return fail(PTSS_ETIMEOUT, "a bounded wait on the device expired (a frame lane for a peer lane, or a workgroup of the one-launch "
                                   "frame kernel for its shard): the frame was not traced as specified");
    }
    return PTSS_OK;
}

// ---- the steps of a frame (ptss_generate_frame) ------------------------------------------------------------------------
// The chunked image assumes a camera within the geometry's magnitude range (ptpack.h): outside it the frames use the plain one.
void selectImage(ptss_context* c) {
    if (!c->images[1].dBlob) return;
    const int want = cameraInRange(c->camera) ? 0 : 1;
    if (want != c->active) {
        c->active = want;
        c->cameraDirty = true;
    }
}

ptss::EyeParams eyeParams(const ptss_context* c) {   // {camera, s (CudaTracer.cu:334), aspect, invW, invH}
    return {c->camera, -2 * ptm::tan(c->camera.fieldOfView * 0.5f), (float)c->tile.height / (float)c->tile.width, 1.0f / c->tile.width,
            1.0f / c->tile.height, nullptr};
}

// harvest the newest finished live-count readbacks (never blocks)
void harvestHints(ptss_context* c) {
    for (Lane& ln : c->lanes)
        for (int q = 0; q < 4; ++q) {
            if (!ln.hintPending[q] || hipEventQuery(ln.hintEvent[q]) != hipSuccess) continue;
            const uint32_t* src = ln.hCounts + (size_t)q * ptss::kCountWords;
            for (int b = 0; b <= ptss::kMaxBounces; ++b) {
                uint32_t mx = 0;
                for (int s = 0; s < ptss::kShards; ++s) mx = std::max(mx, src[ptss::countIndex(b, s)]);
                ln.hint[b] = mx;
            }
            ln.haveHint = true;
            ln.hintPending[q] = false;
        }
    (void)hipGetLastError();
}

// Several lanes: each runs on its own stream, forked from the caller's here and joined into it by flushAndJoin; their
// launches are issued round-robin, bounce by bounce, so that the streams advance together.
// STRICT ordering (the default): every frame forks, so the lanes start behind whatever the caller put on its stream
// before this call — a reader of the previous frame's pixels or accumulator, a zero-fill, a newly bound buffer's writer.
// FREE-RUNNING (cfg.lanesFreeRun, opt-in): the fork happens only when the library's own work on the caller's stream
// requires it (the clear of a reset, the camera precomputes) — otherwise a lane's next frame depends on nothing but
// its own previous one, and the lanes run on, frame after frame, while the caller's stream merely waits for each
// frame's end (the join); the caller has promised not to touch the buffers in between (include/ptss.h).
int forkLanes(ptss_context* c, bool forkNeeded) {
    if (c->lanes.size() > 1 && (forkNeeded || c->frameIndex == 0 || !c->cfg.lanesFreeRun)) {
        HIP_TRY(hipEventRecord(c->evFork, c->stream));
        for (Lane& ln : c->lanes) HIP_TRY(hipStreamWaitEvent(ln.stream, c->evFork, 0));
    }
    // Free-running lanes with S > 1: this frame parks its samples in the buffer of its parity, which displayKernel of the frame
    // two back (same parity, on the caller's stream) must have emptied — the only thing a free-running lane ever waits for
    // on the caller's side, and an event that has nearly always fired by now.
    if (c->stagedTwice && c->frameIndex >= 2)
        for (Lane& ln : c->lanes) HIP_TRY(hipStreamWaitEvent(ln.stream, c->evDisplay[c->frameIndex & 1u], 0));
    return PTSS_OK;
}

// cfg.timeKernels: brackets the one kernel that launch() enqueues on stream s with an event pair (drainKernelEvents)
template <class Launch>
int timedLaunch(ptss_context* c, hipStream_t s, Launch launch) {
    if (!c->cfg.timeKernels) return launch();
    EventPair ev{nullptr, nullptr};
    if (c->evFree.empty() && c->evBusy.size() >= 4096) drainKernelEvents(c, true);
    if (c->evFree.empty()) {
        HIP_TRY(hipEventCreate(&ev.a));
        HIP_TRY(hipEventCreate(&ev.b));
    } else {
        ev = c->evFree.back();
        c->evFree.pop_back();
    }
    HIP_TRY(hipEventRecord(ev.a, s));
    RC_TRY(launch());
    HIP_TRY(hipEventRecord(ev.b, s));
    c->evBusy.push_back(ev);
    return PTSS_OK;
}

// every bounce in ONE launch (frameKernel): CudaTracer.cu:622-633 without leaving the device; its grid is the frame's tiles
int traceOneLaunch(ptss_context* c, const ptss::FrameBuffers& fb, int numIterations, bool bounded, const ptss::EyeParams& eye) {
    const SceneImage& im = c->image();
    return timedLaunch(c, c->stream, [&] {
        HIP_TRY(ptss::launchFrame(c->stream, fb, im.dBlob, im.layout, numIterations, bounded, c->lanes[0].maxBlocks, c->tile, eye,
                                          &c->launchedKernels));
        return PTSS_OK;
    });
}

// one launch per bounce and lane (CudaTracer.cu:622-633, guard evaluated on the device), the lanes round-robin inside a bounce
int traceBounces(ptss_context* c, ptss::FrameBuffers* fbs, int numIterations, bool bounded, const ptss::EyeParams& eye) {
    const SceneImage& im = c->image();
    const int K = (int)c->lanes.size();
    for (int i = 0; i < numIterations; ++i)
        for (int k = 0; k < K; ++k) {
            Lane& ln = c->lanes[(size_t)k];
            const hipStream_t ls = K > 1 ? ln.stream : c->stream;
            // grid: one tile per workgroup for the expected live count (+1.5 %), never more than the lane's share of the
            // frame; the kernel grid-strides, so a low hint costs time, not correctness
            int blocks = ln.maxBlocks;
            if (i > 0 && ln.haveHint) {
                // tiles for the fullest shard (+1.5 %), times kShards (workgroup b serves shard b % kShards)
                const unsigned long long tilesPerShard = ((unsigned long long)ln.hint[i] * 65 / 64 + ptss::kBlock) / ptss::kBlock + 1;
                const unsigned long long want = tilesPerShard * ptss::kShards;
                if (want < (unsigned long long)blocks) blocks = (int)want;
            }
            // launches wider than 16 resident rounds stop growing (gridCap, ptss_create)
            if (c->gridCap > 0 && c->gridCap * ptss::kShards < blocks) blocks = c->gridCap * ptss::kShards;
            // the peers' done totals once their bounce i - 1 of this frame has ended (all of those launches precede this
            // one in host order, so a kernel that waits for them never waits for something behind it in a shared queue)
            if (i > 0)
                for (int j = 0, p = 0; j < K; ++j)
                    if (j != k) fbs[k].peerTarget[p++] = c->lanes[(size_t)j].doneTarget[i - 1];
            RC_TRY(timedLaunch(c, ls, [&] {
                HIP_TRY(ptss::launchBounce(ls, fbs[k], im.dBlob, im.layout, i, i == numIterations - 1, im.inLds, bounded, blocks, c->tile, eye,
                                               &c->launchedKernels));
                return PTSS_OK;
            }));
            ln.doneTarget[i] += (uint32_t)blocks;  // every workgroup of the launch adds 1 to done[i][its shard] as it ends
        }
    return PTSS_OK;
}

// flushKernel of every lane (CudaTracer.cu:637), the live-count readbacks for later grids, and the join into the caller's stream
int flushAndJoin(ptss_context* c, const ptss::FrameBuffers* fbs, int numIterations) {
    const int K = (int)c->lanes.size();
    for (int k = 0; k < K; ++k) {
        Lane& ln = c->lanes[(size_t)k];
        const hipStream_t ls = K > 1 ? ln.stream : c->stream;
        // (flushKernel itself waits, on the device, until every peer lane has finished the previous frame: FrameBuffers::myFrameDone)
        ptss::FlushTargets targets{};
        for (int j = 0, p = 0; j < K; ++j)
            if (j != k) {
                for (int b = 0; b <= ptss::kMaxBounces; ++b) targets.target[p][b] = c->lanes[(size_t)j].doneTarget[b];
                ++p;
            }
        HIP_TRY(ptss::launchFlush(ls, fbs[k], numIterations, targets));
        // every 8th frame (and until a hint exists) copy counts[] to pinned memory for later grid sizing
        if (!ln.haveHint || (c->frameIndex & 7u) == 0) {
            const int q = (int)((c->frameIndex >> 3) & 3u);
            if (!ln.hintPending[q]) {
                HIP_TRY(hipMemcpyAsync(ln.hCounts + (size_t)q * ptss::kCountWords, ln.dLastCounts, ptss::kCountWords * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, ls));
                HIP_TRY(hipEventRecord(ln.hintEvent[q], ls));
                ln.hintPending[q] = true;
            }
        }
        // the join: the caller's stream is ordered behind every lane's frame (the lanes themselves run on) — ONE event, behind
        // the last lane's flushKernel, which ends only when every other lane's has (FrameBuffers::joinsFrame); an event per lane cost 1-2 %
        if (K > 1 && k == K - 1) {
            HIP_TRY(hipEventRecord(ln.evDone[c->frameIndex & 1u], ls));
            HIP_TRY(hipStreamWaitEvent(c->stream, ln.evDone[c->frameIndex & 1u], 0));
        }
    }
    return PTSS_OK;
}

}  // namespace

extern "C" {

int ptss_version(void) { return PTSS_VERSION; }

const char* ptss_error_string(int code) {
    switch (code) {
        case PTSS_OK: return "ok";
        case PTSS_EINVAL: return "invalid argument";
        case PTSS_EHIP: return "HIP runtime error";
        case PTSS_ENODEVICE: return "no usable HIP device";
        case PTSS_ENOMEM: return "out of memory";
        case PTSS_ERANGE: return "buffer too small or index out of range";
        case PTSS_ETIMEOUT: return "a frame lane timed out waiting for a peer lane";
        default: return "unknown error";
    }
}

const char* ptss_last_error_detail(void) { return g_detail.c_str(); }

int ptss_default_config(ptss_render_config* cfg) {
    if (!cfg) return fail(PTSS_EINVAL, "cfg is null");
    memset(cfg, 0, sizeof(*cfg));
    cfg->structSize = (unsigned int)sizeof(*cfg);
    cfg->width = 512;  // DIM, CudaUtils.h:7
    cfg->height = 512;
    cfg->seed = 0x5EEDull;
    cfg->maxIterations = 15;  // CudaTracer.h:39
    cfg->device = 0;
    cfg->tileRank = 0;
    cfg->tileWorld = 1;
    cfg->bandRows = 8;
    cfg->syncEachFrame = 1;
    cfg->floatAccumulator = 0;
    cfg->timeKernels = 0;
    cfg->samplesPerPass = 1;
    cfg->everySphereLoop = 0;
    cfg->frameLanes = 0;
    cfg->lanesFreeRun = 0;
    cfg->oneLaunchFrames = 0;
    return PTSS_OK;
}

int ptss_create(const ptss_scene_desc* scene, const ptss_render_config* cfg, ptss_context** out) {
    if (!scene || !cfg || !out) return fail(PTSS_EINVAL, "null argument");
    if (cfg->structSize != (unsigned int)sizeof(ptss_render_config))
        return fail(PTSS_EINVAL, "cfg->structSize is not this library's sizeof(ptss_render_config): the caller was built against another "
                                 "ptss.h (compare ptss_version() with PTSS_VERSION) or did not start from ptss_default_config");
    if (cfg->width <= 0 || cfg->height <= 0 || (long long)cfg->width * cfg->height > (1ll << 31) - 256)
        return fail(PTSS_EINVAL, "bad frame size");
    if (cfg->maxIterations == 0 || cfg->maxIterations > (unsigned)ptss::kMaxBounces)
        return fail(PTSS_EINVAL, "maxIterations must be in [1, 64]");
    if (cfg->tileWorld <= 0 || cfg->tileRank < 0 || cfg->tileRank >= cfg->tileWorld || cfg->bandRows <= 0)
        return fail(PTSS_EINVAL, "bad tile spec");
    const int spp = cfg->samplesPerPass == 0 ? 1 : cfg->samplesPerPass;
    if (spp < 1 || spp > 64) return fail(PTSS_EINVAL, "samplesPerPass must be in [1, 64]");
    if ((long long)cfg->width * cfg->height >= (1ll << 26)) return fail(PTSS_EINVAL, "frame too large (>= 2^26 pixels)");
    {
        // A ray's word inside its shard's region is addressed in 32 bits (slotWord: 19 planes per block): the rays of one
        // pass — local pixels x sample lanes, rounded up to whole tiles per shard — must stay below 2^32 / 19 (~226
        // million; the whole pool may be larger than 4 GB, regions are based with 64-bit arithmetic).
        const long long rows = localRows(*cfg);
        const unsigned long long rays = ((unsigned long long)cfg->width * rows + 255ull) / 256ull * 256ull * (unsigned long long)spp;
        if ((rays + (unsigned long long)ptss::kShards * ptss::kBlock) * ptss::kRayPlanes >= (1ull << 32))
            return fail(PTSS_EINVAL, "too many rays per pass: width x local rows x samplesPerPass must stay below ~226 million");
    }
    int rc = validateScene(*scene);
    if (rc != PTSS_OK) return rc;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(PTSS_ENODEVICE, "hipGetDeviceCount found no device (libptss has no CPU path)", e);
    }
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PTSS_ENODEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(cfg->device));

    ptss_context* c = new (std::nothrow) ptss_context();
    if (!c) return fail(PTSS_ENOMEM, "context");
    c->cfg = *cfg;
    c->maxIterations = cfg->maxIterations;
    c->samples = (uint32_t)spp;
    // Camera(), RenderStructs.h:51-52
    c->camera.rotation = q4(1, 0, 0, 0);
    c->camera.position = v3(0, 0, 0);
    c->camera.zNear = -0.1f;
    c->camera.zFar = -100.0f;
    c->camera.fieldOfView = ptm::kPi / 2.0f;

    c->tile = ptss::TileMap{cfg->width, cfg->height, localRows(*cfg), cfg->tileRank, cfg->tileWorld, cfg->bandRows};
    c->numPixels = (uint32_t)cfg->width * (uint32_t)c->tile.localRows;
    const uint32_t gran = ptss::kBlock > 256 ? (uint32_t)ptss::kBlock : 256u;  // pixel planes are whole tiles
    c->capacity = ((c->numPixels + gran - 1) / gran) * gran;
    if (c->capacity == 0) c->capacity = gran;
    // Frame lanes (ptss_device.h): cfg.frameLanes, or by the size of a pass when 0 — launch-shaped passes (a few
    // resident rounds per launch) gain a fifth from a second lane, wide ones nothing.
    int numLanes = cfg->frameLanes;
    if (numLanes < 0 || numLanes > ptss::kMaxLanes) return (delete c, fail(PTSS_EINVAL, "frameLanes must be in [0, 4]"));
    {
        const unsigned long long rays = (unsigned long long)c->numPixels * c->samples;
        // measured (tools/lanes_bench.py / tools/s1_modes.py, Mrays/s with 1 / 2 lanes, one sample per tick, with the lanes coupled on
        // the device — flushKernel's finished-frames counters): 1920x1080 (2.1 M rays per pass) 13,800 / 16,300; 3840x2160, 1,024 spheres
        // (8.3 M) 4,110 / 4,360 (three lanes 4,580, four 3,470); 1280x720 (0.92 M) 10,010 / 11,160; 1024x576 (0.59 M) 8,050 / 9,090;
        // 800x600 (0.48 M) 7,490 / 7,900; 640x480 (0.31 M) 5,480 / 5,380; 512x512 (0.26 M) 4,730 / 4,570 — below ~0.2 ms a pass is ten launch
        // latencies, nothing to overlap; 1920x1080 S = 40 (83 M) 17,760 / 17,750. Four lanes (five streams with the caller's) share
        // hardware queues and serialise. (With the lanes coupled through stream events the gain at 1280x720 was inside the noise.)
        // All of that is the FREE-RUNNING mode (cfg.lanesFreeRun); ordered strictly on the caller's stream — a fork and a join per
        // frame — two lanes ran at 13,180 against one lane's 13,800, so the library's own choice is then one lane.
        // Round 3, wide passes again (tools/lanes_large.py, interleaved, twice): 3840x2160 S = 4, 12 bounces, 1,024 spheres (33 M rays per
        // pass, the late bounces a hundredth of that) 5,958-5,970 / 6,077; 1920x1080 S = 40 (83 M) 18,273-18,294 / 18,420-18,454: a second
        // lane is worth +2.0 % / +0.8 % there. The rule stays at 2^24 all the same: a caller who wants it asks for frameLanes = 2; by
        // default a wide pass keeps one lane, one set of pools (the second doubles 5-16 GB) and launches that do not overlap, so that
        // a kernel's duration means the same in a profile and in ptss_bounce_kernel_time.
        if (numLanes == 0) numLanes = (cfg->lanesFreeRun && rays >= (3ull << 17) && rays <= (1ull << 24)) ? 2 : 1;
    }
    c->lanes.resize((size_t)numLanes);
    uint32_t shardCount0[ptss::kMaxLanes][ptss::kShards] = {{0}};
    {
        // bounce 0 walks S sample planes of `capacity` pixels (capacity = numPixels rounded up to a tile); tile t belongs
        // to shard t % kShards and to round t / kShards, round R to lane R % numLanes
        const uint32_t tilesPerPlane = c->capacity / ptss::kBlock;
        const uint32_t tiles = tilesPerPlane * c->samples;
        const uint32_t rounds = (tiles + ptss::kShards - 1) / ptss::kShards;
        for (int k = 0; k < numLanes; ++k) {
            const uint32_t laneRounds = (rounds + (uint32_t)numLanes - 1 - (uint32_t)k) / (uint32_t)numLanes;
            c->lanes[(size_t)k].regionCap = (laneRounds ? laneRounds : 1) * ptss::kBlock;
            c->lanes[(size_t)k].maxBlocks = (int)(c->lanes[(size_t)k].regionCap / ptss::kBlock) * ptss::kShards;
        }
        for (uint32_t t = 0; t < tiles; ++t) {
            const uint32_t first = (t % tilesPerPlane) * ptss::kBlock;  // first pixel of the tile inside its plane
            uint32_t cnt = 0;
            if (first < c->numPixels) cnt = c->numPixels - first < (uint32_t)ptss::kBlock ? c->numPixels - first : (uint32_t)ptss::kBlock;
            shardCount0[(t / ptss::kShards) % (uint32_t)numLanes][t % ptss::kShards] += cnt;
        }
    }

#define CREATE_TRY(expr) do { if (int _rc = createCheck((expr), #expr)) return (ptss_destroy(c), _rc); } while (0)   // frees what exists

    {
        hipDeviceProp_t prop;
        CREATE_TRY(hipGetDeviceProperties(&prop, cfg->device));
        c->numCUs = prop.multiProcessorCount;
        SceneState st;
        if (int sceneRc = buildSceneState(*scene, *cfg, numLanes, c->lanes[0].maxBlocks, c->numCUs, st)) return (ptss_destroy(c), sceneRc);
        adoptSceneState(c, st);
    }
    CREATE_TRY(hipMalloc(&c->dRngHome, (size_t)ptss::kHomeWords * c->capacity * c->samples * sizeof(uint32_t)));
    for (int k = 0; k < numLanes; ++k)
        if (int laneRc = allocLane(c->lanes[(size_t)k], shardCount0[k], numLanes > 1)) return (ptss_destroy(c), laneRc);
    if (numLanes > 1) CREATE_TRY(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    CREATE_TRY(mallocZeroed(&c->dTotal, kTotalWords * sizeof(unsigned long long)));
    CREATE_TRY(mallocZeroed(&c->dAccumOwned, (size_t)3 * c->capacity * sizeof(uint32_t)));
    c->dAccum = c->dAccumOwned;
    if (cfg->floatAccumulator) CREATE_TRY(mallocZeroed(&c->dFsum, (size_t)3 * c->capacity * c->samples * sizeof(float)));
    if (c->samples > 1) {
        c->stagedTwice = numLanes > 1 && cfg->lanesFreeRun != 0;
        const size_t words = (size_t)c->capacity * c->samples * (c->stagedTwice ? 2 : 1);
        CREATE_TRY(mallocZeroed(&c->dStaged, words * sizeof(uint32_t)));
        if (c->stagedTwice)
            for (int q = 0; q < 2; ++q) CREATE_TRY(hipEventCreateWithFlags(&c->evDisplay[q], hipEventDisableTiming));
    }
    CREATE_TRY(hipMalloc(&c->dStrips, (size_t)(c->capacity / ptloc::kStrip) * sizeof(unsigned long long)));
    CREATE_TRY(hipEventCreate(&c->evStart));
    CREATE_TRY(hipEventCreate(&c->evStop));
    CREATE_TRY(hipEventCreate(&c->evEpoch));

    CREATE_TRY(seedStreams(c, cfg->seed, nullptr));
    CREATE_TRY(hipEventRecord(c->evEpoch, nullptr));
    CREATE_TRY(hipDeviceSynchronize());

#undef CREATE_TRY

    *out = c;
    return PTSS_OK;
}

int ptss_destroy(ptss_context* c) {
    if (!c) return PTSS_OK;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
    drainKernelEvents(c, true);
    for (EventPair& p : c->evFree) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (Lane& ln : c->lanes) releaseLane(ln);
    for (hipEvent_t ev : {c->evFork, c->evDisplay[0], c->evDisplay[1], c->evStart, c->evStop, c->evEpoch})
        if (ev) (void)hipEventDestroy(ev);
    for (SceneImage& im : c->images) (void)hipFree(im.dBlob);
    (void)hipFree(c->dRngHome);
    (void)hipFree(c->dTotal);
    (void)hipFree(c->dAccumOwned);
    (void)hipFree(c->dFsum);
    (void)hipFree(c->dStaged);
    (void)hipFree(c->dStrips);
    for (float4* plane : c->dDenoise) (void)hipFree(plane);
    ptss::releaseResortScratch(c->resortScratch);
    (void)hipFree(c->dPathJumpTable);
    (void)hipFree(c->dPathRefill);
    (void)hipFree(c->dChainHead);
    delete c;
    return PTSS_OK;
}

int ptss_generate_frame(ptss_context* c, ptss_uchar4* pixels, int ticks) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    hipStream_t st = c->stream;
    HIP_TRY(hipSetDevice(c->cfg.device));  // contexts of several devices may live in one thread
    c->lastTicks = ticks;
    if (c->numPixels == 0) {  // a rank whose tile is empty (more ranks than row bands): nothing to render
        if (c->resetTicksThisFrame) c->lastResetTick = ticks;
        c->resetTicksThisFrame = false;
        c->lastMs = 0.0f;
        return PTSS_OK;
    }

    selectImage(c);
    bool forkNeeded = false;
    if (c->resetTicksThisFrame) {  // CudaTracer.cu:602-608
        forkNeeded = true;
        c->lastResetTick = ticks;
        HIP_TRY(ptss::launchClear(st, frameBuffers(c, 0, pixels, 0)));
        c->resetTicksThisFrame = false;
    }
    const int sample = ticks - c->lastResetTick;
    const int K = (int)c->lanes.size();
    ptss::FrameBuffers fbs[ptss::kMaxLanes];
    for (int k = 0; k < K; ++k) fbs[k] = frameBuffers(c, k, pixels, sample);

    if (c->cfg.syncEachFrame) HIP_TRY(hipEventRecord(c->evStart, st));  // :611

    const int numIterations = c->usePathTracer ? (int)c->maxIterations : 1;  // :620
    ptss::EyeParams eye = eyeParams(c);
    // the shorter sphere candidate test: bounded geometry AND a camera within the same range (ray origins are the camera or points on primitives)
    const bool bounded = c->image().layout.sphereBounded != 0 && cameraInRange(c->camera);
    if (c->cameraDirty) {  // origin-only parts of the primary-ray tests (computeEyeRaysKernel :614 itself is fused into bounce 0)
        forkNeeded = true;
        HIP_TRY(ptss::launchPrimaryPrep(st, c->image().dBlob, c->image().layout, c->camera.position));
        // ... and which primitives each 64-pixel strip's eye rays can reach (csrc/ptstrip.h): the same inputs — this camera, this image
        // — and so the same trigger. Every call that changes either raises it: ptss_set_camera, selectImage, ptss_set_scene,
        // ptss_update_triangles, ptss_resort_triangles (ptss_reseed touches neither)
        c->stripsOn = ptstrip::eligible(c->image().layout, bounded);
        if (c->stripsOn) HIP_TRY(ptss::launchStripMasks(st, c->dStrips, c->capacity, c->numPixels, c->image().dBlob, c->image().layout, c->tile, eye));
        c->cameraDirty = false;
    }
    // only the bounce kernels' bounce 0 reads the words; the one-launch frame kernel (frames of a few tiles) visits everything
    if (c->stripsOn && !(c->image().oneLaunch && K == 1)) eye.strips = c->dStrips;
    c->stripsRead = eye.strips != nullptr;
    harvestHints(c);
    RC_TRY(forkLanes(c, forkNeeded));
    if (c->cfg.timeKernels) drainKernelEvents(c, false);
    RC_TRY(c->image().oneLaunch && K == 1 ? traceOneLaunch(c, fbs[0], numIterations, bounded, eye) : traceBounces(c, fbs, numIterations, bounded, eye));
    RC_TRY(flushAndJoin(c, fbs, numIterations));
    if (c->samples > 1) {
        HIP_TRY(ptss::launchDisplay(st, fbs[0]));  // S > 1: add the pass's staged samples, then the display value
        if (c->stagedTwice) HIP_TRY(hipEventRecord(c->evDisplay[c->frameIndex & 1u], st));
    }
    c->countParity ^= 1;
    c->frameIndex++;

    if (c->cfg.syncEachFrame) {  // :639-642
        HIP_TRY(hipEventRecord(c->evStop, st));
        HIP_TRY(hipEventSynchronize(c->evStop));
        HIP_TRY(hipEventElapsedTime(&c->lastMs, c->evStart, c->evStop));
        // (a 4-byte read-back per frame: only where several lanes wait for each other; a one-launch context is checked by
        // ptss_synchronize and the ptss_read_* calls — its frames are a third of a millisecond)
        return c->lanes.size() > 1 ? checkLaneTimeouts(c) : PTSS_OK;
    }
    return PTSS_OK;
}

int ptss_set_camera(ptss_context* c, const ptss_camera* camera) {
    if (!c || !camera) return fail(PTSS_EINVAL, "null argument");
    c->camera = *camera;
    c->cameraDirty = true;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_read_strip_words(ptss_context* c, unsigned long long* host_words, size_t capacity, size_t* count, int* enabled) {
    if (!c || !host_words || !count || !enabled) return fail(PTSS_EINVAL, "null argument");
    const size_t n = c->capacity / ptloc::kStrip;
    *count = n;
    if (capacity < n) return fail(PTSS_EINVAL, "host_words holds fewer words than the context has strips");
    const bool on = c->stripsRead && !c->cameraDirty;
    *enabled = on ? 1 : 0;
    if (!on) {
        for (size_t i = 0; i < n; ++i) host_words[i] = ptstrip::kAll;
        return PTSS_OK;
    }
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host_words, c->dStrips, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_get_camera(const ptss_context* c, ptss_camera* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->camera;
    return PTSS_OK;
}

int ptss_request_reset(ptss_context* c) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_set_mode(ptss_context* c, int usePathTracer) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->usePathTracer = usePathTracer != 0;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_set_max_iterations(ptss_context* c, unsigned int maxIterations) {
    if (!c || maxIterations == 0 || maxIterations > (unsigned)ptss::kMaxBounces)
        return fail(PTSS_EINVAL, "maxIterations must be in [1, 64]");
    c->maxIterations = maxIterations;
    return PTSS_OK;
}

int ptss_set_stream(ptss_context* c, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->stream = (hipStream_t)hipStream;
    return PTSS_OK;
}

int ptss_bind_accumulator(ptss_context* c, uint32_t* dev) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->dAccum = dev ? dev : c->dAccumOwned;
    return PTSS_OK;
}

int ptss_accumulator_devptr(ptss_context* c, uint32_t** out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->dAccum;
    return PTSS_OK;
}

int ptss_float_accumulator_devptr(ptss_context* c, float** out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->dFsum;
    return PTSS_OK;
}

int ptss_alloc_pixels(ptss_context* c, ptss_uchar4** out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMalloc(out, (size_t)c->capacity * sizeof(ptss_uchar4)));
    HIP_TRY(hipMemset(*out, 0, (size_t)c->capacity * sizeof(ptss_uchar4)));
    return PTSS_OK;
}

int ptss_free_pixels(ptss_context* c, ptss_uchar4* dev) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    HIP_TRY(hipFree(dev));
    return PTSS_OK;
}

int ptss_local_pixels(const ptss_context* c, size_t* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->numPixels;
    return PTSS_OK;
}

int ptss_local_rows(const ptss_context* c, int* rows, int cap, int* count) {
    if (!c || !count) return fail(PTSS_EINVAL, "null argument");
    int n = 0;
    for (int y = 0; y < c->tile.height; ++y) {
        if ((y / c->tile.bandRows) % c->tile.world != c->tile.rank) continue;
        if (rows) {
            if (n >= cap) return fail(PTSS_ERANGE, "rows[] too small");
            rows[n] = y;
        }
        ++n;
    }
    *count = n;
    return PTSS_OK;
}

int ptss_synchronize(ptss_context* c) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return checkLaneTimeouts(c);
}

int ptss_read_accumulator(ptss_context* c, uint32_t* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    if (count != (size_t)3 * c->numPixels) return fail(PTSS_ERANGE, "count must be 3 * local pixels");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host, c->dAccum, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return checkLaneTimeouts(c);
}

int ptss_read_float_accumulator(ptss_context* c, float* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    if (!c->dFsum) return fail(PTSS_EINVAL, "context was created without floatAccumulator");
    if (count != (size_t)3 * c->numPixels) return fail(PTSS_ERANGE, "count must be 3 * local pixels");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->samples == 1) {
        HIP_TRY(hipMemcpy(host, c->dFsum, count * sizeof(float), hipMemcpyDeviceToHost));
    } else {  // per-stream sums, added in lane order 0..S-1 (a fixed order: reproducible, and what the oracle does)
        std::vector<float> lane(count);
        for (size_t k = 0; k < count; ++k) host[k] = 0.0f;
        for (uint32_t l = 0; l < c->samples; ++l) {
            HIP_TRY(hipMemcpy(lane.data(), c->dFsum + (size_t)3 * l * c->capacity, count * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < count; ++k) host[k] = host[k] + lane[k];
        }
    }
    return checkLaneTimeouts(c);
}

int ptss_read_pixels(ptss_context* c, const ptss_uchar4* dev, ptss_uchar4* host, size_t count) {
    if (!c || !dev || !host) return fail(PTSS_EINVAL, "null argument");
    if (count > c->numPixels) return fail(PTSS_ERANGE, "count exceeds local pixels");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host, dev, count * sizeof(ptss_uchar4), hipMemcpyDeviceToHost));
    return checkLaneTimeouts(c);
}

int ptss_read_rng_state(ptss_context* c, size_t local_pixel, uint32_t* out6) { return ptss_read_rng_state_lane(c, local_pixel, 0, out6); }

int ptss_read_rng_state_lane(ptss_context* c, size_t local_pixel, unsigned int lane, uint32_t* out6) {
    if (!c || !out6) return fail(PTSS_EINVAL, "null argument");
    if (local_pixel >= c->numPixels || lane >= c->samples) return fail(PTSS_ERANGE, "pixel or lane out of range");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out6, c->dRngHome + (size_t)ptss::kHomeWords * ((size_t)lane * c->capacity + local_pixel), 6 * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_last_pass_ms(ptss_context* c, float* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->lastMs;
    return PTSS_OK;
}

int ptss_samples_since_reset(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->resetTicksThisFrame ? 0 : (c->lastTicks - c->lastResetTick + 1) * (int)c->samples;
    return PTSS_OK;
}

int ptss_live_counts(ptss_context* c, uint32_t* out, int cap, int* n) {
    if (!c || !out || !n) return fail(PTSS_EINVAL, "null argument");
    const int numIterations = c->usePathTracer ? (int)c->maxIterations : 1;
    if (cap < numIterations) return fail(PTSS_ERANGE, "out[] too small");
    std::vector<uint32_t> raw(ptss::kCountWords), sum(ptss::kCountWords, 0u);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Lane& ln : c->lanes) {  // the frame's count = its lanes' counts added up
        HIP_TRY(hipMemcpy(raw.data(), ln.dLastCounts, raw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < raw.size(); ++k) sum[k] += raw[k];
    }
    // a bounce whose input is <= 128 rays did not run (CudaTracer.cu:622): report 0 from there on
    bool stopped = false;
    for (int i = 0; i < numIterations; ++i) {
        uint32_t total = 0;
        for (int s = 0; s < ptss::kShards; ++s) total += sum[ptss::countIndex(i, s)];
        if (total <= (c->tile.world > 1 ? 0u : ptss::kMinLiveRays)) stopped = true;
        out[i] = stopped ? 0u : total;
    }
    *n = numIterations;
    return checkLaneTimeouts(c);
}

int ptss_total_ray_bounces(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long perLane[ptss::kMaxLanes];
    HIP_TRY(hipMemcpy(perLane, c->dTotal, sizeof(perLane), hipMemcpyDeviceToHost));
    *out = 0;
    for (size_t k = 0; k < c->lanes.size(); ++k) *out += perLane[k];
    return checkLaneTimeouts(c);
}

int ptss_guard_timeouts(ptss_context* c, unsigned int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, c->dTotal + ptss::kMaxLanes + 8, sizeof(v), hipMemcpyDeviceToHost));
    *out = v;
    return PTSS_OK;
}

int ptss_one_launch_frames(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = (c->image().oneLaunch && c->lanes.size() == 1) ? 1 : 0;
    return PTSS_OK;
}

int ptss_frame_lanes(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = (int)c->lanes.size();
    return PTSS_OK;
}

int ptss_launched_kernels(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->launchedKernels;
    return PTSS_OK;
}

int ptss_guard_flags(const ptss_context* c, unsigned int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->image().guardFlags;
    return PTSS_OK;
}

// the calls on the caller's stream (queries, features, film): counts and indices travel as 32-bit words, and a null stream is the context's
static inline bool fits31(unsigned long long v) { return v < (1ull << 31); }
static inline hipStream_t streamOf(const ptss_context* c, void* hipStream) { return hipStream ? static_cast<hipStream_t>(hipStream) : c->stream; }

// ptss_intersect / ptss_occluded: the context's own scene image (images[0]; the query kernel is exact on every image, so the
// camera's range plays no part), no frame state, the caller's stream
static int rayQuery(ptss_context* c, bool any, const ptss_ray_query* rays, void* out, size_t n, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (n == 0) return PTSS_OK;
    if (!rays || !out) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (((uintptr_t)rays | (uintptr_t)out) & (any ? 3u : 15u) || (uintptr_t)rays & 15u)
        return fail(PTSS_EINVAL, "rays and hits must be 16-byte aligned, verdicts 4-byte aligned");
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchQuery(st, any, im.dBlob, im.layout, im.inLds, rays, out, (uint32_t)n, c->gridCap * ptss::kShards,
                              &c->launchedKernels));
    return PTSS_OK;
}

int ptss_intersect(ptss_context* c, const ptss_ray_query* dev_rays, ptss_ray_hit* dev_hits, size_t n, void* hipStream) {
    return rayQuery(c, false, dev_rays, dev_hits, n, hipStream);
}

int ptss_occluded(ptss_context* c, const ptss_ray_query* dev_rays, uint32_t* dev_occluded, size_t n, void* hipStream) {
    return rayQuery(c, true, dev_rays, dev_occluded, n, hipStream);
}

// ptss_render_features: the scene image the queries use (images[0], exact for every camera), the context's CURRENT camera, no frame state
int ptss_render_features(ptss_context* c, ptss_pixel_feature* dev_features, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features) return fail(PTSS_EINVAL, "dev_features is null");
    if ((uintptr_t)dev_features & 15u) return fail(PTSS_EINVAL, "dev_features must be 16-byte aligned");
    if (c->numPixels == 0) return PTSS_OK;   // a rank whose tile is empty
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    HIP_TRY(ptss::launchFeatures(st, im.dBlob, im.layout, im.inLds, c->tile, eyeParams(c), defaultColor, dev_features, c->numPixels,
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
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    HIP_TRY(ptss::launchFeaturesMotion(st, im.dBlob, im.layout, im.inLds, c->tile, eyeParams(c), defaultColor, dev_features, c->numPixels,
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
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    HIP_TRY(ptss::launchFeaturesSpecular(st, im.dBlob, im.layout, im.inLds, c->tile, eyeParams(c), defaultColor, dev_features, dev_steps,
                                         c->numPixels, maxSteps, c->gridCap * ptss::kShards, c->specularFeatureLaunches));
    return PTSS_OK;
}

int ptss_specular_feature_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->specularFeatureLaunches[0];
    out2[1] = c->specularFeatureLaunches[1];
    return PTSS_OK;
}

// ptss_intersect_chain: ptss_intersect's image (images[0], exact for every ray), no frame state, the caller's stream; the chain of
// csrc/ptspecular.h behind every hit (ptss_chain.hip)
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
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    if (!(options && options->schedule == PTSS_CHAIN_REFILL)) {
        HIP_TRY(ptss::launchChain(st, im.dBlob, im.layout, im.inLds, dev_rays, dev_hits, dev_chain, (uint32_t)n, maxSteps, c->gridCap * ptss::kShards,
                                  &c->chainLaunches[0]));
        return PTSS_OK;
    }
    if (!c->dChainHead) HIP_TRY(hipMalloc(&c->dChainHead, 2 * sizeof(uint32_t)));   // (set in front of every kernel: nothing to clear)
    HIP_TRY(ptss::launchChainRefill(st, im.dBlob, im.layout, im.inLds, dev_rays, dev_hits, dev_chain, (uint32_t)n, maxSteps, options->maxWorkgroups,
                                    c->numCUs, c->dChainHead, &c->chainLaunches[1]));
    return PTSS_OK;
}

int ptss_chain_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->chainLaunches[0];
    out2[1] = c->chainLaunches[1];
    return PTSS_OK;
}

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

// ptss_trace_paths / ptss_trace_paths_opt: the queries' scene image (images[0], exact for every ray), the scene's guard flags and default
// colour, no frame state. options == nullptr: ptss_trace_paths itself
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
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    if (!refill) {
        HIP_TRY(ptss::launchPathQuery(st, im.dBlob, im.layout, im.inLds, dev_rays, dev_rng, dev_results, (uint32_t)n, (int)maxIterations, defaultColor,
                                      im.guardFlags, c->gridCap * ptss::kShards, c->pathLaunches));
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
    c->refillStream = st;
    HIP_TRY(ptss::launchPathRefill(st, im.dBlob, im.layout, im.inLds, dev_rays, dev_rng, dev_results, (uint32_t)n, (int)maxIterations, defaultColor,
                                   im.guardFlags, options->maxWorkgroups, c->numCUs, c->dPathRefill, c->refillLaunches));
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
    if (!c || !out5) return fail(PTSS_EINVAL, "null argument");
    out5[0] = c->refillLaunches[0];
    out5[1] = c->refillLaunches[1];
    out5[2] = out5[3] = out5[4] = 0;
    if (!c->dPathRefill) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->refillStream));
    HIP_TRY(hipMemcpy(out5 + 2, c->dPathRefill + 1, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_path_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->pathLaunches[0];
    out2[1] = c->pathLaunches[1];
    return PTSS_OK;
}

// ---- the film of a path query (ptss_film.hip). Like the queries: images[0] at most, no frame state, the caller's stream ----
// What the film calls share behind their own ctx and params checks, in the order each of them checks it: the film's size, n == 0 (nothing
// to do: PTSS_OK with go == false), the call's own verdict on its buffers (`badBuffers`: null first, then alignment; evaluated by the caller,
// reported here), n, firstPixel + n against the film where there is no index, the scene image where the call reads it, device and stream.
struct FilmCall {
    bool go = false;
    hipStream_t st = nullptr;
    uint32_t firstPixel = 0, n = 0, filmPixels = 0;   // firstPixel as the launch takes it: 0 with an index
    const float* quantTable = nullptr;                // the frame's own thresholds (frameBuffers); with a scene image only
};

static const float* quantTableOf(const SceneImage& im) { return reinterpret_cast<const float*>(im.dBlob + im.layout.offQuant); }

static int filmCall(ptss_context* c, FilmCall* f, unsigned long long filmPixels, const char* filmTooLarge, size_t n, const char* badBuffers,
                    const uint32_t* dev_index, size_t firstPixel, bool readsImage, void* hipStream) {
    if (!fits31(filmPixels)) return fail(PTSS_ERANGE, filmTooLarge);
    if (n == 0) return PTSS_OK;
    if (badBuffers) return fail(PTSS_EINVAL, badBuffers);
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (!dev_index && (firstPixel > filmPixels || n > filmPixels - firstPixel)) return fail(PTSS_ERANGE, "firstPixel + n leaves the film");
    const SceneImage& im = c->images[0];
    if (readsImage && !im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    *f = FilmCall{true, streamOf(c, hipStream), dev_index ? 0u : (uint32_t)firstPixel, (uint32_t)n, (uint32_t)filmPixels,
                  readsImage ? quantTableOf(im) : nullptr};
    return PTSS_OK;
}

// a launch with an index may count rejected entries: ptss_film_rejected synchronises on its stream
static void noteFilmIndex(ptss_context* c, const uint32_t* dev_index, hipStream_t st) {
    if (dev_index) {
        c->filmStream = st;
        c->filmIndexed = true;
    }
}

static const char* const kNullBuffer = "null buffer with n > 0";

int ptss_generate_rays(ptss_context* c, const ptss_film_camera* film, size_t firstPixel, const uint32_t* dev_index, size_t n, ptss_path_rng* dev_rng,
                       ptss_ray_query* dev_rays, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptcam::cameraError(film)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_rng || !dev_rays ? kNullBuffer
                      : ((uintptr_t)dev_rays & 15u) || (((uintptr_t)dev_rng | (uintptr_t)dev_index) & 3u)
                          ? "rays must be 16-byte aligned, dev_rng and dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, (unsigned long long)film->width * (unsigned long long)film->height, "width * height must be below 2^31", n, bad, dev_index,
                    firstPixel, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchFilmRays(f.st, ptcam::filmOf(*film), f.firstPixel, dev_index, f.n, dev_rng, dev_rays, nullptr,
                                 c->dTotal + kFilmRejectedWord, &c->filmLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_accumulate_paths(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                          ptss_film_entry* dev_film, size_t filmPixels, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    const char* bad = !dev_results || !dev_film ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film | (uintptr_t)dev_history) & 15u) ||
                              (((uintptr_t)dev_index | (uintptr_t)dev_pixels) & 3u)
                          ? "results, film and history must be 16-byte aligned, dev_index and dev_pixels 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchFilmAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, f.filmPixels, dev_pixels, dev_history, f.quantTable,
                                       c->dTotal + kFilmRejectedWord, &c->filmLaunches[1]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_ray_features(ptss_context* c, const ptss_ray_query* dev_rays, ptss_pixel_feature* dev_features, size_t n, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (n == 0) return PTSS_OK;
    if (!dev_rays || !dev_features) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if (((uintptr_t)dev_rays | (uintptr_t)dev_features) & 15u) return fail(PTSS_EINVAL, "rays and features must be 16-byte aligned");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    HIP_TRY(ptss::launchRayFeatures(st, im.dBlob, im.layout, im.inLds, dev_rays, defaultColor, dev_features, (uint32_t)n, c->gridCap * ptss::kShards,
                                    &c->filmLaunches[2]));
    return PTSS_OK;
}

int ptss_film_launches(const ptss_context* c, unsigned long long* out3) {
    if (!c || !out3) return fail(PTSS_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k) out3[k] = c->filmLaunches[k];
    return PTSS_OK;
}

int ptss_film_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->filmIndexed) HIP_TRY(hipStreamSynchronize(c->filmStream));
    HIP_TRY(hipMemcpy(out, c->dTotal + kFilmRejectedWord, sizeof(*out), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

// ---- adaptive film sampling (ptss_adaptive.hip; csrc/ptadaptive.h). Like the film calls: no frame state, the caller's stream ----
int ptss_accumulate_paths_stats(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                                ptss_film_entry* dev_film, unsigned long long* dev_moments, size_t filmPixels, ptss_uchar4* dev_pixels,
                                ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    const char* bad = !dev_results || !dev_film || !dev_moments ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film | (uintptr_t)dev_history) & 15u) ||
                              (((uintptr_t)dev_index | (uintptr_t)dev_pixels) & 3u) || ((uintptr_t)dev_moments & 7u)
                          ? "results, film and history must be 16-byte aligned, dev_moments 8-byte, dev_index and dev_pixels 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchStatsAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, dev_moments, f.filmPixels, dev_pixels, dev_history,
                                        f.quantTable, c->dTotal + kFilmRejectedWord, &c->adaptiveLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_default_plan_params(ptss_plan_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_plan_params);
    p->minSamples = 8u;
    p->maxSamples = ptad::kSampleLimit;
    p->threshold = 0.5f;
    return PTSS_OK;
}

int ptss_plan_cdf_entries(size_t filmPixels, size_t* entries) {
    if (!entries) return fail(PTSS_EINVAL, "entries is null");
    if (filmPixels == 0 || !fits31(filmPixels)) return fail(PTSS_ERANGE, "filmPixels must be in [1, 2^31)");
    *entries = (size_t)ptad::cdfEntries(filmPixels);
    return PTSS_OK;
}

// What the two plan calls share behind their own ctx and params checks, in this order: the film's size, n, n == 0 (nothing to do: PTSS_OK
// with go == false), the call's own verdict on its buffers (FilmCall's `badBuffers`), device and stream. FilmCall's firstPixel stays 0
static int planCall(ptss_context* c, FilmCall* f, size_t filmPixels, size_t n, const char* badBuffers, void* hipStream) {
    if (filmPixels == 0 || !fits31(filmPixels)) return fail(PTSS_ERANGE, "filmPixels must be in [1, 2^31)");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (badBuffers) return fail(PTSS_EINVAL, badBuffers);
    HIP_TRY(hipSetDevice(c->cfg.device));
    *f = FilmCall{true, streamOf(c, hipStream), 0u, (uint32_t)n, (uint32_t)filmPixels, nullptr};
    return PTSS_OK;
}

int ptss_plan_samples(ptss_context* c, const ptss_film_entry* dev_film, const unsigned long long* dev_moments, size_t filmPixels,
                      const ptss_plan_params* params, size_t n, unsigned long long* dev_cdf, uint32_t* dev_index, ptss_plan_info* dev_info,
                      void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptad::paramsError(params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_film || !dev_moments || !dev_cdf || !dev_index ? kNullBuffer
                      : ((uintptr_t)dev_film & 15u) || (((uintptr_t)dev_moments | (uintptr_t)dev_cdf | (uintptr_t)dev_info) & 7u) || ((uintptr_t)dev_index & 3u)
                          ? "film must be 16-byte aligned, dev_moments, dev_cdf and dev_info 8-byte, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(planCall(c, &f, filmPixels, n, bad, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchPlanSamples(f.st, dev_film, dev_moments, f.filmPixels, *params, f.n, dev_cdf, dev_index, dev_info, &c->adaptiveLaunches[1]));
    return PTSS_OK;
}

int ptss_adaptive_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->adaptiveLaunches[0];
    out2[1] = c->adaptiveLaunches[1];
    return PTSS_OK;
}

// ---- the linear film (ptss_linear.hip; csrc/ptlinear.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_linear_params(ptss_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_linear_params);
    p->scaleLog2 = 20;
    p->clampMax = 65536.f;
    p->exposure = 1.f;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_accumulate_paths_linear(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                                 ptss_linear_entry* dev_film, size_t filmPixels, const ptss_linear_params* params, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_results || !dev_film ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film) & 15u) || ((uintptr_t)dev_index & 3u)
                          ? "results and film must be 16-byte aligned, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchLinearAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, nullptr, f.filmPixels, *params,
                                         c->dTotal + kFilmRejectedWord, &c->linearLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_linear_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->linearLaunches[0];
    out2[1] = c->linearLaunches[1];
    return PTSS_OK;
}

// ---- adaptive sampling on the linear film (ptss_linear.hip, ptss_adaptive.hip; csrc/ptlinstats.h). Like the film calls:
// no frame state, the caller's stream ----
int ptss_default_linear_plan_params(ptss_linear_plan_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_linear_plan_params);
    p->minSamples = 8u;
    p->maxSamples = ptad::kSampleLimit;
    p->threshold = 0.02f;
    p->floor = 0.015625f;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0u;
    return PTSS_OK;
}

int ptss_accumulate_paths_linear_stats(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                                       ptss_linear_entry* dev_film, ptss_linear_moment* dev_moments, size_t filmPixels,
                                       const ptss_linear_params* params, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_results || !dev_moments ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film | (uintptr_t)dev_moments) & 15u) || ((uintptr_t)dev_index & 3u)
                          ? "results, film and moments must be 16-byte aligned, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchLinearAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, dev_moments, f.filmPixels, *params,
                                         c->dTotal + kFilmRejectedWord, &c->linStatsLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_plan_samples_linear(ptss_context* c, const ptss_linear_moment* dev_moments, size_t filmPixels, const ptss_linear_params* params,
                             const ptss_linear_plan_params* plan, size_t n, unsigned long long* dev_cdf, uint32_t* dev_index,
                             ptss_plan_info* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptls::paramsError(plan, params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_moments || !dev_cdf || !dev_index ? kNullBuffer
                      : ((uintptr_t)dev_moments & 15u) || (((uintptr_t)dev_cdf | (uintptr_t)dev_info) & 7u) || ((uintptr_t)dev_index & 3u)
                          ? "moments must be 16-byte aligned, dev_cdf and dev_info 8-byte, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(planCall(c, &f, filmPixels, n, bad, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchPlanSamplesLinear(f.st, dev_moments, f.filmPixels, *params, *plan, f.n, dev_cdf, dev_index, dev_info, &c->linStatsLaunches[1]));
    return PTSS_OK;
}

int ptss_linear_stats_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->linStatsLaunches[0];
    out2[1] = c->linStatsLaunches[1];
    return PTSS_OK;
}

// ---- the filtered linear film (ptss_splat.hip; csrc/ptsplat.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_splat_filter(ptss_splat_filter* f) {
    if (!f) return fail(PTSS_EINVAL, "filter is null");
    f->structSize = (unsigned int)sizeof(ptss_splat_filter);
    f->kind = PTSS_SPLAT_TENT;
    f->radius = 1.f;
    f->alpha = 2.f;
    f->reserved = 0u;
    return PTSS_OK;
}

int ptss_generate_rays_positions(ptss_context* c, const ptss_film_camera* film, size_t firstPixel, const uint32_t* dev_index, size_t n,
                                 ptss_path_rng* dev_rng, ptss_ray_query* dev_rays, ptss_film_position* dev_positions, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptcam::cameraError(film)) return fail(PTSS_EINVAL, what);
    if (!dev_positions) return fail(PTSS_EINVAL, "dev_positions is null (ptss_generate_rays makes rays without positions)");
    const char* bad = !dev_rng || !dev_rays ? kNullBuffer
                      : ((uintptr_t)dev_rays & 15u) || ((uintptr_t)dev_positions & 7u) || (((uintptr_t)dev_rng | (uintptr_t)dev_index) & 3u)
                          ? "rays must be 16-byte aligned, dev_positions 8-byte, dev_rng and dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, (unsigned long long)film->width * (unsigned long long)film->height, "width * height must be below 2^31", n, bad, dev_index,
                    firstPixel, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchFilmRays(f.st, ptcam::filmOf(*film), f.firstPixel, dev_index, f.n, dev_rng, dev_rays, dev_positions,
                                 c->dTotal + kFilmRejectedWord, &c->filmLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

// what the two splat calls check in front of filmCall: ctx, filter, params, the film's sides
static int splatArguments(const ptss_context* c, const ptss_splat_filter* filter, const ptss_linear_params* params, int width, int height) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptspl::filterError(filter)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (width < 1 || height < 1 || width > ptspl::kMaxFilmSide || height > ptspl::kMaxFilmSide)
        return fail(PTSS_ERANGE, "width and height must be in [1, 2^22]");
    return PTSS_OK;
}

static const char* splatBuffersError(const ptss_path_result* dev_results, const ptss_film_position* dev_positions, const ptss_splat_entry* dev_film) {
    return !dev_results || !dev_positions || !dev_film ? kNullBuffer
           : (((uintptr_t)dev_results | (uintptr_t)dev_film) & 15u) || ((uintptr_t)dev_positions & 7u)
               ? "results and film must be 16-byte aligned, dev_positions 8-byte aligned"
               : nullptr;
}

// the device counters of a splat: ptss_splat_stats synchronises on the stream of the latest one
static void noteSplat(ptss_context* c, hipStream_t st) {
    c->splatStream = st;
    c->splatCounted = true;
}

int ptss_splat_paths(ptss_context* c, const ptss_path_result* dev_results, const ptss_film_position* dev_positions, size_t n,
                     ptss_splat_entry* dev_film, int width, int height, const ptss_splat_filter* filter, const ptss_linear_params* params,
                     void* hipStream) {
    RC_TRY(splatArguments(c, filter, params, width, height));
    FilmCall f;   // (positions take the place of an index: n is not bound by the film)
    RC_TRY(filmCall(c, &f, (unsigned long long)width * (unsigned long long)height, "width * height must be below 2^31", n,
                    splatBuffersError(dev_results, dev_positions, dev_film), reinterpret_cast<const uint32_t*>(dev_positions), 0, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchSplatScatter(f.st, dev_results, dev_positions, f.n, dev_film, width, height, *filter, *params, c->dTotal + kSplatCountersWord,
                                     &c->splatLaunches[0]));
    noteSplat(c, f.st);
    return PTSS_OK;
}

int ptss_splat_paths_homed(ptss_context* c, const ptss_path_result* dev_results, const ptss_film_position* dev_positions, size_t firstPixel, size_t n,
                           ptss_splat_entry* dev_film, int width, int height, const ptss_splat_filter* filter, const ptss_linear_params* params,
                           void* hipStream) {
    RC_TRY(splatArguments(c, filter, params, width, height));
    FilmCall f;
    RC_TRY(filmCall(c, &f, (unsigned long long)width * (unsigned long long)height, "width * height must be below 2^31", n,
                    splatBuffersError(dev_results, dev_positions, dev_film), nullptr, firstPixel, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchSplatHomed(f.st, dev_results, dev_positions, f.firstPixel, f.n, dev_film, width, height, *filter, *params,
                                   c->dTotal + kSplatCountersWord, &c->splatLaunches[1]));
    noteSplat(c, f.st);
    return PTSS_OK;
}

int ptss_splat_stats(ptss_context* c, unsigned long long* out5) {
    if (!c || !out5) return fail(PTSS_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k) out5[k] = c->splatLaunches[k];
    out5[3] = out5[4] = 0;
    if (!c->splatCounted) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->splatStream));
    HIP_TRY(hipMemcpy(out5 + 3, c->dTotal + kSplatCountersWord, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

// ---- the meter of the two linear films (ptss_meter.hip; csrc/ptmeter.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_meter_params(ptss_meter_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_meter_params);
    p->key = 0.18f;
    p->lowPermille = 100u;
    p->highPermille = 20u;
    p->rate = 1.f;
    p->minExposure = 1.f / 65536.f;
    p->maxExposure = 65536.f;
    p->reserved = 0u;
    return PTSS_OK;
}

// What the calls over a range of a film share behind their own ctx and params checks, in ptss_resolve_linear's order: count == 0 (nothing
// to do: PTSS_OK with go == false), the call's own verdict on its buffers (FilmCall's `badBuffers`), the range, the scene image where the
// call reads it, `writes` (a call none of whose outputs is there has nothing to do either, and does not touch the device), device and
// stream. FilmCall's firstPixel and n are the range; filmPixels stays 0
static int rangeCall(ptss_context* c, FilmCall* f, size_t firstPixel, size_t count, const char* badBuffers, bool readsImage, bool writes,
                     void* hipStream) {
    if (count == 0) return PTSS_OK;
    if (badBuffers) return fail(PTSS_EINVAL, badBuffers);
    if (!fits31(firstPixel) || !fits31(count) || !fits31(firstPixel + count)) return fail(PTSS_ERANGE, "firstPixel + count must be below 2^31");
    const SceneImage& im = c->images[0];
    if (readsImage && !im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    if (!writes) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    *f = FilmCall{true, streamOf(c, hipStream), (uint32_t)firstPixel, (uint32_t)count, 0u, readsImage ? quantTableOf(im) : nullptr};
    return PTSS_OK;
}

static int meterFilm(ptss_context* c, const void* dev_film, bool splat, size_t firstPixel, size_t count, uint32_t* dev_histogram, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    const char* bad = !dev_film || !dev_histogram ? "null film or histogram with count > 0"
                      : ((uintptr_t)dev_film & 15u) || ((uintptr_t)dev_histogram & 3u) ? "film must be 16-byte aligned, dev_histogram 4-byte aligned"
                                                                                         : nullptr;
    FilmCall f;
    RC_TRY(rangeCall(c, &f, firstPixel, count, bad, false, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchMeterHistogram(f.st, dev_film, splat, f.firstPixel, f.n, dev_histogram, &c->meterLaunches[0]));
    return PTSS_OK;
}

int ptss_meter_linear(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, uint32_t* dev_histogram, void* hipStream) {
    return meterFilm(c, dev_film, false, firstPixel, count, dev_histogram, hipStream);
}

int ptss_meter_splat(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, uint32_t* dev_histogram, void* hipStream) {
    return meterFilm(c, dev_film, true, firstPixel, count, dev_histogram, hipStream);
}

int ptss_meter_exposure(ptss_context* c, const uint32_t* dev_histogram, const ptss_linear_params* params, const ptss_meter_params* meter,
                        ptss_meter_state* dev_state, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptmeter::paramsError(meter)) return fail(PTSS_EINVAL, what);
    if (!dev_histogram || !dev_state) return fail(PTSS_EINVAL, "null histogram or state");
    if (((uintptr_t)dev_histogram & 3u) || ((uintptr_t)dev_state & 7u)) return fail(PTSS_EINVAL, "dev_histogram must be 4-byte aligned, dev_state 8-byte aligned");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchMeterExposure(streamOf(c, hipStream), dev_histogram, *params, *meter, dev_state, &c->meterLaunches[1]));
    return PTSS_OK;
}

int ptss_meter_launches(const ptss_context* c, unsigned long long* out3) {
    if (!c || !out3) return fail(PTSS_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k) out3[k] = c->meterLaunches[k];
    return PTSS_OK;
}

// ---- glare for the two linear films (ptss_glare.hip; csrc/ptglare.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_glare_params(ptss_glare_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_glare_params);
    p->levels = 6;
    p->mode = PTSS_GLARE_MIX;
    p->threshold = 0.f;
    p->strength = 0.1f;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_glare_layout(int width, int height, int levels, ptss_glare_level out[8], size_t* entries) {
    if (!out || !entries) return fail(PTSS_EINVAL, "null argument");
    if (levels < 1 || levels > ptglare::kMaxLevels) return fail(PTSS_EINVAL, "levels must be in [1, 8]");
    if (const char* what = ptglare::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    *entries = ptglare::layoutOf(width, height, levels, out);
    return PTSS_OK;
}

// what the glare calls check first: ctx, the film's parameters, the glare's, the film's kind and its sides
static int glareArguments(const ptss_context* c, const ptss_linear_params* params, const ptss_glare_params* glare, int filmKind, int width, int height) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptglare::paramsError(glare, *params)) return fail(PTSS_EINVAL, what);
    if (filmKind != PTSS_GLARE_FILM_LINEAR && filmKind != PTSS_GLARE_FILM_SPLAT) return fail(PTSS_EINVAL, "unknown film kind");
    if (const char* what = ptglare::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    return PTSS_OK;
}

int ptss_glare_build(ptss_context* c, const void* dev_film, int filmKind, int width, int height, const ptss_linear_params* params,
                     const ptss_glare_params* glare, ptss_glare_entry* dev_pyramid, void* hipStream) {
    RC_TRY(glareArguments(c, params, glare, filmKind, width, height));
    if (!dev_film || !dev_pyramid) return fail(PTSS_EINVAL, "null film or pyramid");
    if (((uintptr_t)dev_film | (uintptr_t)dev_pyramid) & 15u) return fail(PTSS_EINVAL, "film and pyramid must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchGlareBuild(streamOf(c, hipStream), dev_film, filmKind == PTSS_GLARE_FILM_SPLAT, width, height, *params, *glare, dev_pyramid,
                                   c->glareLaunches));
    return PTSS_OK;
}

int ptss_glare_launches(const ptss_context* c, unsigned long long* out3) {
    if (!c || !out3) return fail(PTSS_EINVAL, "null argument");
    for (int k = 0; k < 3; ++k) out3[k] = c->glareLaunches[k];
    return PTSS_OK;
}

// ---- the denoiser of the two linear films (ptss_lindenoise.hip; csrc/ptlindn.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_denoise_linear_params(ptss_denoise_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_denoise_linear_params);
    p->levels = 5;
    p->sigmaLuminance = 3.f;   // design choices, not measurements: three standard errors, and ptss_default_denoise_params' geometry
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.f;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0u;
    return PTSS_OK;
}

int ptss_denoise_linear_workspace(int width, int height, size_t* bytes) {
    if (!bytes) return fail(PTSS_EINVAL, "bytes is null");
    if (const char* what = ptldn::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    size_t off[4];
    *bytes = ptldn::workspaceLayout((size_t)width * (size_t)height, off);
    return PTSS_OK;
}

int ptss_denoise_linear(ptss_context* c, const void* dev_film, int filmKind, int width, int height, const ptss_linear_moment* dev_moments,
                        const ptss_pixel_feature* dev_features, const ptss_linear_params* params, const ptss_denoise_linear_params* denoise,
                        void* dev_workspace, ptss_linear_entry* dev_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptldn::paramsError(denoise)) return fail(PTSS_EINVAL, what);
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return fail(PTSS_EINVAL, "unknown film kind");
    if (const char* what = ptldn::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    if (!dev_film || !dev_moments || !dev_features || !dev_workspace || !dev_out) return fail(PTSS_EINVAL, "null film, moments, features, workspace or out");
    if (((uintptr_t)dev_film | (uintptr_t)dev_moments | (uintptr_t)dev_features | (uintptr_t)dev_workspace | (uintptr_t)dev_out) & 15u)
        return fail(PTSS_EINVAL, "film, moments, features, workspace and out must be 16-byte aligned");
    if ((const void*)dev_out == dev_film) return fail(PTSS_EINVAL, "dev_out must not be dev_film");
    size_t off[4];
    const size_t bytes = ptldn::workspaceLayout((size_t)width * (size_t)height, off);
    const uintptr_t ws = (uintptr_t)dev_workspace;
    if (((uintptr_t)dev_out >= ws && (uintptr_t)dev_out - ws < bytes) || ((uintptr_t)dev_film >= ws && (uintptr_t)dev_film - ws < bytes))
        return fail(PTSS_EINVAL, "film and out must not lie inside the workspace");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLinearDenoise(streamOf(c, hipStream), dev_film, filmKind == PTSS_FILM_SPLAT, width, height, dev_moments, dev_features, *params,
                                      *denoise, c->linDenoiseForm, dev_workspace, dev_out, c->linDenoiseLaunches));
    return PTSS_OK;
}

int ptss_denoise_linear_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->linDenoiseLaunches[0];
    out2[1] = c->linDenoiseLaunches[1];
    return PTSS_OK;
}

int ptss_debug_denoise_linear_form(ptss_context* c, int form) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (form < 0 || form == 3 || form > 11) return fail(PTSS_EINVAL, "form must be 0, 1, 2 or 4 .. 11");
    c->linDenoiseForm = form;
    return PTSS_OK;
}

// ---- carrying the two linear films across a camera move (ptss_linreproject.hip; csrc/ptlinrp.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_reproject_linear_params(ptss_reproject_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_reproject_linear_params);
    p->cosNormal = 0.9f;   // ptss_default_reproject_params' tests; a cap of 64 samples of history (design choices, not measurements)
    p->depthTolerance = 0.02f;
    p->minCoverage = 0.25f;
    p->maxHistory = 64u;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_reproject_linear(ptss_context* c, const ptss_film_camera* now, const ptss_pixel_feature* dev_features_now,
                          const ptss_pixel_motion* dev_motion_now, const ptss_film_camera* prev, const ptss_pixel_feature* dev_features_prev,
                          const void* dev_film_prev, int filmKind, const ptss_linear_moment* dev_moments_prev, const ptss_linear_params* film,
                          const ptss_reproject_linear_params* params, void* dev_film_out, ptss_linear_moment* dev_moments_out,
                          ptss_reproject_linear_info* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    // in the order of the header's list: null pointers, structSize and parameter ranges, the cameras, the film's parameters, the kind,
    // moments on one side only, alignment, overlap
    if (!now || !prev || !film || !params || !dev_features_now || !dev_features_prev || !dev_film_prev || !dev_film_out)
        return fail(PTSS_EINVAL, "null camera, parameters, features, previous film or output film");
    if (const char* what = ptlrp::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlrp::cameraError(now)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlrp::cameraError(prev)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return fail(PTSS_EINVAL, "unknown film kind");
    if ((dev_moments_prev == nullptr) != (dev_moments_out == nullptr))
        return fail(PTSS_EINVAL, "dev_moments_prev and dev_moments_out must be given together or not at all");
    if (((uintptr_t)dev_features_now | (uintptr_t)dev_motion_now | (uintptr_t)dev_features_prev | (uintptr_t)dev_film_prev | (uintptr_t)dev_moments_prev |
         (uintptr_t)dev_film_out | (uintptr_t)dev_moments_out) & 15u)
        return fail(PTSS_EINVAL, "features, motion, films and moments must be 16-byte aligned");
    if ((uintptr_t)dev_info & 7u) return fail(PTSS_EINVAL, "dev_info must be 8-byte aligned");
    if (const char* what = ptlrp::buffersError(now, dev_features_now, prev, dev_features_prev, dev_film_prev, dev_moments_prev, dev_film_out, dev_moments_out))
        return fail(PTSS_EINVAL, what);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLinearReproject(streamOf(c, hipStream), *now, dev_features_now, dev_motion_now, *prev, dev_features_prev, dev_film_prev,
                                        filmKind == PTSS_FILM_SPLAT, dev_moments_prev, *film, *params, dev_film_out, dev_moments_out, dev_info,
                                        &c->linReprojectLaunches));
    return PTSS_OK;
}

int ptss_reproject_linear_launches(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->linReprojectLaunches;
    return PTSS_OK;
}

// ---- upsampling the two linear films (ptss_linupsample.hip; csrc/ptlinup.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_upsample_linear_params(ptss_upsample_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_upsample_linear_params);
    p->factor = 2;   // ptss_default_upsample_params' values (design choices, not measurements)
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.0f;
    p->flags = 0u;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_upsample_linear(ptss_context* c, const void* dev_film_lo, int filmKind, int width, int height, const ptss_pixel_feature* dev_features_lo,
                         const ptss_pixel_feature* dev_features_hi, const ptss_linear_params* film, const ptss_upsample_linear_params* params,
                         ptss_linear_entry* dev_film_hi, ptss_upsample_linear_info* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    // in the order of the header's list: null pointers, the parameters, the kind, the film's parameters, the sides, alignment, overlap
    if (!film || !params || !dev_film_lo || !dev_features_lo || !dev_features_hi || !dev_film_hi)
        return fail(PTSS_EINVAL, "null parameters, film, features or output film");
    if (const char* what = ptlup::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return fail(PTSS_EINVAL, "unknown film kind");
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlup::sidesError(width, height, params->factor)) return fail(PTSS_ERANGE, what);
    if (((uintptr_t)dev_film_lo | (uintptr_t)dev_features_lo | (uintptr_t)dev_features_hi | (uintptr_t)dev_film_hi) & 15u)
        return fail(PTSS_EINVAL, "films and features must be 16-byte aligned");
    if ((uintptr_t)dev_info & 7u) return fail(PTSS_EINVAL, "dev_info must be 8-byte aligned");
    const size_t loBytes = 32 * (size_t)width * (size_t)height, hiBytes = loBytes * (size_t)params->factor * (size_t)params->factor;
    if (ptlup::rangesOverlap(dev_film_hi, hiBytes, dev_film_lo, loBytes)) return fail(PTSS_EINVAL, "dev_film_hi overlaps dev_film_lo");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLinearUpsample(streamOf(c, hipStream), dev_film_lo, filmKind == PTSS_FILM_SPLAT, width, height, dev_features_lo, dev_features_hi,
                                       *film, *params, c->linUpsampleForm, dev_film_hi, dev_info, &c->linUpsampleLaunches));
    return PTSS_OK;
}

int ptss_upsample_linear_launches(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->linUpsampleLaunches;
    return PTSS_OK;
}

int ptss_debug_upsample_linear_form(ptss_context* c, int form) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (form < 0 || form > 2) return fail(PTSS_EINVAL, "form must be 0, 1 or 2");
    c->linUpsampleForm = form;
    return PTSS_OK;
}

// ---- rays from surface points and the gutter fill (ptss_surface.hip; csrc/ptsurface.h). Like the film calls: images[0] at most, no frame state, the caller's stream ----
int ptss_generate_rays_surface(ptss_context* c, const ptss_surface_params* params, const ptss_surface_point* dev_points, size_t numPoints,
                               size_t firstPoint, const uint32_t* dev_index, size_t n, ptss_path_rng* dev_rng, ptss_ray_query* dev_rays,
                               ptss_ray_hit* dev_surfels, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptsurf::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (!fits31(numPoints)) return fail(PTSS_ERANGE, "numPoints must be below 2^31");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (!dev_points || !dev_rng || !dev_rays) return fail(PTSS_EINVAL, kNullBuffer);
    if ((((uintptr_t)dev_points | (uintptr_t)dev_rays | (uintptr_t)dev_surfels) & 15u) || (((uintptr_t)dev_rng | (uintptr_t)dev_index) & 3u))
        return fail(PTSS_EINVAL, "points, rays and surfels must be 16-byte aligned, dev_rng and dev_index 4-byte aligned");
    if (!dev_index && (firstPoint > numPoints || n > numPoints - firstPoint)) return fail(PTSS_ERANGE, "firstPoint + n leaves the points");
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchSurfaceRays(st, im.dBlob, im.layout, *params, dev_points, (uint32_t)numPoints, dev_index ? 0u : (uint32_t)firstPoint, dev_index,
                                    (uint32_t)n, dev_rng, dev_rays, dev_surfels, c->dTotal + kSurfaceRejectedWord, &c->surfaceLaunches[0]));
    c->surfaceStream = st;
    c->surfaceCounted = true;
    return PTSS_OK;
}

int ptss_dilate_linear(ptss_context* c, const ptss_linear_entry* dev_film, int width, int height, ptss_linear_entry* dev_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_film || !dev_out) return fail(PTSS_EINVAL, "null film");
    if (dev_film == dev_out) return fail(PTSS_EINVAL, "dev_out must not be dev_film");
    if (((uintptr_t)dev_film | (uintptr_t)dev_out) & 15u) return fail(PTSS_EINVAL, "films must be 16-byte aligned");
    if (const char* what = ptsurf::dilateSidesError(width, height)) return fail(PTSS_ERANGE, what);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchDilateLinear(streamOf(c, hipStream), dev_film, width, height, c->dilateForm, dev_out, &c->surfaceLaunches[1]));
    return PTSS_OK;
}

int ptss_surface_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    for (int k = 0; k < 2; ++k) out2[k] = c->surfaceLaunches[k];
    return PTSS_OK;
}

int ptss_surface_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->surfaceCounted) HIP_TRY(hipStreamSynchronize(c->surfaceStream));
    HIP_TRY(hipMemcpy(out, c->dTotal + kSurfaceRejectedWord, sizeof(*out), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_debug_dilate_linear_form(ptss_context* c, int form) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (form < 0 || form > 2) return fail(PTSS_EINVAL, "form must be 0, 1 or 2");
    c->dilateForm = form;
    return PTSS_OK;
}

// ---- reading a baked light map back (ptss_lightmap.hip; csrc/ptlightmap.h). images[0]'s materials at most, no frame state, the caller's stream ----
int ptss_default_lightmap_params(ptss_lightmap_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    *p = ptss_lightmap_params{};
    p->structSize = (unsigned int)sizeof(*p);
    p->atlasWidth = p->atlasHeight = 1;
    p->filter = PTSS_LIGHTMAP_BILINEAR;
    return PTSS_OK;
}

int ptss_lookup_lightmap(ptss_context* c, const ptss_lightmap_params* params, const ptss_linear_params* film, const ptss_surface_block* dev_blocksTri,
                         const ptss_surface_block* dev_blocksSph, const ptss_linear_entry* dev_map, const ptss_ray_hit* dev_hits, size_t n,
                         ptss_linear_entry* dev_out, uint32_t* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlm::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlm::rangeError(params)) return fail(PTSS_ERANGE, what);
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (!dev_map || !dev_hits || !dev_out || (params->numTriangleBlocks > 0 && !dev_blocksTri) || (params->numSphereBlocks > 0 && !dev_blocksSph))
        return fail(PTSS_EINVAL, kNullBuffer);
    if ((((uintptr_t)dev_blocksTri | (uintptr_t)dev_blocksSph | (uintptr_t)dev_map | (uintptr_t)dev_hits | (uintptr_t)dev_out) & 15u) ||
        ((uintptr_t)dev_info & 3u))
        return fail(PTSS_EINVAL, "blocks, map, hits and out must be 16-byte aligned, dev_info 4-byte aligned");
    if (ptlrp::rangesOverlap(dev_out, 32 * n, dev_map, 32 * (size_t)params->atlasWidth * (size_t)params->atlasHeight))
        return fail(PTSS_EINVAL, "dev_out overlaps dev_map");
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLookupLightmap(streamOf(c, hipStream), im.dBlob, im.layout, *params, *film, dev_blocksTri, dev_blocksSph, dev_map, dev_hits,
                                       (uint32_t)n, c->lightmapForm, dev_out, dev_info, &c->lightmapLaunches));
    return PTSS_OK;
}

// ptss_lookup_lightmap's checks and one more buffer: the chain rows whose throughput tints the FILTERED rows (ptlightmap.h step 6)
int ptss_lookup_lightmap_chain(ptss_context* c, const ptss_lightmap_params* params, const ptss_linear_params* film,
                               const ptss_surface_block* dev_blocksTri, const ptss_surface_block* dev_blocksSph, const ptss_linear_entry* dev_map,
                               const ptss_ray_hit* dev_hits, const ptss_chain_result* dev_chain, size_t n, ptss_linear_entry* dev_out,
                               uint32_t* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlm::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlm::rangeError(params)) return fail(PTSS_ERANGE, what);
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (!dev_map || !dev_hits || !dev_chain || !dev_out || (params->numTriangleBlocks > 0 && !dev_blocksTri) ||
        (params->numSphereBlocks > 0 && !dev_blocksSph))
        return fail(PTSS_EINVAL, kNullBuffer);
    if ((((uintptr_t)dev_blocksTri | (uintptr_t)dev_blocksSph | (uintptr_t)dev_map | (uintptr_t)dev_hits | (uintptr_t)dev_chain | (uintptr_t)dev_out) & 15u) ||
        ((uintptr_t)dev_info & 3u))
        return fail(PTSS_EINVAL, "blocks, map, hits, chain and out must be 16-byte aligned, dev_info 4-byte aligned");
    if (ptlrp::rangesOverlap(dev_out, 32 * n, dev_map, 32 * (size_t)params->atlasWidth * (size_t)params->atlasHeight))
        return fail(PTSS_EINVAL, "dev_out overlaps dev_map");
    if (ptlrp::rangesOverlap(dev_out, 32 * n, dev_chain, 32 * n) || ptlrp::rangesOverlap(dev_out, 32 * n, dev_hits, 48 * n))
        return fail(PTSS_EINVAL, "dev_out overlaps dev_chain or dev_hits");
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLookupLightmapChain(streamOf(c, hipStream), im.dBlob, im.layout, *params, *film, dev_blocksTri, dev_blocksSph, dev_map, dev_hits,
                                            dev_chain, (uint32_t)n, dev_out, dev_info, &c->lightmapChainLaunches));
    return PTSS_OK;
}

int ptss_lightmap_chain_launches(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->lightmapChainLaunches;
    return PTSS_OK;
}

int ptss_lightmap_launches(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->lightmapLaunches;
    return PTSS_OK;
}

int ptss_debug_lightmap_form(ptss_context* c, int form) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (form < 0 || form > 2) return fail(PTSS_EINVAL, "form must be 0, 1 or 2");
    c->lightmapForm = form;
    return PTSS_OK;
}

// ---- the resolves of the two linear films (ptss_resolve.hip). Like the film calls: no frame state, the caller's stream ----
// The one body behind the six, each of which has checked ctx. In this order: the film's parameters (with `glare`: glareArguments), then
// rangeCall's checks — count == 0, the buffers, the range, the scene image, nothing to write. The buffers: `missing` is the caller's
// verdict on the pointers it requires, `nullText` and `alignText` are its own wordings; the alignment asked of a pointer is the same in
// every call, and a pointer a call does not have is null. With `glare` the range has to lie in the film as well, which is looked at
// once the buffers have passed. dev_state: the metered resolves' (required there: `missing`), a glare resolve's or nullptr
static int resolveLinearFilm(ptss_context* c, const void* dev_film, bool splat, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             const ptss_meter_state* dev_state, const ptss::GlareResolveArgs* glare, bool missing, const char* nullText,
                             const char* alignText, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history,
                             unsigned long long* launches, void* hipStream) {
    if (glare) {
        RC_TRY(glareArguments(c, params, glare->params, splat ? PTSS_GLARE_FILM_SPLAT : PTSS_GLARE_FILM_LINEAR, glare->width, glare->height));
    } else if (const char* what = ptlin::paramsError(params)) {
        return fail(PTSS_EINVAL, what);
    }
    const void* dev_pyramid = glare ? glare->pyramid : nullptr;
    const char* bad = missing ? nullText
                      : (((uintptr_t)dev_film | (uintptr_t)dev_pyramid | (uintptr_t)dev_linear | (uintptr_t)dev_history) & 15u) ||
                              ((uintptr_t)dev_state & 7u) || ((uintptr_t)dev_pixels & 3u)
                          ? alignText
                          : nullptr;
    if (glare && count != 0 && !bad) {
        const unsigned long long filmPixels = (unsigned long long)glare->width * (unsigned long long)glare->height;   // below 2^31
        if (firstPixel > filmPixels || count > filmPixels - firstPixel) return fail(PTSS_ERANGE, "firstPixel + count leaves the film");
    }
    FilmCall f;
    RC_TRY(rangeCall(c, &f, firstPixel, count, bad, true, dev_linear || dev_pixels || dev_history, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchLinearFilmResolve(f.st, dev_film, splat, f.firstPixel, f.n, *params, dev_state, glare, f.quantTable, dev_linear, dev_pixels,
                                          dev_history, launches));
    return PTSS_OK;
}

static const char* const kResolveAlign = "film, linear and history must be 16-byte aligned, dev_pixels 4-byte aligned";
static const char* const kResolveMeteredAlign = "film, linear and history must be 16-byte aligned, dev_state 8-byte, dev_pixels 4-byte aligned";
static const char* const kResolveGlareAlign =
    "film, pyramid, linear and history must be 16-byte aligned, dev_state 8-byte, dev_pixels 4-byte aligned";

int ptss_resolve_linear(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                        ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, false, firstPixel, count, params, nullptr, nullptr, !dev_film, "null film with count > 0", kResolveAlign,
                             dev_linear, dev_pixels, dev_history, &c->linearLaunches[1], hipStream);
}

int ptss_resolve_splat(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                       ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, true, firstPixel, count, params, nullptr, nullptr, !dev_film, "null film with count > 0", kResolveAlign,
                             dev_linear, dev_pixels, dev_history, &c->splatLaunches[2], hipStream);
}

int ptss_resolve_linear_metered(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                                const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                                ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, false, firstPixel, count, params, dev_state, nullptr, !dev_film || !dev_state,
                             "null film or state with count > 0", kResolveMeteredAlign, dev_linear, dev_pixels, dev_history,
                             &c->meterLaunches[2], hipStream);
}

int ptss_resolve_splat_metered(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                               const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                               ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, true, firstPixel, count, params, dev_state, nullptr, !dev_film || !dev_state,
                             "null film or state with count > 0", kResolveMeteredAlign, dev_linear, dev_pixels, dev_history,
                             &c->meterLaunches[2], hipStream);
}

int ptss_resolve_linear_glare(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                              int width, int height, const ptss_glare_params* glare, const ptss_glare_entry* dev_pyramid,
                              const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                              ptss_history_entry* dev_history, void* hipStream) {
    const ptss::GlareResolveArgs g{width, height, glare, dev_pyramid};
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, false, firstPixel, count, params, dev_state, &g, !dev_film || !dev_pyramid,
                             "null film or pyramid with count > 0", kResolveGlareAlign, dev_linear, dev_pixels, dev_history,
                             &c->glareLaunches[2], hipStream);
}

int ptss_resolve_splat_glare(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             int width, int height, const ptss_glare_params* glare, const ptss_glare_entry* dev_pyramid,
                             const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                             ptss_history_entry* dev_history, void* hipStream) {
    const ptss::GlareResolveArgs g{width, height, glare, dev_pyramid};
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, true, firstPixel, count, params, dev_state, &g, !dev_film || !dev_pyramid,
                             "null film or pyramid with count > 0", kResolveGlareAlign, dev_linear, dev_pixels, dev_history,
                             &c->glareLaunches[2], hipStream);
}

// ---- tone curves for the two linear films (ptss_tone.hip; csrc/pttone.h). Like the film calls: no frame state, the caller's stream ----
int ptss_default_tone_params(ptss_tone_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_tone_params);
    p->curve = PTSS_TONE_FILMIC;   // design choices, not measurements: a common filmic fit, the display's own transfer, the TGA's depth
    p->transfer = PTSS_TRANSFER_SRGB;
    p->bits = 8;
    p->flags = 0u;
    p->white = 4.0f;
    p->filmic[0] = 2.51f, p->filmic[1] = 0.03f, p->filmic[2] = 2.43f, p->filmic[3] = 0.59f, p->filmic[4] = 0.14f;
    p->reserved = 0u;
    return PTSS_OK;
}

size_t ptss_tone_table_floats(int bits) { return (bits == 8 || bits == 10) ? (size_t)pttone::tableFloats(bits) : 0; }

int ptss_tone_build(ptss_context* c, const ptss_tone_params* tone, float* dev_table, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = pttone::paramsError(tone)) return fail(PTSS_EINVAL, what);
    if (!dev_table) return fail(PTSS_EINVAL, "dev_table is null");
    if ((uintptr_t)dev_table & 15u) return fail(PTSS_EINVAL, "dev_table must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchToneBuild(streamOf(c, hipStream), *tone, dev_table, &c->toneLaunches[0]));
    return PTSS_OK;
}

int ptss_resolve_toned(ptss_context* c, const void* dev_film, int filmKind, size_t firstPixel, size_t count, const ptss_linear_params* params,
                       const ptss_tone_params* tone, const float* dev_table, const ptss_meter_state* dev_state, int width, int height,
                       const ptss_glare_params* glare, const ptss_glare_entry* dev_pyramid, ptss_history_entry* dev_linear, uint32_t* dev_pixels,
                       ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return fail(PTSS_EINVAL, "unknown film kind");
    if (glare)
        RC_TRY(glareArguments(c, params, glare, filmKind, width, height));
    else if (const char* what = ptlin::paramsError(params))
        return fail(PTSS_EINVAL, what);
    if (const char* what = pttone::paramsError(tone)) return fail(PTSS_EINVAL, what);
    if (!glare && dev_pyramid) return fail(PTSS_EINVAL, "a pyramid needs its glare parameters");
    const bool missing = !dev_film || !dev_table || (glare && !dev_pyramid);
    const char* bad = missing ? "null film, table or pyramid with count > 0"
                      : (((uintptr_t)dev_film | (uintptr_t)dev_table | (uintptr_t)dev_pyramid | (uintptr_t)dev_linear | (uintptr_t)dev_history) & 15u) ||
                              ((uintptr_t)dev_state & 7u) || ((uintptr_t)dev_pixels & 3u)
                          ? "film, table, pyramid, linear and history must be 16-byte aligned, dev_state 8-byte, dev_pixels 4-byte aligned"
                          : nullptr;
    if (glare && count != 0 && !bad) {
        const unsigned long long filmPixels = (unsigned long long)width * (unsigned long long)height;   // below 2^31
        if (firstPixel > filmPixels || count > filmPixels - firstPixel) return fail(PTSS_ERANGE, "firstPixel + count leaves the film");
    }
    FilmCall f;
    RC_TRY(rangeCall(c, &f, firstPixel, count, bad, true, dev_linear || dev_pixels || dev_history, hipStream));
    if (!f.go) return PTSS_OK;
    const ptss::GlareResolveArgs g{width, height, glare, dev_pyramid};
    HIP_TRY(ptss::launchTonedResolve(f.st, dev_film, filmKind == PTSS_FILM_SPLAT, f.firstPixel, f.n, *params, *tone, dev_table, dev_state,
                                     glare ? &g : nullptr, c->toneForm, dev_linear, dev_pixels, dev_history, &c->toneLaunches[1]));
    return PTSS_OK;
}

int ptss_tone_launches(const ptss_context* c, unsigned long long* out2) {
    if (!c || !out2) return fail(PTSS_EINVAL, "null argument");
    out2[0] = c->toneLaunches[0], out2[1] = c->toneLaunches[1];
    return PTSS_OK;
}

int ptss_debug_tone_form(ptss_context* c, int form) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (form < 0 || form > 2) return fail(PTSS_EINVAL, "form must be 0, 1 or 2");
    c->toneForm = form;
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
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    const int fW = factor * c->tile.width, fH = factor * c->tile.height;
    const ptss::TileMap tile{fW, fH, factor * c->tile.localRows, c->tile.rank, c->tile.world, factor * c->tile.bandRows};
    const ptss::EyeParams eye{c->camera, -2 * ptm::tan(c->camera.fieldOfView * 0.5f), (float)fH / (float)fW, 1.0f / fW, 1.0f / fH};
    HIP_TRY(ptss::launchFeatures(st, im.dBlob, im.layout, im.inLds, tile, eye, defaultColor, dev_features_hi, (uint32_t)n,
                                 c->gridCap * ptss::kShards, &c->launchedKernels));
    return PTSS_OK;
}

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

int ptss_upsample_launches(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->upsampleLaunches;
    return PTSS_OK;
}

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
                const hipError_t e = hipMalloc(&plane, (size_t)c->numPixels * sizeof(float4));
                if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PTSS_ENOMEM : PTSS_EHIP, "ptss_denoise: colour planes", e);
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

// ---- scene updates on a live context -----------------------------------------------------------------------------
int ptss_set_scene(ptss_context* c, const ptss_scene_desc* scene) {
    if (!c || !scene) return fail(PTSS_EINVAL, "null argument");
    RC_TRY(validateScene(*scene));
    HIP_TRY(hipSetDevice(c->cfg.device));
    SceneState st;   // the new blobs exist before the old ones go: on any error the context keeps its scene
    RC_TRY(buildSceneState(*scene, c->cfg, (int)c->lanes.size(), c->lanes[0].maxBlocks, c->numCUs, st));
    if (int rc = quiesce(c)) {
        releaseSceneState(st);
        return rc;
    }
    if (c->updated) (void)hipStreamSynchronize(c->updateStream);
    harvestHints(c);   // (every read-back has landed) ... and the old scene's live counts say nothing about the new one's
    for (Lane& ln : c->lanes) ln.haveHint = false;
    for (SceneImage& im : c->images) (void)hipFree(im.dBlob);
    adoptSceneState(c, st);
    c->cameraDirty = true;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_update_triangles(ptss_context* c, const ptss_triangle* dev_triangles, size_t first, size_t count, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (count == 0) return PTSS_OK;
    if (!dev_triangles) return fail(PTSS_EINVAL, "dev_triangles is null with count > 0");
    if ((uintptr_t)dev_triangles & 3u) return fail(PTSS_EINVAL, "dev_triangles must be 4-byte aligned");
    const size_t T = (size_t)c->images[0].layout.numTriangles;
    if (first >= T || count > T - first) return fail(PTSS_ERANGE, "first .. first + count - 1 leaves the scene's triangles");
    for (const SceneImage& im : c->images)
        if (im.dBlob && im.layout.triClassed)
            return fail(PTSS_EINVAL, "the scene image stores its triangles grouped by edge class (T <= 255), an order that depends on the "
                                     "vertices: replace the scene with ptss_set_scene (repacking so small a scene costs microseconds)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    unsigned long long* rejected = c->dTotal + kRejectedWord;
    for (SceneImage& im : c->images) {
        if (!im.dBlob) continue;
        HIP_TRY(ptss::launchSceneUpdate(st, im.dBlob, im.layout, dev_triangles, (uint32_t)first, (uint32_t)count, rejected, &c->launchedKernels));
        rejected = nullptr;   // the second image drops the same records: counted once
        if (ptss::meshImage(im.layout)) HIP_TRY(ptss::launchMeshRefit(st, im.dBlob, im.layout, &c->launchedKernels));
    }
    c->updateStream = st;
    c->updated = true;
    c->cameraDirty = true;   // the camera-origin rows (offPrimTri) belong to the old vertices
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

// The kd order rebuilt on the device (csrc/ptorder.h, ptss_resort.hip). Only a mesh image has one: a context never holds a
// mesh image beside a second image (planImages), so at most one image is re-sorted.
int ptss_resort_triangles(ptss_context* c, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    SceneImage* mesh = nullptr;
    for (SceneImage& im : c->images)
        if (im.dBlob && ptss::meshImage(im.layout)) mesh = &im;
    if (!mesh) return PTSS_OK;   // no kd order to rebuild: nothing launched, nothing counted
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    // the scratch exists before anything is launched: on failure the image is untouched
    if (int rc = createCheck(ptss::reserveResortScratch(c->resortScratch, mesh->layout.numTriangles), "ptss_resort_triangles: scratch")) return rc;
    HIP_TRY(ptss::launchResort(st, mesh->dBlob, mesh->layout, c->resortScratch));
    ++c->resortLaunches;
    HIP_TRY(ptss::launchMeshRefit(st, mesh->dBlob, mesh->layout, &c->launchedKernels));
    c->updateStream = st;
    c->updated = true;
    c->cameraDirty = true;   // the camera-origin rows (offPrimTri) are indexed by stored position
    return PTSS_OK;          // the same scene: no reset
}

int ptss_resort_launches(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->resortLaunches;
    return PTSS_OK;
}

int ptss_update_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->updated) HIP_TRY(hipStreamSynchronize(c->updateStream));
    HIP_TRY(hipMemcpy(out, c->dTotal + kRejectedWord, sizeof(*out), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_reseed(ptss_context* c, unsigned long long seed) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    HIP_TRY(hipSetDevice(c->cfg.device));
    RC_TRY(quiesce(c));   // no lane is still drawing from the streams
    if (int rc = createCheck(seedStreams(c, seed, c->stream), "ptss_reseed: rngInitKernel")) return rc;
    c->cfg.seed = seed;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_read_triangle_bounds(ptss_context* c, float* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    const SceneImage& im = c->image();
    if (!ptss::meshImage(im.layout)) return fail(PTSS_EINVAL, "the scene image in use is not a mesh image");
    const size_t leaves = (size_t)im.layout.mesh.numLeaves, groups = (size_t)im.layout.mesh.numGroups;
    if (count != 12 * (leaves + groups)) return fail(PTSS_ERANGE, "count must be 12 * (leaves + groups)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->updated) HIP_TRY(hipStreamSynchronize(c->updateStream));
    HIP_TRY(hipMemcpy(host, im.dBlob + im.layout.mesh.offLeaf, 12 * leaves * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host + 12 * leaves, im.dBlob + im.layout.mesh.offGroup, 12 * groups * sizeof(float), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_read_triangle_positions(ptss_context* c, int* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    const SceneImage& im = c->image();
    if (!ptss::meshImage(im.layout)) return fail(PTSS_EINVAL, "the scene image in use is not a mesh image");
    if (count != (size_t)im.layout.numTriangles) return fail(PTSS_ERANGE, "count must be the scene's triangle count");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->updated) HIP_TRY(hipStreamSynchronize(c->updateStream));
    HIP_TRY(hipMemcpy(host, im.dBlob + im.layout.offTriPos, count * sizeof(int), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_triangle_leaves(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    const ptss::SceneLayout& L = c->image().layout;
    *out = ptss::meshImage(L) ? L.mesh.numLeaves : 0;
    return PTSS_OK;
}

int ptss_debug_counters(ptss_context* c, unsigned long long* out8) {
    if (!c || !out8) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
#if PTSS_DIAG
    HIP_TRY(ptss::readDiagCounters(out8));
#else
    for (int k = 0; k < 8; ++k) out8[k] = 0ull;   // the shipped library carries no counter (ptss_diag.h)
#endif
    return PTSS_OK;
}

int ptss_bounce_kernel_time(ptss_context* c, double* total_ms, unsigned long long* launches) {
    if (!c || !total_ms || !launches) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Lane& ln : c->lanes)
        if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
    drainKernelEvents(c, true);
    // union of the launch intervals (one lane: they do not overlap, and this is the sum of the durations)
    std::sort(c->kernelSpans.begin(), c->kernelSpans.end());
    double busy = 0.0, curA = 0.0, curB = -1.0;
    for (const auto& sp : c->kernelSpans) {
        if (curB < curA || sp.first > curB) {
            if (curB >= curA) busy += curB - curA;
            curA = sp.first;
            curB = sp.second;
        } else if (sp.second > curB) {
            curB = sp.second;
        }
    }
    if (curB >= curA) busy += curB - curA;
    *total_ms = busy;
    *launches = c->kernelSpans.size();
    c->kernelSpans.clear();
    HIP_TRY(hipEventRecord(c->evEpoch, c->stream));   // a fresh epoch for the next window: float32 ms stay fine-grained
    HIP_TRY(hipEventSynchronize(c->evEpoch));
    return checkLaneTimeouts(c);
}

}  // extern "C"
