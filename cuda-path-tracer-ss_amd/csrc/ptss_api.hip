// ptss_api.hip — context management and the frame driver behind include/ptss.h: version, error text and default config; create,
// destroy and ptss_generate_frame; camera, mode, stream and accumulator calls; the read-backs of frame state; scene updates on a
// live context; diagnostics. The other call families live in ptss_api_query.hip, ptss_api_film.hip and ptss_api_post.hip, the
// context itself in ptss_context.h.
//
// ptss_generate_frame is the reference's generateFrame (CudaTracer/CudaTracer.cu:587-647) with the
// host taken out of the inner loop: the per-bounce live-ray count stays on the device
// (FrameBuffers::counts), every bounce kernel is launched unconditionally and applies the
// reference's `numRays > 128` guard itself, so a frame is one uninterrupted stream of launches
// with at most one event wait at the end (cfg.syncEachFrame, the reference's :639-642).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <new>
#include <string>

#include "ptss_context.h"
#include "ptpack.h"
#include "ptstrip.h"

using namespace ptv;
using ptpack::cameraInRange;
static_assert(sizeof(ptpack::Row) == sizeof(float4) && alignof(ptpack::Row) == alignof(float4), "a packed row is uploaded as a float4");

#if PTSS_DIAG
namespace ptss { hipError_t readDiagCounters(unsigned long long* out8); }
#endif

static thread_local std::string g_detail;   // the text behind ptss_last_error_detail: every file of the layer writes it through fail

int fail(int code, const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf, sizeof(buf), "%s", what);
    g_detail = buf;
    return code;
}

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
    fb.totalRayBounces = c->dTotal + kLaneTotalsWord + laneIdx;
    fb.guardTimeouts = reinterpret_cast<uint32_t*>(c->dTotal + kGuardTimeoutsWord);
    fb.accum = c->dAccum;
    fb.fsum = c->dFsum;
    fb.staged = c->dStaged ? c->dStaged + (c->stagedTwice ? (size_t)(c->frameIndex & 1u) * c->capacity * c->samples : 0) : nullptr;
    fb.quantTable = quantTableOf(c->image());
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
    HIP_TRY(hipMemcpy(&v, c->dTotal + kGuardTimeoutsWord, sizeof(v), hipMemcpyDeviceToHost));
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
    HIP_TRY(hipMemcpy(perLane, c->dTotal + kLaneTotalsWord, sizeof(perLane), hipMemcpyDeviceToHost));
    *out = 0;
    for (size_t k = 0; k < c->lanes.size(); ++k) *out += perLane[k];
    return checkLaneTimeouts(c);
}

int ptss_guard_timeouts(ptss_context* c, unsigned int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, c->dTotal + kGuardTimeoutsWord, sizeof(v), hipMemcpyDeviceToHost));
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

int ptss_launched_kernels(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::launchedKernels, out); }

int ptss_guard_flags(const ptss_context* c, unsigned int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->image().guardFlags;
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
    (void)c->lastUpdate.synchronize();
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
    c->lastUpdate.note(st);
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
    c->lastUpdate.note(st);
    c->cameraDirty = true;   // the camera-origin rows (offPrimTri) are indexed by stored position
    return PTSS_OK;          // the same scene: no reset
}

int ptss_resort_launches(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::resortLaunches, out); }

int ptss_update_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    return readBehind(c, c->lastUpdate, c->dTotal + kRejectedWord, 1, out);
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
    HIP_TRY(c->lastUpdate.synchronize());
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
    HIP_TRY(c->lastUpdate.synchronize());
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
