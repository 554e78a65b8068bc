// ptss_device.h — device-side data layout shared by the kernels (ptss_kernels.hip) and the
// context code (ptss_api*.hip, over ptss_context.h). See DESIGN.md "Data layout in HBM". The scene image's own description (SceneLayout, the sizes that
// shape it, bounceLdsBytes) is host-clean and lives in ptscene.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptmath.h"
#include "ptscene.h"
#include "ptss_types.h"
#include "xorwow.h"

namespace ptdn { struct Level; }   // ptdenoise.h
namespace ptrp { struct View; struct Params; }   // ptreproject.h
namespace ptcam { struct Film; }   // ptcamera.h

namespace ptss {

// ---- ray pools: struct-of-arrays in tile blocks ------------------------------------------------------------
// A pool is cut into kShards equal regions of regionCap slots; the workgroups with blockIdx % kShards == s read and write
// region s only and own the s-th live-ray counter, so the compaction atomics of one launch are spread over kShards
// addresses (one address sustains only ~88 returning atomics/us on MI355X — measured: a single counter was a 45 ps/ray
// serial floor, profiles/README.md). A region's survivors can never outnumber its input, so regionCap =
// ceil(tiles / kShards) * kBlock always suffices. Inside a region the rays of one tile (kBlock consecutive slots) form a
// BLOCK of kRayPlanes planes of kBlock words: word (slot, plane p) = ((slot / kBlock) * kRayPlanes + p) * kBlock +
// slot % kBlock. Lane i of a wave touches word i of a plane — 256-B contiguous wave accesses — and a plane's offset
// inside the block is a compile-time constant (addressing: ptraypool.h, tileBlock / slotWord).
enum RayPlane : int {
    kOx = 0, kOy, kOz,        // origin
    kDx, kDy, kDz,            // direction
    kL0x, kL0y, kL0z,         // radiance0 (accumulated)
    kTx, kTy, kTz,            // radiance1 (throughput)
    kPix,                     // local pixel index (Ray::pixelOffset)
    kR0, kR1, kR2, kR3, kR4,  // XORWOW v[0..4]
    kRd,                      // XORWOW d
    kRayPlanes                // = 19 planes = 76 B per ray
};
constexpr int kHomeWords = 8;     // per-pixel RNG home record: v0..v4, d, 2 pad words (32 B)
constexpr int kMaxBounces = 64;  // counts has (kMaxBounces + 1) x kShards entries
// Build-time switches (eight, PTSS_BLOCK and PTSS_CHUNK of them in ptscene.h; tools/build_variants.py builds A/B variants — the shipped library uses the defaults). What was
// tried and rejected with numbers lives in profiles/README.md and in the history, not behind switches here.
#ifndef PTSS_SHARDS
#define PTSS_SHARDS 16    // pool regions / live-ray counters per bounce
#endif
#ifndef PTSS_MINWAVES
#define PTSS_MINWAVES 7   // __launch_bounds__ waves/SIMD of the unbounded-geometry instantiations: 72 VGPRs. Measured, same box:
                          // 5 waves (96 VGPRs) 13.3, 6 (80) 14.2, 7 (72) 14.5, 8 (64, spills) 11.4 Grays/s
#endif
#ifndef PTSS_MINWAVES_BOUNDED
#define PTSS_MINWAVES_BOUNDED 6   // the instantiations for bounded scenes (SceneLayout::sphereBounded: the shorter sphere test) want 80
                                  // registers: at 7 waves the shorter test costs 3 % (32 instead of 16 B of scratch), at 6 it gains — same-box
                                  // A/B against 7 waves + the long test: c3 +0.5 %, c2 +2.3 %, one sample per tick at 1080p +2.5-3 %
#endif
#ifndef PTSS_MINWAVES_FIRST
#define PTSS_MINWAVES_FIRST 6   // bounce 0's instantiation (eye rays fused in, camera-origin tests): at 7 waves it spills 32 B, at 6
                                // (80 VGPRs) none — same-box A/B: that kernel 3,035 -> 2,826 us per launch, the pass +0.9 %
#endif
#ifndef PTSS_ABLATE
#define PTSS_ABLATE 0   // measurement only (WRONG images): bit 0 no NEE, 1 no closest-hit loops, 2 no scatter, 3 no finishPath
#endif
#ifndef PTSS_DIAG
#define PTSS_DIAG 0     // diagnostic counters (ptss_diag.h; tools/*_hist.py, *_stat.py): bit 0 sphere candidates per lane, 1 scatter
                        // blocks, 2 chunk culling, 3 shadow-segment pairs, 4 shadow-queue lengths. 0: no counter exists in the code
#endif
constexpr int kShards = PTSS_SHARDS;        // pool regions / live-ray counters per bounce
constexpr int kCountStride = 32;            // one counter per 128-B line
constexpr int kCountWords = (kMaxBounces + 1) * kShards * kCountStride;
__host__ __device__ inline int countIndex(int bounce, int shard) { return (bounce * kShards + shard) * kCountStride; }
constexpr uint32_t kMinLiveRays = 128;  // loop guard `numRays > 128`, CudaTracer.cu:622

struct TileMap {
    int width, height;      // full frame
    int localRows;          // rows owned by this context
    int rank, world, bandRows;
};

struct EyeParams {  // computeEyeRay constants evaluated once on the host with ptm::tan
    ptss_camera camera;
    float s;        // -2 * tan(fov/2)
    float aspect;   // H / W
    float invW, invH;
    const unsigned long long* strips;   // bounce 0 of a bounce kernel: the strip words of this camera (ptstrip.h; word waveFirst >> 6), or nullptr:
                                        // every primitive is visited. The last member: no other kernel argument moves
};

// ---- frame lanes: one frame traced as K independent ray populations on K streams of one device -----------------
// A launch-shaped pass (one sample per pixel: ten kernels of 30-90 us) loses a fifth of its time to the ramp and tail of
// launches only a few resident rounds wide. Lane k owns the bounce-0 tiles of rounds R with R % K == k (round R = tiles
// 16 R .. 16 R + 15, one per shard), its own pools, counters and stream; all per-pixel state (random streams,
// accumulator, display) is shared — lanes touch disjoint pixels. The tail of one lane's launch overlaps the other lanes'
// kernels. The loop guard `numRays > 128` (CudaTracer.cu:622) stays a WHOLE-FRAME quantity: a lane whose own count is
// above 128 knows the frame's is; only a lane holding <= 128 rays (then at most one workgroup per shard has work) waits
// for its peers' counts of that bounce and adds them up. "Peer p's counts of bounce b are final" means: every workgroup of
// p's bounce b - 1 launch has ended. Each workgroup of a bounce kernel therefore adds 1 to its lane's done[b - 1][shard]
// as its last act (sixteen counters per bounce, one per 128-B line, never reset: they grow by the grid size of every
// frame's launch), and the host hands each launch the total the peers' counters reach once their bounce b - 1 of THIS
// frame is through (it knows every grid it launched). The waiter only ever depends on kernels that were enqueued before
// it — all lanes' bounce b - 1 launches precede any lane's bounce b in host order — so lanes that share a hardware queue
// cannot deadlock. (Earlier designs, measured: a stream-ordered hipStreamWriteValue32 after every kernel cost 9 %; a done
// word stored at the START of bounce b plus a one-thread signal kernel behind bounce b - 1 of lanes 1.. cost 4 %.)
// So the image is the one-lane image, exactly, for every K, whatever the streams' queue mapping.
constexpr int kMaxLanes = 4;

struct FrameBuffers {
    float* pool[2];          // ray pools (ping-pong), kRayPlanes planes each
    uint32_t* rngHome;       // kHomeWords words per local pixel: where a pixel's stream rests between paths
    uint32_t* counts;        // counts[countIndex(b, s)]: rays of shard s entering bounce b of the current frame (two buffers
                             // alternate per frame, so that a peer lane can still read this frame's counts after flushKernel)
    uint32_t* countsNext;    // the other buffer: flushKernel arms it for the next frame
    const uint32_t* shardCount0;  // [kShards] pixels per shard (constant per context): counts of bounce 0
    uint32_t* lastCounts;    // the previous frame's counts (copied by flushKernel before it re-arms `counts`)
    unsigned long long* totalRayBounces;
    uint32_t* accum;         // uint3 per local pixel (totalPixelColors)
    float* fsum;             // float3 per local pixel or nullptr
    const float* quantTable; // the same thresholds in global memory (flushKernel has no staged scene)
    uint32_t* staged;        // S > 1 only: this pass's sample of every stream, x | y << 8 | z << 16 (one plane per sample lane)
    ptss_uchar4* pixels;     // display buffer or nullptr
    uint32_t regionCap;      // slots per shard region (a multiple of kBlock); a region is regionCap * kRayPlanes words
    uint32_t numPixels;      // local pixels
    uint32_t plane;          // numPixels rounded up to kBlock: stride of the per-pixel planes (one plane per sample lane)
    uint32_t samples;        // S = cfg.samplesPerPass: independent random streams per pixel traced per pass
    uint32_t firstTiles;     // tiles of bounce 0 = S * plane / kBlock
    uint32_t minLive;        // a bounce runs while more than this many rays are live: 128 (CudaTracer.cu:622),
                             // 0 in a sharded context (the guard is a whole-frame quantity; DESIGN.md "Sharding")
    float inverseTicks;      // 1.f / (ticks - lastResetTick + 1)
    float defaultColor[3];
    uint32_t guardFlags;     // GuardFlag bits (ptscene.h) of the scene the frame renders: which range guards hold for its constants
    // frame lanes (laneCount = 1: everything below is inert)
    uint32_t laneIndex, laneCount;
    uint32_t frameRays;              // rays all lanes together start a pass with (numPixels x samples): bounce 0's guard
    uint32_t numPeers;               // laneCount - 1
    const uint32_t* peerCounts[kMaxLanes - 1];  // the peers' counts[] of the current frame
    const uint32_t* peerDone[kMaxLanes - 1];    // the peers' done[countIndex(b, s)]: workgroups of shard s that ended bounce b, all frames
    uint32_t peerTarget[kMaxLanes - 1];         // bounce kernel of bounce b: what peer p's done[b - 1][*] add up to once its bounce
                                                // b - 1 of this frame has ended (compared wrap-safe)
    uint32_t* myDone;                // this lane's own counters
    // flushKernel re-arms the count buffer of the frame BEFORE this one for the frame after it, and a peer lane may run one
    // frame behind and still read that buffer: each lane counts its finished frames (flushKernel's last act), and a flush
    // waits (bounded) until every peer has finished the previous frame. (As stream-ordered event waits between the lanes'
    // streams the same dependency cost 3.5 % of a 1080p pass at one sample per tick.)
    uint32_t* myFrameDone;                          // frames this lane has finished, all time
    const uint32_t* peerFrameDone[kMaxLanes - 1];
    uint32_t frameSeq;                              // frames finished before this one (what the peers' counters must have reached)
    uint32_t joinsFrame;                            // 1 in the LAST lane: its flushKernel also waits for the peers' flushes of THIS frame (all of them
                                                    // enqueued before it), so that one event behind it orders the caller's stream after the whole frame
    uint32_t* guardTimeouts;         // incremented when a wait for a peer lane expired (must stay 0). The host reads it at its next
                                     // synchronising call and returns PTSS_ETIMEOUT (ptss_api.hip checkLaneTimeouts)
};

// ---- launchers (ptss_kernels.hip) --------------------------------------------------------------
// Every launcher that takes `launched` records the instantiation it enqueued there, once the launch has succeeded: bit `base + index`
// of ptss_launched_kernels, base one of the PTSS_KERNEL_* ranges (ptss_types.h), index the instantiation's place in its range.
inline void markLaunched(unsigned long long* launched, int base, int index = 0) { *launched |= 1ull << (base + index); }
hipError_t launchRngInit(hipStream_t st, uint32_t* rngHome, uint32_t plane, uint32_t samples, TileMap tile, uint64_t seed,
                         const uint32_t* jumpTable);
hipError_t launchDisplay(hipStream_t st, const FrameBuffers& fb);
hipError_t launchClear(hipStream_t st, const FrameBuffers& fb);
hipError_t launchPrimaryPrep(hipStream_t st, float4* sceneBlob, const SceneLayout& layout, ptss_vec3 origin);
// the strip words of a camera (ptstrip.h): masks = plane / 64 words, one per 64 local pixels of the context's plane
hipError_t launchStripMasks(hipStream_t st, unsigned long long* masks, uint32_t plane, uint32_t numPixels, const float4* sceneBlob,
                            const SceneLayout& layout, TileMap tile, EyeParams eye);
hipError_t launchBounce(hipStream_t st, const FrameBuffers& fb, const float4* sceneBlob, SceneLayout layout, int bounce,
                        bool isLast, bool sceneInLds, bool bounded, int gridBlocks, TileMap tile, EyeParams eye, unsigned long long* launched);
hipError_t launchFrame(hipStream_t st, const FrameBuffers& fb, const float4* sceneBlob, SceneLayout layout, int numBounces, bool bounded, int gridBlocks,
                       TileMap tile, EyeParams eye, unsigned long long* launched);   // every bounce of a frame in ONE launch (frameKernel): the whole grid must be resident
int frameOccupancyBlocksPerCU(const SceneLayout& layout, bool bounded);
struct FlushTargets {  // flushKernel re-derives the guard of every bounce: target[p][b] = peer p's done total after ITS bounce b of this frame
    uint32_t target[kMaxLanes - 1][kMaxBounces + 1];
};
hipError_t launchFlush(hipStream_t st, const FrameBuffers& fb, int numBounces, const FlushTargets& targets);  // one per lane
int bounceOccupancyBlocksPerCU(const SceneLayout& layout, bool sceneInLds, bool bounded);
// batched ray queries (ptss_intersect / ptss_occluded): rays = n x 32 B, out = n x 48 B hits (any = false) or n uint32 verdicts
hipError_t launchQuery(hipStream_t st, bool any, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* out,
                       uint32_t n, int maxBlocks, unsigned long long* launched);
// first-hit features (ptss_render_features): out = n x 32 B, one ptss_pixel_feature per local pixel
hipError_t launchFeatures(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                          ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, unsigned long long* launched);
// ... and the motion rows beside them (ptss_render_features_motion; PTSS_KERNEL_FEATURES_MOTION + inLds of *launched): prevRecords = `count` caller
// records (76 B each, a device pointer; not read when count = 0), motionOut = n x 16 B, one ptss_pixel_motion per local pixel
hipError_t launchFeaturesMotion(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                                ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, const void* prevRecords, uint32_t first,
                                uint32_t count, void* motionOut, unsigned long long* launched);
// features behind mirrors and glass (ptss_render_features_specular; csrc/ptspecular.h): out as launchFeatures', steps = n uint32 or nullptr,
// maxSteps 0 .. ptsp::kMaxSteps. No bit of ptss_launched_kernels: launches[0] (in place) or launches[1] (in LDS) is incremented
hipError_t launchFeaturesSpecular(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                                  ptss_vec3 defaultColor, void* out, void* steps, uint32_t n, int maxSteps, int maxBlocks,
                                  unsigned long long* launches);
// batched path queries (ptss_paths.hip; ptss_seed_path_rng / ptss_trace_paths): rng = n x 24 B (ptss_path_rng), rays = n x 32 B, out = n x 16 B
// (ptss_path_result); firstSequence + n <= 2^32; maxIterations 1 .. kMaxBounces. No bit of ptss_launched_kernels: launches[0] (in place) or
// launches[1] (in LDS) is incremented by launchPathQuery
hipError_t launchPathRngSeed(hipStream_t st, void* rng, uint32_t n, uint64_t seed, uint32_t firstSequence, uint32_t skip, const uint32_t* jumpTable);
hipError_t launchPathQuery(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* rng, void* out,
                           uint32_t n, int maxIterations, ptss_vec3 defaultColor, uint32_t guardFlags, int maxBlocks, unsigned long long* launches);
// ... with the refill schedule (ptss_trace_paths_opt, PTSS_PATHS_REFILL): the same buffers and bytes. maxWorkgroups >= 0 caps
// the grid (0: the resident workgroups of the instantiation on numCUs compute units). state: kPathRefillWords 64-bit device words of the
// context, [0] the queue head, set on `st` in front of the kernel, [1..3] wave iterations, lane iterations, dequeues (cumulative). Its own
// launches[0] / launches[1]
constexpr int kPathRefillWords = 4;
hipError_t launchPathRefill(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* rng, void* out,
                            uint32_t n, int maxIterations, ptss_vec3 defaultColor, uint32_t guardFlags, int maxWorkgroups, int numCUs,
                            unsigned long long* state, unsigned long long* launches);
// the film of a path query (ptss_film.hip; ptss_generate_rays / ptss_accumulate_paths / ptss_ray_features): index = n uint32 or nullptr (then
// pixel firstPixel + i, and firstPixel + n <= the film's pixels), rng = n x 24 B, rays = n x 32 B, results = n x 16 B, film = filmPixels x 16 B
// (ptss_film_entry), pixels / history = filmPixels entries or nullptr, features = n x 32 B. rejected: the device counter of dropped index
// entries. No bit of ptss_launched_kernels: *launches is incremented once per call that launched
// positions: n x 8 B (ptss_film_position) written as well, or nullptr (ptss_generate_rays' own kernel, as it was)
hipError_t launchFilmRays(hipStream_t st, const ptcam::Film& film, uint32_t firstPixel, const uint32_t* index, uint32_t n, void* rng, void* rays,
                          void* positions, unsigned long long* rejected, unsigned long long* launches);
hipError_t launchFilmAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                uint32_t filmPixels, ptss_uchar4* pixels, void* history, const float* quantTable, unsigned long long* rejected,
                                unsigned long long* launches);
hipError_t launchRayFeatures(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays,
                             ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, unsigned long long* launches);
// adaptive film sampling (ptss_adaptive.hip; ptss_accumulate_paths_stats / ptss_plan_samples). launchStatsAccumulate:
// launchFilmAccumulate's buffers and bytes plus moments = filmPixels x 8 B, each ray's squared bytes added. launchPlanSamples: cdf =
// ptad::cdfEntries(filmPixels) x 8 B (the film's running sums, then the scan's workspace), index = n uint32 out, info = 32 B or nullptr.
// No bit of ptss_launched_kernels: *launches is incremented once per call that launched
hipError_t launchStatsAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                 unsigned long long* moments, uint32_t filmPixels, ptss_uchar4* pixels, void* history, const float* quantTable,
                                 unsigned long long* rejected, unsigned long long* launches);
hipError_t launchPlanSamples(hipStream_t st, const void* film, const unsigned long long* moments, uint32_t filmPixels,
                             const ptss_plan_params& params, uint32_t n, unsigned long long* cdf, uint32_t* index, ptss_plan_info* info,
                             unsigned long long* launches);
// adaptive sampling on the linear film (ptss_adaptive.hip; ptss_plan_samples_linear; the moments are launchLinearAccumulate's).
// launchPlanSamplesLinear: launchPlanSamples' cdf, index and info over moments = filmPixels x 32 B (ptss_linear_moment); both params checked
// by the caller (ptlin::paramsError, ptls::paramsError). No bit of ptss_launched_kernels: *launches is incremented once per call that launched
hipError_t launchPlanSamplesLinear(hipStream_t st, const void* moments, uint32_t filmPixels, const ptss_linear_params& film,
                                   const ptss_linear_plan_params& params, uint32_t n, unsigned long long* cdf, uint32_t* index,
                                   ptss_plan_info* info, unsigned long long* launches);
// the linear film (ptss_linear.hip; ptss_accumulate_paths_linear / ptss_accumulate_paths_linear_stats).
// launchLinearAccumulate: launchFilmAccumulate's results, index and counter, film = filmPixels x 32 B (ptss_linear_entry), moments =
// filmPixels x 32 B (ptss_linear_moment); each of the two may be nullptr, not both. params: checked by the caller (ptlin::paramsError).
// No bit of ptss_launched_kernels: *launches is incremented once per call that launched
hipError_t launchLinearAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                  void* moments, uint32_t filmPixels, const ptss_linear_params& params, unsigned long long* rejected,
                                  unsigned long long* launches);
// the resolves of the two linear films (ptss_resolve.hip; ptss_resolve_linear / ptss_resolve_splat, their _metered and _glare forms; DESIGN.md
// §3.29 - §3.32): pixels firstPixel .. firstPixel + count of the film, 32 B per pixel and a ptss_splat_entry where `splat`, into linear /
// history (16 B per pixel) and pixels, each or nullptr (not all three). state = 48 B, read, or nullptr: no exposure but params'. glare =
// nullptr, or the film's sides, the glare's parameters and the pyramid launchGlareBuild made, read at level 1 only. params and glare:
// checked by the caller (ptlin::paramsError, ptglare::paramsError, ptglare::sidesError). No bit of ptss_launched_kernels: *launches is
// incremented once per call that launched
struct GlareResolveArgs {
    int width, height;
    const ptss_glare_params* params;
    const void* pyramid;
};
hipError_t launchLinearFilmResolve(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, const ptss_linear_params& params,
                                   const ptss_meter_state* state, const GlareResolveArgs* glare, const float* quantTable, void* linear,
                                   ptss_uchar4* pixels, void* history, unsigned long long* launches);
// tone curves for the two linear films (ptss_tone.hip; ptss_tone_build, ptss_resolve_toned). table =
// pttone::tableFloats(tone.bits) floats, 16-byte aligned. launchTonedResolve: launchLinearFilmResolve's arguments with the tone's
// parameters and its table; pixels = one 32-bit word per pixel; form: 0 the shipped lookup, 1 the table staged in LDS, 2 the guess settled
// against global memory. tone: checked by the caller (pttone::paramsError). No bit of ptss_launched_kernels: *launches is incremented once
// per call that launched
hipError_t launchToneBuild(hipStream_t st, const ptss_tone_params& tone, float* table, unsigned long long* launches);
hipError_t launchTonedResolve(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, const ptss_linear_params& params,
                              const ptss_tone_params& tone, const float* table, const ptss_meter_state* state, const GlareResolveArgs* glare, int form,
                              void* linear, uint32_t* pixels, void* history, unsigned long long* launches);
// the filtered linear film (ptss_splat.hip; ptss_splat_paths / ptss_splat_paths_homed). results = n x 16 B, positions = n x
// 8 B, film = width x height x 32 B (ptss_splat_entry). launchSplatHomed: sample i is homed at pixel firstPixel + i, n > 0 and firstPixel +
// n <= width * height. counters: two device words, samples dropped and samples clamped. filter and params: checked by the caller
// (ptspl::filterError, ptlin::paramsError). No bit of ptss_launched_kernels: *launches is incremented once per call that launched
hipError_t launchSplatScatter(hipStream_t st, const void* results, const void* positions, uint32_t n, void* film, int width, int height,
                              const ptss_splat_filter& filter, const ptss_linear_params& params, unsigned long long* counters,
                              unsigned long long* launches);
hipError_t launchSplatHomed(hipStream_t st, const void* results, const void* positions, uint32_t firstPixel, uint32_t n, void* film, int width,
                            int height, const ptss_splat_filter& filter, const ptss_linear_params& params, unsigned long long* counters,
                            unsigned long long* launches);
// the meter of the two linear films (ptss_meter.hip; ptss_meter_linear / ptss_meter_splat / ptss_meter_exposure). film = 32 B
// per pixel, a ptss_splat_entry where `splat`; histogram = PTSS_METER_BINS x 4 B, added to; state = 48 B, read and written by
// launchMeterExposure. params and meter: checked by the caller (ptlin::paramsError, ptmeter::paramsError). No bit of
// ptss_launched_kernels: *launches is incremented once per call that launched
hipError_t launchMeterHistogram(hipStream_t st, const void* film, bool splat, uint32_t firstPixel, uint32_t count, uint32_t* histogram,
                                unsigned long long* launches);
hipError_t launchMeterExposure(hipStream_t st, const uint32_t* histogram, const ptss_linear_params& params, const ptss_meter_params& meter,
                               ptss_meter_state* state, unsigned long long* launches);
// glare for the two linear films (ptss_glare.hip; ptss_glare_build). film = width x height x 32 B, a ptss_splat_entry where
// `splat`; pyramid = the entries ptglare::layoutOf counts, 32 B each. launches[0] is incremented once when every kernel of the build
// launched, launches[1] by each kernel that did. params and glare: checked by the caller (ptlin::paramsError, ptglare::paramsError,
// ptglare::sidesError). No bit of ptss_launched_kernels
hipError_t launchGlareBuild(hipStream_t st, const void* film, bool splat, int width, int height, const ptss_linear_params& params,
                            const ptss_glare_params& glare, void* pyramid, unsigned long long* launches);
// the denoiser of the two linear films (ptss_lindenoise.hip; ptss_denoise_linear). film = width x height x 32 B, a
// ptss_splat_entry where `splat`; moments and features = 32 B per pixel; workspace = what ptldn::workspaceLayout counts; out = width x
// height x 32 B. form: 0 the measured table of forms per spacing, 1 every pass unstaged, 2 staged wherever a staged kernel exists, 4 + mask staged at
// pass k where bit k of the 3-bit mask is set.
// launches[0] is incremented once when every kernel of the call launched, launches[1] by each kernel that did. params and denoise:
// checked by the caller (ptlin::paramsError, ptldn::paramsError, ptldn::sidesError). No bit of ptss_launched_kernels
hipError_t launchLinearDenoise(hipStream_t st, const void* film, bool splat, int width, int height, const void* moments, const void* features,
                               const ptss_linear_params& params, const ptss_denoise_linear_params& denoise, int form, void* workspace, void* out,
                               unsigned long long* launches);
// seeding a linear film from the previous pose's (ptss_linreproject.hip; ptss_reproject_linear). Every film, moment and
// feature buffer holds 32 B per pixel of its camera; motionNow, momentsPrev / momentsOut (together) and info may be null. *launches is
// incremented when the kernel launched. Everything checked by the caller (ptlrp::cameraError, ptlrp::paramsError, ptlin::paramsError).
// No bit of ptss_launched_kernels
hipError_t launchLinearReproject(hipStream_t st, const ptss_film_camera& now, const void* featuresNow, const void* motionNow,
                                 const ptss_film_camera& prev, const void* featuresPrev, const void* filmPrev, bool splat, const void* momentsPrev,
                                 const ptss_linear_params& film, const ptss_reproject_linear_params& params, void* filmOut, void* momentsOut,
                                 void* info, unsigned long long* launches);
// a linear film of factor times the size from a small one (ptss_linupsample.hip; ptss_upsample_linear). filmLo and
// featuresLo hold 32 B per pixel of width x height, featuresHi and filmHi of factor * width x factor * height; info may be null. form: 0
// the measured table, 1 taps from global memory, 2 staged in LDS. *launches is incremented when the kernel launched. Everything checked
// by the caller (ptlup::paramsError, ptlup::sidesError, ptlin::paramsError). No bit of ptss_launched_kernels
hipError_t launchLinearUpsample(hipStream_t st, const void* filmLo, bool splat, int width, int height, const void* featuresLo,
                                const void* featuresHi, const ptss_linear_params& film, const ptss_upsample_linear_params& params, int form,
                                void* filmHi, void* info, unsigned long long* launches);
// rays from surface points (ptss_surface.hip; ptss_generate_rays_surface). points: numPoints rows of 16 B; rng: n streams of
// 24 B; rays: n rows of 32 B; surfels (may be null): n rows of 48 B; index may be null. The image's counts bound every gather inside
// the kernel; *rejected counts the dropped entries. Everything else checked by the caller (ptsurf::paramsError). *launches is
// incremented when the kernel launched. No bit of ptss_launched_kernels
hipError_t launchSurfaceRays(hipStream_t st, const float4* sceneBlob, const SceneLayout& layout, const ptss_surface_params& params,
                             const void* points, uint32_t numPoints, uint32_t firstPoint, const uint32_t* index, uint32_t n, void* rng, void* rays,
                             void* surfels, unsigned long long* rejected, unsigned long long* launches);
// one gutter-fill pass over a linear film (ptss_surface.hip; ptss_dilate_linear). film and out: width x height entries of 32 B, not the
// same buffer. form: 0 the shipped one, 1 from global memory, 2 staged in LDS. Sides checked by the caller (ptsurf::dilateSidesError)
hipError_t launchDilateLinear(hipStream_t st, const void* film, int width, int height, int form, void* out, unsigned long long* launches);
// hits -> film rows through a baked light map (ptss_lightmap.hip; ptss_lookup_lightmap). blocksTri / blocksSph: rows of 16 B
// (null with a count of 0 in params); map: atlasWidth x atlasHeight entries of 32 B; hits: n rows of 48 B; out: n entries of 32 B; info
// (may be null): four uint32 counts, added to. form: 0 the shipped one, 1 one lane per hit, 2 four lanes per hit. Everything checked by
// the caller (ptlm::paramsError, rangeError); the kernel holds every table row and index against params and the image's counts
hipError_t launchLookupLightmap(hipStream_t st, const float4* sceneBlob, const SceneLayout& layout, const ptss_lightmap_params& params,
                                const ptss_linear_params& film, const void* blocksTri, const void* blocksSph, const void* map, const void* hits,
                                uint32_t n, int form, void* out, void* info, unsigned long long* launches);
// ... tinted by a chain's throughput (ptss_lookup_lightmap_chain): chain = n rows of 32 B (ptss_chain_result), one lane per hit
hipError_t launchLookupLightmapChain(hipStream_t st, const float4* sceneBlob, const SceneLayout& layout, const ptss_lightmap_params& params,
                                     const ptss_linear_params& film, const void* blocksTri, const void* blocksSph, const void* map, const void* hits,
                                     const void* chain, uint32_t n, void* out, void* info, unsigned long long* launches);
// ray queries carried through mirrors and glass (ptss_chain.hip; ptss_intersect_chain): rays = n x 32 B, hits = n x 48 B,
// chain = n x 32 B (ptss_chain_result) or nullptr, maxSteps 0 .. ptsp::kMaxSteps. No bit of ptss_launched_kernels: *launches is incremented.
// launchChain: one lane per ray, launchQuery's grid. launchChainRefill: launchPathRefill's grid and claiming; head: a 32-bit device word of
// the context for this kernel alone, set on `st` in front of the kernel
hipError_t launchChain(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* hits, void* chain,
                       uint32_t n, int maxSteps, int maxBlocks, unsigned long long* launches);
hipError_t launchChainRefill(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* hits, void* chain,
                             uint32_t n, int maxSteps, int maxWorkgroups, int numCUs, uint32_t* head, unsigned long long* launches);
// one pass of ptss_denoise (ptss_denoise.hip; PTSS_KERNEL_DENOISE of *launched). first: src is the accumulator (3 uint32 per pixel), else a colour
// plane (float4 per pixel); last: dst is the display buffer (uchar4 per pixel), else a colour plane
hipError_t launchDenoise(hipStream_t st, bool first, bool last, const void* src, void* dst, const void* features, int width, int height,
                         const ptdn::Level& level, float inverseTicks, unsigned long long* launched);
// ptss_update_triangles (ptss_update.hip). launchSceneUpdate: `count` caller records (76 B each, a device pointer) replace the
// vertices and normals of the triangles with original indices first .. first + count - 1 (PTSS_KERNEL_UPDATE of *launched); rejected: the
// device counter of records left unwritten, or nullptr not to count (the second image of a context sees the same records).
// launchMeshRefit: every leaf and group bound of a mesh image recomputed from its stored rows (PTSS_KERNEL_REFIT).
hipError_t launchSceneUpdate(hipStream_t st, float4* sceneBlob, const SceneLayout& layout, const void* records, uint32_t first, uint32_t count,
                             unsigned long long* rejected, unsigned long long* launched);
hipError_t launchMeshRefit(hipStream_t st, float4* sceneBlob, const SceneLayout& layout, unsigned long long* launched);
// ptss_resort_triangles (ptss_resort.hip; csrc/ptorder.h): the triangle rows of a mesh image put into the kd order of their current vertices,
// offTriPos and the area lights' stored positions rewritten. No bit of ptss_launched_kernels (the caller counts the call); the caller refits
// the bounds behind it (launchMeshRefit). The scratch — one allocation, about 178 B per triangle plus the sort's temporary — belongs to the
// context: reserveResortScratch allocates it, or replaces it when the triangle count has changed, BEFORE anything is launched (hipErrorOutOfMemory: nothing was touched).
struct ResortScratch {
    char* base = nullptr;
    int capacity = 0;                 // triangles
    float4* rows = nullptr;           // 8 per triangle: the gathered rows
    unsigned long long* keysIn = nullptr, *keysOut = nullptr;
    int2* seg = nullptr;              // per position: its segment [lo, hi)
    uint32_t* codes = nullptr;        // 3 x T: the centroid codes by original index, axis by axis
    int* iota = nullptr, *order = nullptr, *newPos = nullptr;
    uint32_t* extent = nullptr;       // 6 per leaf-sized slot: a segment's minima and complemented maxima
    size_t extentBytes = 0;
    void* temp = nullptr;             // the sort's temporary
    size_t tempBytes = 0;
};
hipError_t reserveResortScratch(ResortScratch& scratch, int numTriangles);
void releaseResortScratch(ResortScratch& scratch);
hipError_t launchResort(hipStream_t st, float4* sceneBlob, const SceneLayout& layout, const ResortScratch& scratch);
// ptss_reproject (ptss_reproject.hip; PTSS_KERNEL_REPROJECT of *launched): accum = 3 uint32 per pixel, features = 32 B and histories = 16 B per pixel;
// historyPrev = nullptr: no history (featuresPrev and prev are then not read)
hipError_t launchReproject(hipStream_t st, const uint32_t* accum, const void* featuresNow, const void* featuresPrev, const void* historyPrev,
                           void* historyOut, int width, int height, const ptrp::View& now, const ptrp::View& prev, const ptrp::Params& params,
                           float inverseTicks, float n, unsigned long long* launched);
// ptss_reproject_motion (PTSS_KERNEL_REPROJECT_MOTION of *launched): the same, the world point of a hit taken from motionNow (16 B per pixel)
hipError_t launchReprojectMotion(hipStream_t st, const uint32_t* accum, const void* featuresNow, const void* motionNow, const void* featuresPrev,
                                 const void* historyPrev, void* historyOut, int width, int height, const ptrp::View& now, const ptrp::View& prev,
                                 const ptrp::Params& params, float inverseTicks, float n, unsigned long long* launched);
// ptss_upsample (ptss_upsample.hip; csrc/ptupsample.h): lo = width x height RGBA words, features = 32 B per pixel of their frame, outHi = one RGBA
// word and outFloat (or nullptr) 16 B per pixel of the factor times larger frame. No bit of ptss_launched_kernels: *launches is incremented
hipError_t launchUpsample(hipStream_t st, const void* lo, const void* featuresLo, const void* featuresHi, void* outHi, void* outFloat, int width,
                          int height, int factor, const ptdn::Level& level, unsigned long long* launches);

}  // namespace ptss
