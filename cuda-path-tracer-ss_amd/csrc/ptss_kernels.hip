// ptss_kernels.hip — the hot path as hand-written HIP for gfx950 (CDNA4, 64-lane waves).
//
// Kernels (reference kernels they replace, paths relative to the reference's CudaTracer/):
//   rngInitKernel   <- curandSetupKernel            CudaTracer.cu:22-29
//   clearKernel     <- clearPixels                  CudaTracer.cu:31-49
//   bounceKernel<first> <- computeEyeRaysKernel     CudaTracer.cu:51-61, 321-343 (fused into bounce 0)
//   bounceKernel    <- pathTraceKernel + thrust::partition + the per-ray part of writeToPixelsKernel
//                                                   CudaTracer.cu:106-206, :629, :63-104
//   flushKernel     <- writeToPixelsKernel for rays still alive when the loop guard stops the frame
//                                                   CudaTracer.cu:622, :63-104
//
// Design: one ray per lane; ray state in SoA planes (coalesced 256-B wave accesses), pools cut
// into kShards regions with one live-ray counter each; the whole scene staged once per workgroup into LDS
// and read by broadcast; divergence is attacked at WAVE level, without barriers: sphere hits are resolved
// from per-lane candidate bit masks, triangle tests exit wave-uniformly, and the shadow rays of two lights
// at a time are regrouped densely through a wave-private LDS queue; live rays are compacted by the wave
// that traced them (64-bit ballot + popcount lane rank + one returning atomic per wave on the shard's
// device-resident counter, issued before the tone-mapping of the finished lanes so its round trip hides),
// so the host never reads a ray count inside a frame; a path that ends tone-maps into the integer
// accumulator right there and parks its XORWOW state in the per-pixel home record. Bounce 0 makes its own
// eye rays. Reciprocals, square roots and divisions use hardware approximation + one fma correction where
// that is proven bit-identical to IEEE (ptmath.h). No MFMA: there is no dense contraction in this path.
//
// Arithmetic mirrors oracle/oracle.cpp operation for operation (ptmath.h; -ffp-contract=off);
// every restructuring is argued exact where it is made.
//
// The device code below the kernels sits in layer headers, each including only earlier ones: ptwave.h -> ptraypool.h, ptprim.h ->
// ptaccel.h -> pthit.h -> ptshade.h. This file holds the kernels and their launches, and stays ONE translation unit: the diagnostic
// counters (ptss_diag.h) are local to it. (ptss_paths.hip, the path-query kernels, is a second translation unit over the same layers,
// with copies of its own.)
#include "ptss_device.h"
#include "ptmotion.h"
#include "ptspecular.h"
#include "pthit.h"
#include "ptshade.h"
#include "ptstrip.h"

#include <array>
#include <utility>

namespace ptss {

// =================================================================================================
// curand_init(seed, sequence, 0, ...) per stream: sequence = globalPixel * S + lane (S = 1: the pixel index,
// as the reference's `offset`, CudaTracer.cu:26-28)
__global__ void rngInitKernel(uint32_t* __restrict__ rngHome, uint32_t plane, uint32_t samples, TileMap tile, uint64_t seed,
                              const uint32_t* __restrict__ jumpTable) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = (uint32_t)tile.width * (uint32_t)tile.localRows;
    const uint32_t lane = i / plane, p = i - lane * plane;
    if (lane >= samples || p >= n) return;
    const PixelCoord pc = locate(tile, p);
    ptrng::State s = ptrng::seeded(seed);
    ptrng::skip_subsequences(s, pc.globalIndex * samples + lane, jumpTable);
    storeHome(rngHome, i, s);
}

__global__ void clearKernel(FrameBuffers fb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fb.numPixels) return;
    fb.accum[3 * i] = 0;
    fb.accum[3 * i + 1] = 0;
    fb.accum[3 * i + 2] = 0;
    if (fb.fsum)
        for (uint32_t l = 0; l < fb.samples; ++l) {
            float* fs = fb.fsum + 3u * (l * fb.plane + i);
            fs[0] = 0;
            fs[1] = 0;
            fs[2] = 0;
        }
    if (fb.pixels) fb.pixels[i] = ptss_uchar4{0, 0, 0, 0};
}

// S > 1 only: the display value of writeToPixelsKernel (CudaTracer.cu:94-98), once the pass has added all its samples
__global__ void displayKernel(FrameBuffers fb) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= fb.numPixels) return;
    U3 t = reinterpret_cast<const U3*>(fb.accum)[p];
    uint32_t l = 0;
    for (; l + 8 <= fb.samples; l += 8) {  // this pass's S samples of the pixel (finishPath), coalesced per lane plane; eight
        uint32_t q[8];                      // independent fetches in flight per thread (one at a time ran at 2.6 TB/s)
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = fb.staged[(l + k) * fb.plane + p];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            t.x += q[k] & 255u;
            t.y += (q[k] >> 8) & 255u;
            t.z += (q[k] >> 16) & 255u;
        }
    }
    for (; l < fb.samples; ++l) {
        const uint32_t q = fb.staged[l * fb.plane + p];
        t.x += q & 255u;
        t.y += (q >> 8) & 255u;
        t.z += (q >> 16) & 255u;
    }
    reinterpret_cast<U3*>(fb.accum)[p] = t;
    if (fb.pixels) {
        const uint32_t px = (uint32_t)(unsigned char)(t.x * fb.inverseTicks + 0.5f) |
                            ((uint32_t)(unsigned char)(t.y * fb.inverseTicks + 0.5f) << 8) |
                            ((uint32_t)(unsigned char)(t.z * fb.inverseTicks + 0.5f) << 16) | (255u << 24);
        reinterpret_cast<uint32_t*>(fb.pixels)[p] = px;
    }
}

// Origin-only parts of the primary-ray tests, one thread per primitive; rerun when the camera moves.
__global__ void primaryPrepKernel(float4* __restrict__ blob, SceneLayout L, vec3 origin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L.numSpheres && !L.accelSpheres) {
        const float4 sp = blob[L.offSphere + i];
        const vec3 v = origin - xyz(sp);
        blob[L.offPrimSphere + i] = float4{v.x, v.y, v.z, dot(v, v) - sp.w};
    }
    if (L.accelSpheres && i < L.numChunks) {   // the chunk test's origin part (shiftInChunkPrimary)
        const float4 b = blob[L.offChunk + i];
        const vec3 v = origin - xyz(b);
        const float x = dot(v, v) - b.w;
        blob[L.offPrimChunk + i] = float4{v.x, v.y, v.z, x - ptm::abs(x) * 2.4e-7f};   // down by more than an ulp
    }
    if (i < L.numTriangles) {
        const vec3 v0 = xyz(blob[L.offTri + 3 * i]), e1 = xyz(blob[L.offTri + 3 * i + 1]), e2 = xyz(blob[L.offTri + 3 * i + 2]);
        const vec3 s = origin - v0;
        const vec3 r = cross(s, e1);
        blob[L.offPrimTri + 2 * i] = float4{s.x, s.y, s.z, dot(e2, r)};
        blob[L.offPrimTri + 2 * i + 1] = float4{r.x, r.y, r.z, 0.0f};
    }
}

// Which primitives the eye rays of each 64-pixel strip of the context's plane can reach (ptstrip.h), one thread per strip; rerun
// with primaryPrepKernel, whenever the camera or the scene image changes. Reads the stored sphere and triangle rows, not the
// camera-origin rows primaryPrepKernel writes: the two launches do not depend on each other.
__global__ void stripMaskKernel(unsigned long long* __restrict__ masks, uint32_t numStrips, uint32_t numPixels, const float4* __restrict__ blob,
                                SceneLayout L, TileMap tile, EyeParams eye) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numStrips) return;
    const ptstrip::View view{eye.camera, eye.s, eye.aspect, eye.invW, eye.invH};
    const ptstrip::Tile t{tile.width, tile.rank, tile.world, tile.bandRows};
    masks[i] = ptstrip::stripMask(view, t, numPixels, i * ptloc::kStrip, reinterpret_cast<const float*>(blob), L);
}

// kSceneInLds = true : the scene blob is staged into LDS once per workgroup and read by broadcast
//                      (ds_read, same address in every lane; per-lane gathers in the candidate loops).
// kSceneInLds = false: the blob is read in place (scalar loads where the address is wave-uniform);
//                      scenes whose image does not fit the 64 KiB dynamic-LDS window take this path.
//
// One tile = kBlock rays = one workgroup pass:
//   1. load ray, closest hit (sphere candidate masks + uniform triangle loop), surfel, emission;
//   2. next-event estimation, kNeeLights lights per round: every lane that hit a front face draws
//      the light samples (RNG order as the reference); lanes whose Lambert term can be non-zero
//      append a shadow segment to their wave's LDS queue; the wave then traces the queue densely
//      (lane k takes entry k, k+64, ...) and posts the answers back through LDS. No barrier:
//      producer and consumer are the same wave.
//   3. scatter (lobe choice + new direction), Beer-Lambert, radiance update;
//   4. paths that ended tone-map into the accumulator; 5. survivors are compacted into the
//      shard's region of the other pool.
//
// Exactness of the shadow-ray skip (step 2): the reference adds cosI*L_i*diffuseColor*diffAvg/pi
// when the light is visible. With diffAvg == 0 or cosI == 0 that term is +-0 whenever L_i is finite
// (distance2 in (0, inf); light powers and diffuse colours are checked finite at ptss_create,
// SceneLayout::neeSkipSafe), and radiance + (+-0) == radiance, so visibility cannot change the
// result and the segment is not traced. Every other case runs the literal path.
//
// kFirst: bounce 0 makes its own rays — computeEyeRaysKernel (CudaTracer.cu:51-61, 321-343) is fused in: the
// lane fetches its pixel's random stream from the home record, draws the two jitter samples, builds the
// eye ray in registers (no ray pool read) and intersects with the camera-origin precomputes.
// kAccel: the scene image carries the chunked sphere structure (SceneLayout::accelSpheres) — its own instantiations, so
// that scenes without it run exactly the code they ran before.
// What one workgroup needs to trace one tile (bounceTile): the staged scene, this bounce's input and output regions of its
// shard, the wave's LDS queue. Built by bounceBody (one launch per bounce) and by frameKernel (one launch per frame).
struct TileEnv {
    const float4* sc;          // the scene image as the tile reads it (LDS or global)
    const float4* sceneBlob;   // ... in global memory (the many-sphere image's cold integer tables)
    const float* quantT;
    const float* in;           // this shard's region of the input pool
    float* out;                // ... of the output pool
    float* wq;                 // this wave's LDS queue
    uint32_t* wqOwner;
    unsigned char* wqAnswer;
    uint32_t shard, lane, n;   // n: rays of this shard entering the bounce
    int numLights, bounce;
};

// One tile = kBlock rays of bounce env.bounce, starting at slot / frame-tile offset `base` of the shard. kCoherentIo: the ray
// pools are read and written past the L1 (ldPlane<true>): other workgroups of the SAME launch produced / will consume them.
template <bool kLast, bool kFirst, bool kAccel, bool kBounded, bool kPairs, bool kCoherentIo, bool kMesh = false>
__device__ __forceinline__ void bounceTile(const FrameBuffers& fb, const SceneLayout& L, const TileMap& tile, const EyeParams& eye, const TileEnv& env,
                                           uint32_t base) {
    const float4* sc = env.sc;
    const float4* sceneBlob = env.sceneBlob;
    const float* quantT = env.quantT;
    const float* __restrict__ in = env.in;
    float* __restrict__ out = env.out;
    float* wq = env.wq;
    uint32_t* wqOwner = env.wqOwner;
    unsigned char* wqAnswer = env.wqAnswer;
    const uint32_t shard = env.shard, lane = env.lane, n = env.n;
    const int numLights = env.numLights, bounce = env.bounce;
    {
        const uint32_t i = base + threadIdx.x;
        uint32_t firstPixel = 0, firstLane = 0;
        bool valid = i < n;
        if constexpr (kFirst) {
            const uint32_t start = (((base / kBlock) * fb.laneCount + fb.laneIndex) * kShards + shard) * kBlock;  // frame tile -> first population index
            firstLane = start / fb.plane;                                         // wave-uniform
            firstPixel = start - firstLane * fb.plane + threadIdx.x;
            valid = firstPixel < fb.numPixels;
        }

        // ---- 1. closest hit + surfel (pathTraceKernel :121-163) -----------------------------------
        RayRegs ray;
        ray.o = ray.d = ray.L0 = ray.T = v3(0, 0, 0);
        ray.pix = 0;
        ray.active = false;
        // bounce 0: which primitives this wave's 64 pixels can reach (ptstrip.h), one word per tile at a wave-uniform address. No words
        // (nullptr): every bit set, every primitive visited
        unsigned long long strip = ptstrip::kAll;
        if constexpr (kFirst && !kAccel && kBounded && !kMesh) {
            const uint32_t waveFirst = __builtin_amdgcn_readfirstlane(firstPixel - lane);   // < fb.plane, a multiple of 64
            if (eye.strips != nullptr) strip = eye.strips[waveFirst >> 6];
        }
        if constexpr (kFirst) {
            if (valid) {
                const uint32_t pixel = firstPixel;
                // the wave's lanes hold 64 consecutive local pixels: located once per wave (ptraypool.h locateWave)
                const uint32_t waveFirst = __builtin_amdgcn_readfirstlane(firstPixel - lane);
                const PixelCoord pc = locateLane(tile, locateWave(tile, waveFirst), waveFirst, lane);
                loadHome(fb.rngHome, firstLane * fb.plane + pixel, ray.rng);
                const float jitteredX = pc.x + ptrng::uniform(ray.rng);
                const float jitteredY = pc.gy + ptrng::uniform(ray.rng);
                const vec3 start = v3(((jitteredX * eye.invW) - 0.5f) * eye.s,
                                      1 * ((jitteredY * eye.invH) - 0.5f) * eye.s * eye.aspect, 1.0f) *
                                   eye.camera.zNear;
                ray.o = eye.camera.position;
                ray.d = normalize(rotate(eye.camera.rotation, start));
                ray.L0 = v3(0, 0, 0);
                ray.T = v3(1, 1, 1);
                ray.pix = pixel | (firstLane << kLaneShift);
                ray.active = true;
            }
        } else {
            // a ray's planes are fetched where the tile first needs them (origin/direction here, the RNG state before the light
            // samples, radiance/throughput/pixel before the update): 13 fewer live registers across the closest-hit loops
            if (valid) loadRayGeometry<kCoherentIo>(tileBlock(in, base), threadIdx.x, ray);
        }
#if PTSS_ABLATE & 2
        Hit h;
        h.kind = 2; h.idx = (int)(pixOf(ray.pix) % (uint32_t)L.numTriangles); h.distance = 1.0f + ray.d.x;
        h.w0 = 0.3f; h.w1 = 0.3f; h.w2 = 0.4f;
#else
        const Hit h = closestHit<kFirst, kAccel, kBounded, kMesh>(sc, sceneBlob, L, ray.o, ray.d, valid, reinterpret_cast<uint32_t*>(wq), strip);
#endif
        const bool hit = valid && h.kind != 0;
        if constexpr (!kFirst) {
            if (valid) loadRayRng<kCoherentIo>(tileBlock(in, base), threadIdx.x, ray);
        }
        const float4* td = kMesh ? sceneBlob : sc;   // the triangle tables (global memory in the mesh image)
        vec3 point = v3(0, 0, 0), normal = v3(0, 0, 0);
        float cosI = 0;
        int materialIdx = 0;
        if (hit) {
            point = ray.o + ray.d * h.distance;  // Primitives.h:74, :100
            if (h.kind == 1) {
                normal = normalize(point - xyz(loadRow16(sc + L.offSphere + h.idx)));
                materialIdx = reinterpret_cast<const int*>((kAccel ? sceneBlob : sc) + L.offSphereMat)[h.idx];
            } else {
                const float4* nn = td + L.offTriNormal + 3 * h.idx;
                normal = (xyz(loadRow16(nn)) * h.w0 + xyz(loadRow16(nn + 1)) * h.w1) + xyz(loadRow16(nn + 2)) * h.w2;
                materialIdx = (int)asU(td[L.offTri + 3 * h.idx].w);
            }
            cosI = dot(-ray.d, normal);
        }
        const bool inside = cosI <= 0.0f;
        const bool lit = hit && !inside && !(PTSS_ABLATE & 1);  // shade() runs, :166-169
        const float4* mat = sc + L.offMaterial + 5 * materialIdx;

        // ---- 2. shade(), CudaTracer.cu:345-390: kNeeLights lights per round through the wave queue ----
        vec3 radiance = v3(0, 0, 0);
        for (int l0 = 0; l0 < numLights; l0 += kNeeLights) {
            uint32_t queued = 0;  // wave-uniform
            bool need[kNeeLights];
            float cosL[kNeeLights], distance2[kNeeLights];
            [[maybe_unused]] vec3 pairW[kNeeLights];      // kPairs: the round's segments stay in registers until both are known
            [[maybe_unused]] float pairReach[kNeeLights];
#pragma unroll
            for (int k = 0; k < kNeeLights; ++k) {
                need[k] = false;
                cosL[k] = 0;
                distance2[k] = 0;
                pairW[k] = v3(0, 0, 0);
                pairReach[k] = 0;
                const int li = l0 + k;
                if (li >= numLights) continue;  // uniform
                vec3 lo = v3(0, 0, 0), w_i = v3(0, 0, 0);
                float distance = 0;
                if (lit) {
                    vec3 lightPoint;
                    if (li < L.numPointLights) {
                        lightPoint = xyz(loadRow16(sc + L.offPointLight + 2 * li));
                    } else {  // getAreaLightPoint :392-418 — four draws whether or not the light ends up visible
                        const float4 light = sc[L.offAreaLight + 2 * (li - L.numPointLights)];
                        const float u1 = ptrng::uniform(ray.rng);
                        const float u2 = ptrng::uniform(ray.rng);
                        const float u3 = ptrng::uniform(ray.rng);
                        // 1 / (u1+u2+u3), :403. Each uniform is k 2^-32 + 2^-33 rounded, in [2^-33, 1]: the sum lies in [2^-32, 3],
                        // inside the reciprocal's fast range [2^-125, 2^126) — no guard
                        const float inverseTotal = ptm::rcp_in_range(u1 + u2 + u3);
                        const float weight0 = u1 * inverseTotal, weight1 = u2 * inverseTotal, weight2 = u3 * inverseTotal;
                        // triangleIdx or triangleIdx + 1, :408 — as stored positions (the triangles may be stored grouped by class)
                        const int tri = (ptrng::uniform(ray.rng) > .5f) ? (int)asU(light.w) : (int)asU(sc[L.offAreaLight + 2 * (li - L.numPointLights) + 1].x);
                        const vec3 a = xyz(loadRow16(td + L.offTri + 3 * tri));
                        const vec3 b = xyz(loadRow16(td + L.offTriVert + 2 * tri));
                        const vec3 c = xyz(loadRow16(td + L.offTriVert + 2 * tri + 1));
                        lightPoint = (a * weight0 + b * weight1) + c * weight2;
                    }
                    // head of lineOfSight :423-432
                    const vec3 offset = lightPoint - point;
                    lightSample(offset, distance2[k], distance, w_i);
                    cosL[k] = ptm::max(0.0f, dot(normal, w_i));
                    const bool zeroTerm = L.neeSkipSafe && (distance2[k] > 0.0f) && (distance2[k] < ptm::inf()) &&
                                          (cosL[k] == 0.0f || mat[0].w == 0.0f);
                    need[k] = !zeroTerm;
                    lo = point + (ptm::kRayBump * normal);
                    distance -= 2 * ptm::kRayBump;
                }
                if constexpr (kPairs) {
                    pairW[k] = w_i;
                    pairReach[k] = distance;
                    continue;
                }
                const unsigned long long m = __ballot(need[k]);
                if (need[k]) {
                    const uint32_t slot = queued + __popcll(m & ((1ull << lane) - 1ull));
                    wq[0 * kQueueCap + slot] = lo.x;
                    wq[1 * kQueueCap + slot] = lo.y;
                    wq[2 * kQueueCap + slot] = lo.z;
                    wq[3 * kQueueCap + slot] = w_i.x;
                    wq[4 * kQueueCap + slot] = w_i.y;
                    wq[5 * kQueueCap + slot] = w_i.z;
                    wq[6 * kQueueCap + slot] = distance;
                    wqOwner[slot] = lane | ((uint32_t)k << 8);
                    wqAnswer[k * 64 + lane] = 0;
                }
                queued += (uint32_t)__popcll(m);
            }
            PTSS_DIAG_PAIRS(need[0], need[1], lit);
            waveLdsFence();
            PTSS_DIAG_QUEUE(queued);
            if constexpr (kPairs) {
                // One entry per lane that needs either segment: origin, the two directions and reaches, owner lane | need bits << 8
                // (12 planes of 64). A pass is sized by what it holds: 49+ entries one lane each, fewer -> 32 / 16 / 8 entries
                // with 2 / 4 / 8 lanes sharing the primitive list.
                constexpr int kPairCap = 64;
                const bool needAny = need[0] || need[1];
                const unsigned long long m = __ballot(needAny);
                const uint32_t pairs = (uint32_t)__popcll(m);
                uint32_t* pairOwner = reinterpret_cast<uint32_t*>(wq + 11 * kPairCap);
                if (needAny) {
                    const uint32_t slot = __popcll(m & ((1ull << lane) - 1ull));
                    const vec3 lo = point + (ptm::kRayBump * normal);
                    wq[0 * kPairCap + slot] = lo.x;
                    wq[1 * kPairCap + slot] = lo.y;
                    wq[2 * kPairCap + slot] = lo.z;
                    wq[3 * kPairCap + slot] = pairW[0].x;
                    wq[4 * kPairCap + slot] = pairW[0].y;
                    wq[5 * kPairCap + slot] = pairW[0].z;
                    wq[6 * kPairCap + slot] = pairReach[0];
                    wq[7 * kPairCap + slot] = pairW[1].x;
                    wq[8 * kPairCap + slot] = pairW[1].y;
                    wq[9 * kPairCap + slot] = pairW[1].z;
                    wq[10 * kPairCap + slot] = pairReach[1];
                    pairOwner[slot] = lane | ((need[0] ? 1u : 0u) << 8) | ((need[1] ? 1u : 0u) << 9);
                    wqAnswer[0 * 64 + lane] = 0;
                    wqAnswer[1 * 64 + lane] = 0;
                }
                waveLdsFence();
                for (uint32_t e0 = 0; e0 < pairs;) {
                    const uint32_t rem = pairs - e0;
                    const uint32_t units = (rem + 7u) >> 3;
                    const int chunkLog = (units >= 7u) ? 6 : (units >= 4u ? 5 : (units >= 2u ? 4 : 3));
                    const int shift = 6 - chunkLog;
                    const uint32_t mine = lane >> shift;
                    const uint32_t sub = lane & ((1u << shift) - 1u);
                    const bool have = mine < rem;
                    const uint32_t es = have ? e0 + mine : 0u;
                    const vec3 lo = v3(wq[0 * kPairCap + es], wq[1 * kPairCap + es], wq[2 * kPairCap + es]);
                    const vec3 wA = v3(wq[3 * kPairCap + es], wq[4 * kPairCap + es], wq[5 * kPairCap + es]);
                    const float dA = wq[6 * kPairCap + es];
                    const vec3 wB = v3(wq[7 * kPairCap + es], wq[8 * kPairCap + es], wq[9 * kPairCap + es]);
                    const float dB = wq[10 * kPairCap + es];
                    const uint32_t ow = pairOwner[es];
                    const bool liveA = have && ((ow >> 8) & 1u) != 0u, liveB = have && ((ow >> 9) & 1u) != 0u;
                    bool occA, occB;
                    if (shift == 0) pairAnyHit<kBounded, false>(sc, L, lo, wA, dA, liveA, wB, dB, liveB, 0, 0, occA, occB);
                    else pairAnyHit<kBounded, true>(sc, L, lo, wA, dA, liveA, wB, dB, liveB, shift, (int)sub, occA, occB);
                    const unsigned long long verdictsA = __ballot(occA), verdictsB = __ballot(occB);
                    const unsigned long long group = ((1ull << (1u << shift)) - 1ull) << (mine << shift);
                    if (have && sub == 0u) {
                        if ((verdictsA & group) != 0ull) wqAnswer[0 * 64 + (ow & 63u)] = 1;
                        if ((verdictsB & group) != 0ull) wqAnswer[1 * 64 + (ow & 63u)] = 1;
                    }
                    e0 += 1u << chunkLog;
                }
            } else {
            // Passes over the wave's queue, each sized by what is left (wave-uniform): 49+ segments -> a dense pass,
            // one lane per segment (anyHit, broadcast rows); fewer -> a chunk of 32 / 16 / 8 segments with 2 / 4 / 8
            // lanes per segment sharing the primitive list (anyHitSplit), so that a pass costs about what it holds:
            // 77 segments = 1 + 1/4 dense passes instead of 2, 13 segments = 1/4 instead of 1.
            for (uint32_t e0 = 0; e0 < queued;) {
                const uint32_t rem = queued - e0;
                const uint32_t units = (rem + 7u) >> 3;  // of 8 segments
                // (the chunked sphere traversal is per lane already: those scenes take dense passes only)
                const int chunkLog = (units >= 7u || kAccel || kMesh) ? 6 : (units >= 4u ? 5 : (units >= 2u ? 4 : 3));
                const int shift = 6 - chunkLog;                      // lanes per segment = 1 << shift
                const uint32_t mine = lane >> shift;                 // this lane's segment within the chunk
                const uint32_t sub = lane & ((1u << shift) - 1u);    // its share of the primitive list
                const bool have = mine < rem;
                const uint32_t es = have ? e0 + mine : 0u;
                const vec3 lo = v3(wq[0 * kQueueCap + es], wq[1 * kQueueCap + es], wq[2 * kQueueCap + es]);
                const vec3 wi = v3(wq[3 * kQueueCap + es], wq[4 * kQueueCap + es], wq[5 * kQueueCap + es]);
                const float reach = wq[6 * kQueueCap + es];
                bool occ;
                if (kAccel && (e0 != 0u || queued <= 64u)) {  // dense pass whose OTHER half of the queue planes is free
                    occ = anySpheresHybrid(sc, L, wq + e0, wq + (e0 == 0u ? 64 : 0), lo, wi, reach, have);
                    occ = occ || anyTriangles(sc, L, lo, wi, reach, have && !occ);
                } else {
                    occ = (shift == 0) ? anyHit<kAccel, kBounded, kMesh>(sc, L, lo, wi, reach, have, sceneBlob)
                                       : anyHitSplit<kBounded>(sc, L, lo, wi, reach, have, shift, (int)sub);
                }
                const unsigned long long verdicts = __ballot(occ);  // all lanes vote before anyone branches
                const unsigned long long group = ((1ull << (1u << shift)) - 1ull) << (mine << shift);
                if (have && sub == 0u && (verdicts & group) != 0ull) {
                    const uint32_t ow = wqOwner[es];
                    wqAnswer[(ow >> 8) * 64 + (ow & 63u)] = 1;
                }
                e0 += 1u << chunkLog;
            }
            }
            waveLdsFence();
#pragma unroll
            for (int k = 0; k < kNeeLights; ++k) {
                const int li = l0 + k;
                if (li >= numLights) continue;
                if (need[k] && wqAnswer[k * 64 + lane] == 0) {
                    const vec3 power = (li < L.numPointLights) ? xyz(loadRow16(sc + L.offPointLight + 2 * li + 1))
                                                               : xyz(loadRow16(sc + L.offAreaLight + 2 * (li - L.numPointLights)));
                    addLambertTerm(radiance, cosL[k], power, distance2[k], mat[0], (fb.guardFlags & kGuardLightPowers) != 0u);
                }
            }
            waveLdsFence();
        }

        // ---- 3. scatter + radiance update (pathTraceKernel :172-198) -------------------------------
        bool alive = false;
        if constexpr (!kFirst) {
            if (valid) loadRayRadiance<kCoherentIo>(tileBlock(in, base), threadIdx.x, ray);
        }
        if (valid) {
            if (hit) {
                // emmitance, :163 — read here, after the shadow passes, instead of being held in registers across them
                vec3 directRadiance = v3(0, 0, 0) + xyz(mat[3]);
                if (lit) directRadiance = directRadiance + radiance;
                vec3 indirectRadiance = v3(1, 1, 1);
                if (!kLast && !(PTSS_ABLATE & 4)) indirectRadiance = scatter(mat, ray, point, normal, cosI, fb.guardFlags);
                if (inside) {  // Beer-Lambert, :179-185
                    const float4 ab = mat[2];
                    ray.T = ray.T * v3(ptm::exp(-h.distance * ab.x), ptm::exp(-h.distance * ab.y),
                                       ptm::exp(-h.distance * ab.z));
                }
                ray.L0 = ray.L0 + ray.T * directRadiance;
                ray.T = ray.T * indirectRadiance;
            } else {  // :193-198
                const vec3 dc = v3(fb.defaultColor[0], fb.defaultColor[1], fb.defaultColor[2]);
                ray.L0 = ray.L0 + dc * ray.T;
                ray.active = false;
            }
            alive = ray.active && !kLast;
        }

        // ---- 4+5. stream compaction of the survivors (replaces thrust::partition, :629) and
        // writeToPixelsKernel for the paths that ended. Each wave compacts on its own — 64-bit ballot, popcount lane rank, ONE
        // returning atomic per wave on the shard's counter (16 counters share the load) — no barrier; the atomic is issued
        // first so that its round trip hides behind the tone-mapping of the finished lanes.
        uint32_t slot = 0;
        if constexpr (!kLast) {
            const unsigned long long live = __ballot(alive);
            if (live) {
                const int leader = __ffsll((long long)live) - 1;
                uint32_t base0 = 0;
                if ((int)lane == leader)
                    base0 = atomicAdd(&fb.counts[countIndex(bounce + 1, (int)shard)], (uint32_t)__popcll(live));
                slot = base0;  // consumed after the finish work below
                if (valid && !alive && !(PTSS_ABLATE & 8)) finishPath(fb, ray, quantT);
                slot = __shfl(slot, leader) + __popcll(live & ((1ull << lane) - 1ull));
                if (alive) storeRay<kCoherentIo>(out, slot, ray);
            } else if (valid && !(PTSS_ABLATE & 8)) {
                finishPath(fb, ray, quantT);
            }
        } else {
            if (valid && !(PTSS_ABLATE & 8)) finishPath(fb, ray, quantT);
        }
    }
}

template <bool kLast, bool kSceneInLds, bool kFirst, bool kAccel, bool kBounded, bool kPairsWanted, bool kMesh>
__device__ __forceinline__ void bounceBody(const FrameBuffers& fb, const float4* __restrict__ sceneBlob, const SceneLayout& L, int bounce,
                                           const TileMap& tile, const EyeParams& eye) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    constexpr bool kPairs = kPairsWanted && !kAccel;   // the two shadow segments of a surface point travel and are tested together (SceneLayout::neePairs)
    const uint32_t shard = blockIdx.x % kShards;
    const uint32_t n = fb.counts[countIndex(bounce, (int)shard)];  // this shard's live rays (of this lane)
    if constexpr (kFirst) {
        if (fb.frameRays <= fb.minLive) return;  // loop guard, CudaTracer.cu:622: the frame starts with <= 128 rays
    } else {
        if (n == 0) return;  // nothing of this shard reached this bounce (whatever the guard says)
        if (n <= fb.minLive) {  // loop guard on the FRAME's live count (device-side; every workgroup that has work reaches
            uint32_t own = 0;   // the same verdict). Only a nearly empty shard has to add up; only a nearly empty LANE asks its peers.
            for (int s = 0; s < kShards; ++s) own += fb.counts[countIndex(bounce, s)];
            if (own <= fb.minLive && frameLiveCount(fb, bounce, own, fb.peerTarget) <= fb.minLive) return;
        }
    }

    const uint32_t lane = __lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    float4* work = lds + (kSceneInLds ? L.ldsVec4 : 0);
    float* wq = reinterpret_cast<float*>(work + kBlockScratchVec4) + wave * kWaveLdsWords;  // this wave's queue
    uint32_t* wqOwner = reinterpret_cast<uint32_t*>(wq + 7 * kQueueCap);
    unsigned char* wqAnswer = reinterpret_cast<unsigned char*>(wqOwner + kQueueCap);  // [kNeeLights][64], 0 / 1

    const float4* sc;
    if constexpr (kSceneInLds) {
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    const float* quantT = reinterpret_cast<const float*>(sc + L.offQuant);

    const size_t regionWords = (size_t)fb.regionCap * kRayPlanes;
    const float* __restrict__ in = fb.pool[bounce & 1] + shard * regionWords;  // this shard's region
    float* __restrict__ out = fb.pool[(bounce + 1) & 1] + shard * regionWords;
    const int numLights = L.numPointLights + L.numAreaLights;
    const TileEnv env{sc, sceneBlob, quantT, in, out, wq, wqOwner, wqAnswer, shard, lane, n, numLights, bounce};

    // one tile per workgroup when the host's grid hint is right; grid-stride keeps any n correct
    // bounce 0 walks the FRAME's tiles (S sample planes of fb.plane pixels; tile t belongs to shard t % kShards),
    // every later bounce walks the shard's compacted region
    // (with frame lanes: round R of the frame belongs to lane R % laneCount, whose round R / laneCount it is)
    const uint32_t roundsOfShard = (fb.firstTiles + kShards - 1 - shard) / kShards;
    const uint32_t span = kFirst ? ((roundsOfShard + fb.laneCount - 1 - fb.laneIndex) / fb.laneCount) * kBlock : n;
    for (uint32_t base = (blockIdx.x / kShards) * kBlock; base < span; base += (gridDim.x / kShards) * kBlock) {
        bounceTile<kLast, kFirst, kAccel, kBounded, kPairs, false, kMesh>(fb, L, tile, eye, env, base);
    }
}

template <bool kLast, bool kSceneInLds, bool kFirst, bool kAccel, bool kBounded, bool kPairs, bool kMesh>
__global__ __launch_bounds__(kBlock, (kAccel || kMesh) ? 4 : (kFirst ? PTSS_MINWAVES_FIRST : (kBounded ? PTSS_MINWAVES_BOUNDED : PTSS_MINWAVES))) void bounceKernel(  // chunked scenes: their LDS image (21 KB + the work area) admits four workgroups per CU, so four waves per SIMD = 128 registers cost nothing (round 3: 5 -> 4, no scratch, c5 +2.8 %)
    FrameBuffers fb, const float4* __restrict__ sceneBlob, SceneLayout L, int bounce, TileMap tile, EyeParams eye) {
    bounceBody<kLast, kSceneInLds, kFirst, kAccel, kBounded, kPairs, kMesh>(fb, sceneBlob, L, bounce, tile, eye);
    // frame lanes: "this workgroup of bounce `bounce` has ended" (every workgroup, also one that had nothing to do) — the
    // peers' loop guard of bounce + 1 waits for the whole grid (frameLiveCount). The survivor counters were raised by
    // returning device-scope atomics, so they have been performed when a wave gets here, and the barrier collects the
    // workgroup's waves: a relaxed add is enough. (A RELEASE here writes the XCD's L2 back once per workgroup: 3x slower.)
    if (fb.numPeers != 0) {
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_fetch_add(fb.myDone + countIndex(bounce, (int)(blockIdx.x % kShards)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- ONE LAUNCH PER FRAME (frames whose bounce-0 tiles are all resident at once: up to ~3 * 2^17 rays per pass) -------------
// A pass of a small frame is up to 16 launches that are each at most one resident round wide: such a launch costs what ONE
// tile costs from end to end (~15 us at 512 x 512: scene staging, ray fetch, ~3,300 dependent instructions, the counter
// round trip) whatever the machine could do meanwhile. Here workgroup w = (shard s = w % kShards, tile j =
// w / kShards) stays: it stages the scene once, traces bounce-0 tile j of its shard, and then, bounce after bounce, tile j of
// the shard's compacted region for as long as that tile exists (a region never grows, so a workgroup that finds its tile
// beyond the count is done for good).
// Hand-off between the bounces of ONE shard (the only dependency: survivors are compacted per shard): every workgroup that
// traced a tile of bounce b adds 1 to done[b][s] — word kDoneWord of the (b, s) counter line — after its waves have drained
// their stores (s_waitcnt vmcnt(0), workgroup barrier); a workgroup goes on to bounce b + 1 when done[b][s] has reached the
// tiles the shard had at bounce b (it knows: ceil(n_s(b) / 256)), and then reads n_s(b + 1), raised by returning atomics
// before those arrivals. The rays themselves cross between workgroups through sc1 accesses (ldPlane<true> / stPlane<true>):
// written through, read past the L1 — MI355X_MICROARCH.md's hand-off "one lane of each storing workgroup signals by an
// agent-scope atomic add, the consumer polls that counter with sc1 loads, payload stored and loaded sc1" (no L2 write-back,
// no L1 invalidate per bounce). The loop guard `numRays > 128` (CudaTracer.cu:622) is a whole-frame count: a workgroup whose
// shard still holds more than 128 rays knows the frame does; otherwise lanes 0..15 of its first wave each follow one shard's
// chain of done counters up to this bounce (a few loads, progress kept in registers) and add the shards' counts up.
// Deadlock freedom: the host launches this kernel only when the whole grid is resident at once (ptss_api.hip), so every
// workgroup a waiter depends on is running or has finished; every wait is bounded all the same (peerWaitExpired) and a
// workgroup whose wait expires leaves — the host then reports PTSS_ETIMEOUT.
constexpr int kDoneWord = 1;
// the whole-frame guard adds the shards' counts up across lanes 0..kShards-1 of one wave with a butterfly
static_assert((kShards & (kShards - 1)) == 0 && kShards <= 64, "frameKernel's guard needs a power-of-two shard count of at most 64");

__device__ __forceinline__ bool waitForCount(const uint32_t* word, uint32_t target) {   // bounded; true = reached
    unsigned long long since = 0ull;
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        __builtin_amdgcn_s_sleep(8);
        if (peerWaitExpired(since)) return false;
    }
    return true;
}

template <bool kAccel, bool kBounded, bool kPairsWanted>
__global__ __launch_bounds__(kBlock, kAccel ? 4 : (kBounded ? PTSS_MINWAVES_BOUNDED : PTSS_MINWAVES)) void frameKernel(
    FrameBuffers fb, const float4* __restrict__ sceneBlob, SceneLayout L, int numBounces, TileMap tile, EyeParams eye) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    constexpr bool kPairs = kPairsWanted && !kAccel;
    if (fb.frameRays <= fb.minLive) return;   // loop guard at bounce 0: the frame starts with <= 128 rays
    const uint32_t shard = blockIdx.x % kShards, myTile = blockIdx.x / kShards;
    const uint32_t rounds = (fb.firstTiles + kShards - 1 - shard) / kShards;   // bounce-0 tiles of this shard
    if (myTile >= rounds) return;

    const uint32_t lane = __lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    float4* work = lds + L.ldsVec4;
    uint32_t* bcast = reinterpret_cast<uint32_t*>(work);   // [0] rays of this shard entering the next bounce (~0u: give up), [1] the frame's
    float* wq = reinterpret_cast<float*>(work + kBlockScratchVec4) + wave * kWaveLdsWords;
    uint32_t* wqOwner = reinterpret_cast<uint32_t*>(wq + 7 * kQueueCap);
    unsigned char* wqAnswer = reinterpret_cast<unsigned char*>(wqOwner + kQueueCap);
    for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];   // the scene, once per frame
    __syncthreads();
    const size_t regionWords = (size_t)fb.regionCap * kRayPlanes;
    TileEnv env{lds, sceneBlob, reinterpret_cast<const float*>(lds + L.offQuant), nullptr, nullptr, wq, wqOwner, wqAnswer, shard, lane, 0u,
                L.numPointLights + L.numAreaLights, 0};
    uint32_t tilesNow = rounds, raysNow = 0;
    // the guard's view of the other shards (lanes 0..15 of wave 0, one shard each): the next bounce to verify, -1 = that shard is empty
    int verified = 0;
    for (int b = 0; b < numBounces; ++b) {
        const bool last = b == numBounces - 1;
        env.bounce = b;
        env.n = raysNow;
        env.in = fb.pool[b & 1] + shard * regionWords;
        env.out = fb.pool[(b + 1) & 1] + shard * regionWords;
        const uint32_t base = myTile * kBlock;
        if (b == 0) {
            if (last) bounceTile<true, true, kAccel, kBounded, kPairs, true>(fb, L, tile, eye, env, base);
            else bounceTile<false, true, kAccel, kBounded, kPairs, true>(fb, L, tile, eye, env, base);
        } else if (last) {
            bounceTile<true, false, kAccel, kBounded, kPairs, true>(fb, L, tile, eye, env, base);
        } else {
            bounceTile<false, false, kAccel, kBounded, kPairs, true>(fb, L, tile, eye, env, base);
        }
        if (last) break;
        // publish this tile (its survivors are in the output region, the shard's next count was raised by returning atomics) ...
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __hip_atomic_fetch_add(fb.counts + countIndex(b, (int)shard) + kDoneWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // ... and wait for the shard's other tiles of this bounce; n_s(b + 1) is final once those arrivals are complete
            const uint32_t* done = fb.counts + countIndex(b, (int)shard) + kDoneWord;
            uint32_t next = ~0u;
            unsigned long long since = 0ull;
            for (;;) {
                if (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= tilesNow) {
                    next = __hip_atomic_load(fb.counts + countIndex(b + 1, (int)shard), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
                if (peerWaitExpired(since)) {
                    atomicAdd(fb.guardTimeouts, 1u);
                    break;
                }
            }
            bcast[0] = next;
        }
        __syncthreads();
        const uint32_t next = bcast[0];
        if (next == ~0u) return;
        if (myTile * kBlock >= next) return;   // no tile of bounce b + 1 for this workgroup, nor of any later bounce
        if (next <= fb.minLive) {   // the loop guard is the FRAME's count: ask the other shards (wave 0, one lane per shard)
            if (wave == 0) {
                uint32_t theirs = 0;
                bool ok = true;
                if (lane < kShards) {
                    const int s = (int)lane;
                    while (verified >= 0 && verified <= b) {   // every bounce up to b of shard s must have ended before its count of b + 1 is final
                        const uint32_t tiles = verified == 0 ? (fb.firstTiles + kShards - 1 - (uint32_t)s) / kShards
                                                             : (__hip_atomic_load(fb.counts + countIndex(verified, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + kBlock - 1) / kBlock;
                        if (tiles == 0) {
                            verified = -1;   // nothing of shard s reached this bounce: nothing ever will
                        } else if (waitForCount(fb.counts + countIndex(verified, s) + kDoneWord, tiles)) {
                            ++verified;
                        } else {
                            ok = false;
                            break;
                        }
                    }
                    if (verified > b) theirs = __hip_atomic_load(fb.counts + countIndex(b + 1, s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                uint32_t total = theirs;
#pragma unroll
                for (int off = kShards / 2; off >= 1; off >>= 1) total += (uint32_t)__shfl_xor((int)total, off);
                const bool allOk = __builtin_amdgcn_ballot_w64(!ok) == 0ull;
                if (lane == 0) {
                    if (!allOk) atomicAdd(fb.guardTimeouts, 1u);
                    bcast[1] = allOk ? total : 0u;   // a wait that expired: leave (as if the guard had stopped the frame)
                }
            }
            __syncthreads();
            if (bcast[1] <= fb.minLive) return;
        }
        tilesNow = (next + kBlock - 1) / kBlock;
        raysNow = next;
    }
}

// After the last launched bounce: tone-map whatever the loop guard left alive (<= 128 rays in all
// shards together), and add this frame's ray-bounce total to the running counter.
__global__ void flushKernel(FrameBuffers fb, int numBounces, FlushTargets targets) {
    __shared__ uint32_t totals[kMaxBounces + 1];
    __shared__ int stopShared;
    for (int b = threadIdx.x; b <= numBounces; b += blockDim.x) {
        uint32_t total = 0;
        for (int s = 0; s < kShards; ++s) total += fb.counts[countIndex(b, s)];
        totals[b] = total;  // this lane's rays entering bounce b
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // where did the frame's loop guard stop? (the bounce kernels decided the same way)
        int stop = numBounces;
        unsigned long long sum = 0;
        for (int b = 0; b < numBounces; ++b) {
            uint32_t frame = totals[b];
            if (frame <= fb.minLive) {
                if (b == 0) {
                    frame = fb.frameRays;
                } else {
                    uint32_t want[kMaxLanes - 1];
                    for (int p = 0; p < kMaxLanes - 1; ++p) want[p] = targets.target[p][b - 1];
                    frame = frameLiveCount(fb, b, frame, want);
                }
            }
            if (frame <= fb.minLive) {
                stop = b;
                break;
            }
            sum += totals[b];
        }
        *fb.totalRayBounces += sum;  // this lane's slot
        stopShared = stop;
    }
    __syncthreads();
    const int stop = stopShared;
    const uint32_t i = threadIdx.x;
    if (stop == 0) {
        // Not even bounce 0 ran (<= 128 rays in the frame). Eye rays are made inside bounce 0, so there are
        // none in the pool: do what computeEyeRaysKernel + writeToPixelsKernel would have done to each pixel —
        // two jitter draws, then a sample of radiance 0. (Lane 0 does it for the whole frame.)
        if (fb.laneIndex == 0 && i < fb.numPixels)
            for (uint32_t l = 0; l < fb.samples; ++l) {
                RayRegs ray;
                loadHome(fb.rngHome, l * fb.plane + i, ray.rng);
                (void)ptrng::uniform(ray.rng);
                (void)ptrng::uniform(ray.rng);
                ray.L0 = v3(0, 0, 0);
                ray.pix = i | (l << kLaneShift);
                finishPath(fb, ray, fb.quantTable);
            }
    } else if (stop < numBounces && totals[stop] != 0) {  // the guard left this lane's rays alive: writeToPixelsKernel for them
        for (int s = 0; s < kShards; ++s) {
            // n <= 128 = blockDim.x here by the guard that stopped the loop; clamped all the same, and a slot whose pixel
            // or sample lane is out of range is skipped rather than written through: a stale slot must never be able to
            // fault the device (a GPU memory fault aborts the calling process — DESIGN.md §4a, the round-1 abort)
            uint32_t n = fb.counts[countIndex(stop, s)];
            n = n < blockDim.x ? n : blockDim.x;
            if (i < n) {
                RayRegs ray;
                loadRay(tileBlock(fb.pool[stop & 1] + (size_t)s * fb.regionCap * kRayPlanes, (i / kBlock) * kBlock), i % kBlock, ray);
                if (pixOf(ray.pix) < fb.numPixels && laneOf(ray.pix) < fb.samples) finishPath(fb, ray, fb.quantTable);
            }
        }
    }
    // keep this frame's counters for the host (live counts, grid hints) and arm the OTHER buffer for the next frame:
    // bounce 0 = the shard's pixels, every later bounce 0. This frame's buffer stays as it is: a peer lane may still read it.
    // The other buffer is the one of the frame before this: a peer that runs a frame behind may still be reading it, so
    // wait until every peer has finished that frame (its flushKernel was enqueued before this one: no deadlock in a shared queue).
    if (threadIdx.x == 0)
        for (uint32_t p = 0; p < fb.numPeers; ++p) {
            unsigned long long since = 0ull;
            while ((int32_t)(__hip_atomic_load(fb.peerFrameDone[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - fb.frameSeq) < 0) {
                __builtin_amdgcn_s_sleep(64);
                if (peerWaitExpired(since)) {
                    atomicAdd(fb.guardTimeouts, 1u);
                    break;
                }
            }
        }
    __syncthreads();
    // (every bounce slot, not just this frame's: the other buffer still holds the counts of two frames ago, and the
    // bounce count may change between frames — ptss_set_mode, ptss_set_max_iterations)
    for (int k = threadIdx.x; k < (kMaxBounces + 1) * kShards; k += blockDim.x) {
        const int b = k / kShards, s = k % kShards;
        fb.lastCounts[countIndex(b, s)] = (b <= numBounces) ? fb.counts[countIndex(b, s)] : 0u;
        fb.countsNext[countIndex(b, s)] = (b == 0) ? fb.shardCount0[s] : 0u;
        fb.countsNext[countIndex(b, s) + kDoneWord] = 0u;   // frameKernel's finished-tiles counter of that line
    }
    // This lane has finished the frame: every read of a peer's counters (thread 0, above) has returned by now, and what this
    // kernel wrote — finishPath's accumulator / pixel / float-sum / RNG words of the leftover rays, lastCounts, countsNext, the
    // ray-bounce total — is PUBLISHED before the frame-done word: every wave drains its stores, the workgroup meets, and one
    // lane writes this XCD's L2 back (agent-scope release; once per frame and lane, in a 128-thread kernel) before it stores
    // the word. The join below depends on that: the caller's stream is ordered behind the LAST lane's flush only, and the
    // end-of-kernel write-back of that kernel covers its own XCD's L2, not the one a peer's flush ran on.
    if (fb.numPeers != 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            if (fb.joinsFrame) {  // the last lane's flush ends only when the whole frame has (the join event sits behind it)
                for (uint32_t p = 0; p < fb.numPeers; ++p) {
                    unsigned long long since = 0ull;
                    while ((int32_t)(__hip_atomic_load(fb.peerFrameDone[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - (fb.frameSeq + 1u)) < 0) {
                        __builtin_amdgcn_s_sleep(64);
                        if (peerWaitExpired(since)) {
                            atomicAdd(fb.guardTimeouts, 1u);
                            break;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // one poll loop per peer, then ONE acquire
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the write-back has completed before the word goes out (hipcc may drop the fence's own wait)
            __hip_atomic_store(fb.myFrameDone, fb.frameSeq + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- BATCHED RAY QUERIES (ptss_intersect / ptss_occluded) ---------------------------------------------------
// One lane per query ray, kBlock rays per workgroup, grid-strided; the scene image is staged as bounceBody stages it. Neither kernel
// reads the per-camera rows (offPrim*) nor any frame buffer: a query may run beside the frames of the same context.
// Occlusion: lineOfSight's loop (CudaTracer.cu:434-452) is an OR over independent tests, so anyHit's order-free loops answer it
// for the images whose sphere tests are the literal ones (plain, mesh); the sorted many-sphere image's chunk tests assume origins
// in the scene's range, so there the same loop walks its stored sphere rows instead of the chunks.
// (Diagnostic builds: anyHit's candidate counter, PTSS_DIAG bit 0 slot 4, also counts the occlusion queries' sphere candidates.)
template <bool kAny, bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void queryKernel(const float4* __restrict__ sceneBlob, SceneLayout L, const float4* __restrict__ rays,
                                                       float4* __restrict__ out, uint32_t n) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    const float4* sc;
    if constexpr (kSceneInLds) {
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    const bool mesh = meshImage(L);
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool live = i < n;
        float4 r0 = float4{0, 0, 0, 0}, r1 = float4{0, 0, 0, 0};
        if (live) {
            r0 = rays[2 * (size_t)i];
            r1 = rays[2 * (size_t)i + 1];
        }
        const vec3 o = xyz(r0), d = xyz(r1);
        const float tmax = r0.w;
        if constexpr (kAny) {
            const bool blocked = anyQuery(sc, sceneBlob, L, mesh, o, d, tmax, live);   // (pthit.h: the dispatch by image kind)
            if (live) reinterpret_cast<uint32_t*>(out)[i] = blocked ? 1u : 0u;
        } else {
            const QueryHit q = closestQuery(sc, sceneBlob, L, o, d, tmax, live);
            if (live) {
                float4* h = out + 3 * (size_t)i;
                h[0] = float4{q.point.x, q.point.y, q.point.z, q.dist};
                h[1] = float4{q.normal.x, q.normal.y, q.normal.z, asF((uint32_t)q.materialIdx)};
                h[2] = float4{asF((uint32_t)q.kind), asF((uint32_t)q.prim), q.w1, q.w2};
            }
        }
    }
}

// ---- FIRST-HIT FEATURES (ptss_render_features) --------------------------------------------------------------
// One lane per local pixel: the eye ray through the pixel's centre with bounce 0's operations (bounceTile, kFirst; a jitter of
// 0.5 in place of the two random draws), then closestQuery with tmax = +inf. Like the queries it reads the scene image only.
// kMotion (ptss_render_features_motion): the same trace also answers where the hit point was in the previous pose
// (csrc/ptmotion.h), one 16-byte row per pixel. Only lanes that hit a triangle of the moved range read a previous record — nine
// words of a 76-byte record that is only 4-byte aligned (hipcc emits two 16-byte loads and a 4-byte one, which gfx950 serves at
// that alignment) — so a wave over static surfaces issues none; neighbouring lanes mostly hit the same or neighbouring triangles,
// whose records share cache lines. Without kMotion the argument is empty.
template <bool kMotion>
struct FeatureMotion {};
template <>
struct FeatureMotion<true> {
    const float* prevRecords;   // `count` records of 19 words: the previous pose of triangles first .. first + count - 1
    uint32_t first, count;
    float4* out;
};

template <bool kSceneInLds, bool kMotion = false>
__global__ __launch_bounds__(kBlock) void featureKernel(const float4* __restrict__ sceneBlob, SceneLayout L, TileMap tile, EyeParams eye,
                                                         vec3 defaultColor, float4* __restrict__ out, uint32_t n, FeatureMotion<kMotion> motion) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    const float4* sc;
    if constexpr (kSceneInLds) {
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool live = i < n;
        vec3 d = v3(0, 0, 0);
        if (live) {
            const PixelCoord pc = locate(tile, i);
            const float jitteredX = pc.x + 0.5f;
            const float jitteredY = pc.gy + 0.5f;
            const vec3 start = v3(((jitteredX * eye.invW) - 0.5f) * eye.s,
                                  1 * ((jitteredY * eye.invH) - 0.5f) * eye.s * eye.aspect, 1.0f) *
                               eye.camera.zNear;
            d = normalize(rotate(eye.camera.rotation, start));
        }
        const QueryHit q = closestQuery(sc, sceneBlob, L, eye.camera.position, d, ptm::inf(), live);
        if (live) {
            vec3 albedo = defaultColor;
            if (q.kind != 0) albedo = xyz(loadRow16(sc + L.offMaterial + 5 * q.materialIdx));
            float4* f = out + 2 * (size_t)i;
            f[0] = float4{q.normal.x, q.normal.y, q.normal.z, q.dist};
            f[1] = float4{albedo.x, albedo.y, albedo.z, asF((uint32_t)q.materialIdx)};
            if constexpr (kMotion) {
                const ptmo::Motion m = ptmo::pixelMotion(d, eye.camera.position, q.kind, q.prim, q.dist, q.w1, q.w2, motion.prevRecords,
                                                         motion.first, motion.count);
                motion.out[i] = float4{m.prevPoint.x, m.prevPoint.y, m.prevPoint.z, asF((uint32_t)m.surface)};
            }
        }
    }
}

// ---- FEATURES BEHIND MIRRORS AND GLASS (ptss_render_features_specular) ---------------------------------------
// featureKernel's launch shape and eye ray; then the centre ray is carried through the delta lobes of what it meets
// (csrc/ptspecular.h: perfect reflection and refraction, chosen from the material alone) for at most maxSteps steps, one closestQuery
// per link of the chain. The features are those of the LAST surface hit, depth the float32 sum of the chain's hit distances in
// chain order (a path length); a chain that ends in a miss writes featureKernel's miss row. steps (may be null): the links
// followed, 0 .. maxSteps. A lane whose chain has ended goes on as a dead lane of closestQuery; the loop ends for the whole wave,
// by a ballot, once no lane is live. Per lane only the ray, the running depth and the last hit's normal and material index
// live across a query: the material words are read from the staged image when the step needs them.
template <bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void specularFeatureKernel(const float4* __restrict__ sceneBlob, SceneLayout L, TileMap tile, EyeParams eye,
                                                                 vec3 defaultColor, float4* __restrict__ out, uint32_t* __restrict__ steps, uint32_t n,
                                                                 int maxSteps) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    const float4* sc;
    if constexpr (kSceneInLds) {
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool inFrame = i < n;
        vec3 o = eye.camera.position, d = v3(0, 0, 0);
        if (inFrame) {
            const PixelCoord pc = locate(tile, i);
            const float jitteredX = pc.x + 0.5f;
            const float jitteredY = pc.gy + 0.5f;
            const vec3 start = v3(((jitteredX * eye.invW) - 0.5f) * eye.s,
                                  1 * ((jitteredY * eye.invH) - 0.5f) * eye.s * eye.aspect, 1.0f) *
                               eye.camera.zNear;
            d = normalize(rotate(eye.camera.rotation, start));
        }
        bool live = inFrame;
        vec3 normal = v3(0, 0, 0);
        float depth = ptm::inf();
        int materialIdx = -1;
        bool hit = false;   // the chain ended on a surface
        uint32_t taken = 0;
        for (int k = 0; k <= maxSteps; ++k) {
            if (!waveAny(live)) break;
            const QueryHit q = closestQuery(sc, sceneBlob, L, o, d, ptm::inf(), live);
            if (live) {
                live = false;
                hit = q.kind != 0;
                if (!hit) {   // the chain leaves the scene: the miss row
                    normal = v3(0, 0, 0);
                    depth = ptm::inf();
                    materialIdx = -1;
                } else {
                    normal = q.normal;
                    depth = (k == 0) ? q.dist : depth + q.dist;
                    materialIdx = q.materialIdx;
                    if (k < maxSteps) {
                        const float4* mat = sc + L.offMaterial + 5 * q.materialIdx;
                        const float4 misc = loadRow16(mat + 4);   // specularExponent, indexOfRefraction, flags
                        const ptsp::Material m{loadRow16(mat).w, loadRow16(mat + 1).w, loadRow16(mat + 2).w, misc.x, misc.y, (int)asU(misc.z)};
                        const ptsp::Step s = ptsp::step(m, d, q.point, q.normal);
                        if (s.follows) {
                            o = s.o;
                            d = s.d;
                            ++taken;
                            live = true;
                        }
                    }
                }
            }
        }
        if (inFrame) {
            vec3 albedo = defaultColor;
            if (hit) albedo = xyz(loadRow16(sc + L.offMaterial + 5 * materialIdx));
            float4* f = out + 2 * (size_t)i;
            f[0] = float4{normal.x, normal.y, normal.z, depth};
            f[1] = float4{albedo.x, albedo.y, albedo.z, asF((uint32_t)materialIdx)};
            if (steps) steps[i] = taken;
        }
    }
}

// =================================================================================================
static inline unsigned blocksFor(uint32_t n, unsigned block) { return (n + block - 1) / block; }

hipError_t launchRngInit(hipStream_t st, uint32_t* rngHome, uint32_t plane, uint32_t samples, TileMap tile, uint64_t seed,
                         const uint32_t* jumpTable) {
    hipLaunchKernelGGL(rngInitKernel, dim3(blocksFor(plane * samples, 256)), dim3(256), 0, st, rngHome, plane, samples, tile, seed,
                       jumpTable);
    return hipGetLastError();
}

hipError_t launchDisplay(hipStream_t st, const FrameBuffers& fb) {
    hipLaunchKernelGGL(displayKernel, dim3(blocksFor(fb.numPixels, 256)), dim3(256), 0, st, fb);
    return hipGetLastError();
}

hipError_t launchClear(hipStream_t st, const FrameBuffers& fb) {
    hipLaunchKernelGGL(clearKernel, dim3(blocksFor(fb.numPixels, 256)), dim3(256), 0, st, fb);
    return hipGetLastError();
}

hipError_t launchPrimaryPrep(hipStream_t st, float4* sceneBlob, const SceneLayout& layout, ptss_vec3 origin) {
    const int n = layout.numSpheres > layout.numTriangles ? layout.numSpheres : layout.numTriangles;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(primaryPrepKernel, dim3(blocksFor((uint32_t)n, 64)), dim3(64), 0, st, sceneBlob, layout, origin);
    return hipGetLastError();
}

hipError_t launchStripMasks(hipStream_t st, unsigned long long* masks, uint32_t plane, uint32_t numPixels, const float4* sceneBlob,
                            const SceneLayout& layout, TileMap tile, EyeParams eye) {
    const uint32_t numStrips = plane / ptloc::kStrip;
    if (numStrips == 0) return hipSuccess;
    hipLaunchKernelGGL(stripMaskKernel, dim3(blocksFor(numStrips, 64)), dim3(64), 0, st, masks, numStrips, numPixels, sceneBlob, layout, tile, eye);
    return hipGetLastError();
}

#if PTSS_DIAG
hipError_t readDiagCounters(unsigned long long* out8) { return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_diag), 64); }
#endif
static_assert(sizeof(float4) == kVec4Bytes, "bounceLdsBytes counts rows of float4");

// ---- which instantiation runs: five scene variants, each one {kAccel, kBounded, kPairs, kMesh} of bounceKernel, the first four
// also of frameKernel (the mesh image has none: ptss_create never qualifies it for one launch per frame).
// sceneVariant is the one place that decides; every launch and occupancy query below looks its kernel up through it.
enum SceneVariant : int { kVariantAccel, kVariantBoundedPairs, kVariantBounded, kVariantPlain, kVariantMesh, kNumVariants };
constexpr int kNumFrameVariants = kVariantMesh;
constexpr bool kVariantArgs[kNumVariants][4] = {{true, false, false, false}, {false, true, true, false}, {false, true, false, false},
                                                {false, false, false, false}, {false, false, false, true}};

// bounded: the frame may take the shorter sphere test (SceneLayout::sphereBounded and a camera in range, ptss_api.hip)
static SceneVariant sceneVariant(const SceneLayout& layout, bool bounded) {
    if (meshImage(layout)) return kVariantMesh;   // (the reference's sphere test: one image for every camera)
    if (layout.accelSpheres) return kVariantAccel;
    if (bounded && layout.neePairs) return kVariantBoundedPairs;
    return bounded ? kVariantBounded : kVariantPlain;
}

using KernelFn = void (*)(FrameBuffers, const float4*, SceneLayout, int, TileMap, EyeParams);   // bounceKernel and frameKernel alike

template <size_t... I>   // entry I = variant * 8 + kLast * 4 + kSceneInLds * 2 + kFirst
constexpr std::array<KernelFn, sizeof...(I)> bounceTable(std::index_sequence<I...>) {
    return {{bounceKernel<(I & 4) != 0, (I & 2) != 0, (I & 1) != 0, kVariantArgs[I / 8][0], kVariantArgs[I / 8][1], kVariantArgs[I / 8][2],
                          kVariantArgs[I / 8][3]>...}};
}
template <size_t... V>
constexpr std::array<KernelFn, sizeof...(V)> frameTable(std::index_sequence<V...>) {
    return {{frameKernel<kVariantArgs[V][0], kVariantArgs[V][1], kVariantArgs[V][2]>...}};
}
static int bounceIndex(SceneVariant v, bool last, bool sceneInLds, bool first) { return v * 8 + last * 4 + sceneInLds * 2 + first; }
static KernelFn bounceKernelFor(int index) {
    static constexpr auto table = bounceTable(std::make_index_sequence<kNumVariants * 8>{});
    return table[index];
}
static KernelFn frameKernelFor(SceneVariant v) {
    static constexpr auto table = frameTable(std::make_index_sequence<kNumFrameVariants>{});
    return v < kNumFrameVariants ? table[v] : nullptr;
}
static int blocksPerCU(KernelFn k, size_t lds) {
    int a = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k, kBlock, lds) == hipSuccess ? a : 0;
}

// *launched collects the bit of every instantiation enqueued (ptss_launched_kernels; the PTSS_KERNEL_* ranges of ptss_types.h): a
// bounce kernel's `bounceTable index` in PTSS_KERNEL_BOUNCE, the mesh variant's eight in a range of their own, PTSS_KERNEL_BOUNCE_MESH;
// a frame kernel's variant in PTSS_KERNEL_FRAME. The ranges must stay disjoint and inside the 64-bit word.
constexpr int kKernelBitRanges[][2] = {
    {PTSS_KERNEL_BOUNCE, PTSS_KERNEL_WIDTH_BOUNCE},       {PTSS_KERNEL_FRAME, PTSS_KERNEL_WIDTH_FRAME},
    {PTSS_KERNEL_BOUNCE_MESH, PTSS_KERNEL_WIDTH_BOUNCE_MESH}, {PTSS_KERNEL_QUERY, PTSS_KERNEL_WIDTH_QUERY},
    {PTSS_KERNEL_FEATURES, PTSS_KERNEL_WIDTH_FEATURES},   {PTSS_KERNEL_DENOISE, PTSS_KERNEL_WIDTH_DENOISE},
    {PTSS_KERNEL_UPDATE, PTSS_KERNEL_WIDTH_UPDATE},       {PTSS_KERNEL_REFIT, PTSS_KERNEL_WIDTH_REFIT},
    {PTSS_KERNEL_REPROJECT, PTSS_KERNEL_WIDTH_REPROJECT}, {PTSS_KERNEL_FEATURES_MOTION, PTSS_KERNEL_WIDTH_FEATURES_MOTION},
    {PTSS_KERNEL_REPROJECT_MOTION, PTSS_KERNEL_WIDTH_REPROJECT_MOTION}};
constexpr bool kernelBitRangesDisjoint() {
    unsigned long long taken = 0;
    for (const auto& r : kKernelBitRanges) {
        if (r[0] < 0 || r[1] < 1 || r[0] + r[1] > 64) return false;
        const unsigned long long bits = (r[1] == 64 ? ~0ull : (1ull << r[1]) - 1ull) << r[0];
        if (taken & bits) return false;
        taken |= bits;
    }
    return true;
}
static_assert(kernelBitRangesDisjoint(), "two kernels share a bit of ptss_launched_kernels, or a range leaves the 64-bit word");
static_assert(kNumFrameVariants * 8 == PTSS_KERNEL_WIDTH_BOUNCE && kNumFrameVariants == PTSS_KERNEL_WIDTH_FRAME &&
                  (kNumVariants - kNumFrameVariants) * 8 == PTSS_KERNEL_WIDTH_BOUNCE_MESH,
              "the bounce and frame tables fill their bit ranges");

hipError_t launchBounce(hipStream_t st, const FrameBuffers& fb, const float4* sceneBlob, SceneLayout layout, int bounce,
                        bool isLast, bool sceneInLds, bool bounded, int gridBlocks, TileMap tile, EyeParams eye, unsigned long long* launched) {
    const int index = bounceIndex(sceneVariant(layout, bounded), isLast, sceneInLds, bounce == 0);
    hipLaunchKernelGGL(bounceKernelFor(index), dim3(gridBlocks), dim3(kBlock), bounceLdsBytes(layout, sceneInLds), st, fb, sceneBlob, layout, bounce,
                       tile, eye);
    const hipError_t e = hipGetLastError();
    const bool mesh = index >= kVariantMesh * 8;   // the mesh variant's eight follow the others' in bounceTable
    if (e == hipSuccess) markLaunched(launched, mesh ? PTSS_KERNEL_BOUNCE_MESH : PTSS_KERNEL_BOUNCE, mesh ? index - kVariantMesh * 8 : index);
    return e;
}

hipError_t launchFrame(hipStream_t st, const FrameBuffers& fb, const float4* sceneBlob, SceneLayout layout, int numBounces, bool bounded, int gridBlocks,
                       TileMap tile, EyeParams eye, unsigned long long* launched) {
    const SceneVariant v = sceneVariant(layout, bounded);
    if (!frameKernelFor(v)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(frameKernelFor(v), dim3(gridBlocks), dim3(kBlock), bounceLdsBytes(layout, true), st, fb, sceneBlob, layout, numBounces, tile, eye);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, PTSS_KERNEL_FRAME, v);
    return e;
}
// resident workgroups per CU of the frame kernel `layout` would run (the API's answer; the caller keeps one in reserve)
int frameOccupancyBlocksPerCU(const SceneLayout& layout, bool bounded) {
    const KernelFn k = frameKernelFor(sceneVariant(layout, bounded));
    return k ? blocksPerCU(k, bounceLdsBytes(layout, true)) : 0;
}

// the query kernel (PTSS_KERNEL_QUERY + any * 2 + inLds of *launched): one workgroup per kBlock rays, at most maxBlocks (resident rounds)
hipError_t launchQuery(hipStream_t st, bool any, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* out,
                       uint32_t n, int maxBlocks, unsigned long long* launched) {
    using QueryFn = void (*)(const float4*, SceneLayout, const float4*, float4*, uint32_t);
    static constexpr QueryFn table[4] = {queryKernel<false, false>, queryKernel<false, true>, queryKernel<true, false>, queryKernel<true, true>};
    const int index = (any ? 2 : 0) + (sceneInLds ? 1 : 0);
    unsigned blocks = blocksFor(n, kBlock);
    if (maxBlocks > 0 && blocks > (unsigned)maxBlocks) blocks = (unsigned)maxBlocks;
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    hipLaunchKernelGGL(table[index], dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, static_cast<const float4*>(rays),
                       static_cast<float4*>(out), n);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, PTSS_KERNEL_QUERY, index);
    return e;
}

// the feature kernel, without or with the motion rows (PTSS_KERNEL_FEATURES / PTSS_KERNEL_FEATURES_MOTION + inLds of *launched): one
// workgroup per kBlock local pixels, at most maxBlocks
template <bool kMotion>
static hipError_t launchFeatureKernel(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                                      ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, FeatureMotion<kMotion> motion,
                                      unsigned long long* launched) {
    unsigned blocks = blocksFor(n, kBlock);
    if (maxBlocks > 0 && blocks > (unsigned)maxBlocks) blocks = (unsigned)maxBlocks;
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? featureKernel<true, kMotion> : featureKernel<false, kMotion>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, tile, eye, defaultColor, static_cast<float4*>(out), n, motion);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, kMotion ? PTSS_KERNEL_FEATURES_MOTION : PTSS_KERNEL_FEATURES, sceneInLds ? 1 : 0);
    return e;
}

hipError_t launchFeatures(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                          ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, unsigned long long* launched) {
    return launchFeatureKernel<false>(st, sceneBlob, layout, sceneInLds, tile, eye, defaultColor, out, n, maxBlocks, {}, launched);
}

hipError_t launchFeaturesMotion(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                                ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, const void* prevRecords, uint32_t first,
                                uint32_t count, void* motionOut, unsigned long long* launched) {
    return launchFeatureKernel<true>(st, sceneBlob, layout, sceneInLds, tile, eye, defaultColor, out, n, maxBlocks,
                                     {static_cast<const float*>(prevRecords), first, count, static_cast<float4*>(motionOut)}, launched);
}

// the specular-chain feature kernel: featureKernel's grid. It owns no bit of *launched; launches[inLds] counts instead
// (ptss_specular_feature_launches)
hipError_t launchFeaturesSpecular(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, TileMap tile, EyeParams eye,
                                  ptss_vec3 defaultColor, void* out, void* steps, uint32_t n, int maxSteps, int maxBlocks,
                                  unsigned long long* launches) {
    unsigned blocks = blocksFor(n, kBlock);
    if (maxBlocks > 0 && blocks > (unsigned)maxBlocks) blocks = (unsigned)maxBlocks;
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? specularFeatureKernel<true> : specularFeatureKernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, tile, eye, defaultColor, static_cast<float4*>(out),
                       static_cast<uint32_t*>(steps), n, maxSteps);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++launches[sceneInLds ? 1 : 0];
    return e;
}

hipError_t launchFlush(hipStream_t st, const FrameBuffers& fb, int numBounces, const FlushTargets& targets) {
    hipLaunchKernelGGL(flushKernel, dim3(1), dim3(kMinLiveRays), 0, st, fb, numBounces, targets);
    return hipGetLastError();
}

// Resident workgroups per CU of the mid-bounce instantiation that `layout` runs (registers and this scene's LDS image)
int bounceOccupancyBlocksPerCU(const SceneLayout& layout, bool sceneInLds, bool bounded) {
    return blocksPerCU(bounceKernelFor(bounceIndex(sceneVariant(layout, bounded), false, sceneInLds, false)), bounceLdsBytes(layout, sceneInLds));
}

}  // namespace ptss
