// ptss_paths.hip — the kernels behind ptss_seed_path_rng and ptss_trace_paths (include/ptss.h): the path tracer
// started from the caller's rays. Device code over the layer headers (ptwave.h .. ptshade.h), which are private to each translation
// unit that includes them: this file gets its own copy of closestQuery, anyQuery, lightSample, addLambertTerm and scatter(), the
// functions the frame's bounce kernel and the query kernels are built from, so a path here performs the operations of
// pathTraceKernel's thread body (CudaTracer.cu:106-206) exactly as a path of a frame does. (Diagnostic builds, PTSS_DIAG != 0: the
// hooks inside those functions count into this file's own g_diag, which nothing reads.)
//
// pathQueryKernel has specularFeatureKernel's shape: kBlock lanes per workgroup, grid-strided, one lane per ray, the scene image
// staged as the other query kernels stage it. A lane keeps its ray, throughput, radiance and XORWOW state in registers across the
// iterations; the iteration loop is wave-uniform (it ends, by a ballot, once no lane of the wave is live) and a finished lane rides
// along as a dead lane of closestQuery / anyQuery. Per iteration: one closestQuery; then, light by light in the reference's order
// (point lights, area lights), every lit lane makes the head of lineOfSight (CudaTracer.cu:423-432) as bounceTile's step 2 does —
// the light sample (four draws per area light, visible or not), the bump along the normal, distance - 2 * bump — and the wave traces
// those segments densely, one per lane, with the any-hit of the image's kind (skipped when no lane of the wave has a segment whose
// answer matters: bounceTile's neeSkipSafe shortcut, which skips a test and never a draw); then addLambertTerm, scatter(),
// Beer-Lambert and the two radiance updates in the reference's order. No LDS queue, no lane splitting, no compaction: plain and exact.
//
// Every path runs on its own: the frame loop's guard `numRays > 128` (CudaTracer.cu:622) is a property of a frame, not of a path,
// and does not exist here (the documented behaviour of a tileWorld > 1 context).
//
// pathRefillKernel (ptss_trace_paths_opt with PTSS_PATHS_REFILL) is the same iteration under another schedule: a lane
// whose path has ended takes the next unclaimed ray of the batch. Its comment stands in front of it, below pathQueryKernel.
#include "ptss_device.h"
#include "pthit.h"
#include "ptshade.h"

namespace ptss {

// ptss_seed_path_rng: rngInitKernel's seeding (curand_init(seed, sequence, 0): the scramble, then the 2^67 jump table), then `skip`
// draws discarded one by one. firstSequence + n <= 2^32 (checked by the caller), so the sequence of every entry fits 32 bits.
__global__ void pathRngSeedKernel(uint32_t* __restrict__ rng, uint32_t n, uint64_t seed, uint32_t firstSequence, uint32_t skip,
                                  const uint32_t* __restrict__ jumpTable) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ptrng::State s = ptrng::seeded(seed);
    ptrng::skip_subsequences(s, firstSequence + i, jumpTable);
    for (uint32_t k = 0; k < skip; ++k) (void)ptrng::next(s);
    uint32_t* out = rng + 6 * (size_t)i;   // ptss_path_rng: v[0..4], d
#pragma unroll
    for (int w = 0; w < 5; ++w) out[w] = s.v[w];
    out[5] = s.d;
}

// Registers: with the workgroup size as the only bound the compiler takes 84 (scene in LDS) / 88 (in place) VGPRs and no scratch, which
// admits five waves per SIMD; asking for six (80 registers) puts 20 B per lane of the in-place instantiation into scratch, so no
// second bound is declared. The ~60 scalar registers it spills are SceneLayout's fields, parked in VGPR lanes
// (v_writelane / v_readlane), not in memory.
template <bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void pathQueryKernel(const float4* __restrict__ sceneBlob, SceneLayout L, const float4* __restrict__ rays,
                                                              uint32_t* __restrict__ rng, float4* __restrict__ out, uint32_t n, int maxIterations,
                                                              vec3 defaultColor, uint32_t guardFlags) {
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
    const float4* td = mesh ? sceneBlob : sc;   // the triangle tables (global memory in the mesh image)
    const int numLights = L.numPointLights + L.numAreaLights;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool inBatch = i < n;
        RayRegs ray;
        ray.o = ray.d = ray.L0 = v3(0, 0, 0);
        ray.T = v3(1, 1, 1);
        ray.pix = 0;
        ray.rng = ptrng::State{{0, 0, 0, 0, 0}, 0};
        ray.active = inBatch;
        if (inBatch) {
            ray.o = xyz(rays[2 * (size_t)i]);   // (.w, the row's tmax, is not used: a path starts at distance +inf)
            ray.d = xyz(rays[2 * (size_t)i + 1]);
            const uint32_t* s = rng + 6 * (size_t)i;
#pragma unroll
            for (int w = 0; w < 5; ++w) ray.rng.v[w] = s[w];
            ray.rng.d = s[5];
        }
        uint32_t entered = 0;
        for (int it = 0; it < maxIterations; ++it) {
            const bool live = ray.active;
            if (!waveAny(live)) break;
            const bool last = it == maxIterations - 1;

            // ---- closest hit + surfel (pathTraceKernel :121-163) ----
            const QueryHit q = closestQuery(sc, sceneBlob, L, ray.o, ray.d, ptm::inf(), live);
            const bool hit = live && q.kind != 0;
            const vec3 point = q.point, normal = q.normal;
            const float cosI = hit ? dot(-ray.d, normal) : 0.0f;
            const bool inside = cosI <= 0.0f;
            const bool lit = hit && !inside;   // shade() runs, :166-169
            const float4* mat = sc + L.offMaterial + 5 * (hit ? q.materialIdx : 0);

            // ---- shade(), CudaTracer.cu:345-390: one light at a time, one shadow segment per lit lane ----
            vec3 radiance = v3(0, 0, 0);
            for (int li = 0; li < numLights; ++li) {
                bool need = false;
                float cosL = 0, distance2 = 0, distance = 0;
                vec3 lo = v3(0, 0, 0), w_i = v3(0, 0, 0);
                if (lit) {
                    vec3 lightPoint;
                    if (li < L.numPointLights) {
                        lightPoint = xyz(loadRow16(sc + L.offPointLight + 2 * li));
                    } else {  // getAreaLightPoint :392-418 — four draws whether or not the light ends up visible
                        const float4 light = sc[L.offAreaLight + 2 * (li - L.numPointLights)];
                        const float u1 = ptrng::uniform(ray.rng);
                        const float u2 = ptrng::uniform(ray.rng);
                        const float u3 = ptrng::uniform(ray.rng);
                        const float inverseTotal = ptm::rcp_in_range(u1 + u2 + u3);   // the sum lies in [2^-32, 3] (bounceTile)
                        const float weight0 = u1 * inverseTotal, weight1 = u2 * inverseTotal, weight2 = u3 * inverseTotal;
                        // triangleIdx or triangleIdx + 1, :408 — as stored positions
                        const int tri = (ptrng::uniform(ray.rng) > .5f) ? (int)asU(light.w) : (int)asU(sc[L.offAreaLight + 2 * (li - L.numPointLights) + 1].x);
                        const vec3 a = xyz(loadRow16(td + L.offTri + 3 * tri));
                        const vec3 b = xyz(loadRow16(td + L.offTriVert + 2 * tri));
                        const vec3 c = xyz(loadRow16(td + L.offTriVert + 2 * tri + 1));
                        lightPoint = (a * weight0 + b * weight1) + c * weight2;
                    }
                    // head of lineOfSight :423-432
                    const vec3 offset = lightPoint - point;
                    lightSample(offset, distance2, distance, w_i);
                    cosL = ptm::max(0.0f, dot(normal, w_i));
                    // the term is +-0 whatever the visibility (bounceTile, "Exactness of the shadow-ray skip")
                    const bool zeroTerm = L.neeSkipSafe && (distance2 > 0.0f) && (distance2 < ptm::inf()) && (cosL == 0.0f || mat[0].w == 0.0f);
                    need = !zeroTerm;
                    lo = point + (ptm::kRayBump * normal);
                    distance -= 2 * ptm::kRayBump;
                }
                bool blocked = false;
                if (waveAny(need)) blocked = anyQuery(sc, sceneBlob, L, mesh, lo, w_i, distance, need);
                if (need && !blocked) {
                    const vec3 power = (li < L.numPointLights) ? xyz(loadRow16(sc + L.offPointLight + 2 * li + 1))
                                                               : xyz(loadRow16(sc + L.offAreaLight + 2 * (li - L.numPointLights)));
                    addLambertTerm(radiance, cosL, power, distance2, mat[0], (guardFlags & kGuardLightPowers) != 0u);
                }
            }

            // ---- scatter + radiance update (pathTraceKernel :172-198) ----
            if (live) {
                ++entered;
                if (hit) {
                    vec3 directRadiance = v3(0, 0, 0) + xyz(mat[3]);   // emmitance, :163
                    if (lit) directRadiance = directRadiance + radiance;
                    vec3 indirectRadiance = v3(1, 1, 1);
                    if (!last) indirectRadiance = scatter(mat, ray, point, normal, cosI, guardFlags);
                    if (inside) {  // Beer-Lambert, :179-185
                        const float4 ab = mat[2];
                        ray.T = ray.T * v3(ptm::exp(-q.dist * ab.x), ptm::exp(-q.dist * ab.y), ptm::exp(-q.dist * ab.z));
                    }
                    ray.L0 = ray.L0 + ray.T * directRadiance;
                    ray.T = ray.T * indirectRadiance;
                } else {  // :193-198
                    ray.L0 = ray.L0 + defaultColor * ray.T;
                    ray.active = false;
                }
            }
        }
        if (inBatch) {
            out[i] = float4{ray.L0.x, ray.L0.y, ray.L0.z, asF(entered)};
            uint32_t* s = rng + 6 * (size_t)i;
#pragma unroll
            for (int w = 0; w < 5; ++w) s[w] = ray.rng.v[w];
            s[5] = ray.rng.d;
        }
    }
}

// ---- the refill schedule (ptss_trace_paths_opt with PTSS_PATHS_REFILL) ----
// pathQueryKernel's iteration, one loop instead of two: a lane whose path has ended takes the next unclaimed ray of the batch before the
// wave's next iteration, so the wave's iterations are spent on live lanes as long as the batch has rays. Every path has its own ray row,
// stream and result row, and nothing in an iteration lets a lane's values depend on its neighbours' (neeSkipSafe and the wave-uniform
// exits skip tests, never draws), so ray i gets the bytes pathQueryKernel gives it whichever lane runs it and beside whichever rays.
//
// Claiming. Lane t of workgroup b starts with ray b * kBlock + t (the launcher keeps gridDim.x <= ceil(n / kBlock)); *head, set to
// gridDim.x * kBlock in front of the kernel, is the first ray nobody owns. A wave takes kRefillChunk rays at a time with one returning
// atomic add and keeps them as a reserve [next, end) in scalar registers; before every iteration its dead lanes, ranked in lane order,
// take next, next + 1, .. — from the reserve, then, if that ran out, from one new chunk: at most two steps. A wave that has seen the head
// at or past n claims no more; it leaves the loop when none of its lanes is live. No wave waits for another.
//
// counters[0..2] (cumulative, device): the iterations the waves ran, the live lanes summed over them, the dequeues.
#ifndef PTSS_REFILL_CHUNK
#define PTSS_REFILL_CHUNK 64   // rays per dequeue: the fastest of 64, 256 and 1024 on "mixed" (tools/build_variants.py rc256=PTSS_REFILL_CHUNK=256)
#endif
constexpr uint32_t kRefillChunk = PTSS_REFILL_CHUNK;
static_assert(kRefillChunk >= 64 && kRefillChunk <= 65536, "a chunk fills a whole wave: the refill takes at most two steps");

// Registers: 85 (scene in LDS) / 87 (in place) VGPRs, no scratch: five waves per SIMD as pathQueryKernel.
template <bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void pathRefillKernel(const float4* __restrict__ sceneBlob, SceneLayout L, const float4* __restrict__ rays,
                                                               uint32_t* __restrict__ rng, float4* __restrict__ out, uint32_t n, int maxIterations,
                                                               vec3 defaultColor, uint32_t guardFlags, uint32_t* __restrict__ head,
                                                               unsigned long long* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    const float4* sc;
    if constexpr (kSceneInLds) {   // every workgroup has rays of the static fill: whether it stages does not depend on the head
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    const bool mesh = meshImage(L);
    const float4* td = mesh ? sceneBlob : sc;
    const int numLights = L.numPointLights + L.numAreaLights;
    const uint32_t lane = laneId();

    uint32_t i = blockIdx.x * kBlock + threadIdx.x;   // the ray this lane runs
    RayRegs ray;
    ray.o = ray.d = ray.L0 = v3(0, 0, 0);
    ray.T = v3(1, 1, 1);
    ray.pix = 0;
    ray.rng = ptrng::State{{0, 0, 0, 0, 0}, 0};
    ray.active = i < n;
    if (ray.active) {
        ray.o = xyz(rays[2 * (size_t)i]);
        ray.d = xyz(rays[2 * (size_t)i + 1]);
        const uint32_t* s = rng + 6 * (size_t)i;
#pragma unroll
        for (int w = 0; w < 5; ++w) ray.rng.v[w] = s[w];
        ray.rng.d = s[5];
    }
    uint32_t entered = 0;
    uint32_t next = 0, end = 0;                            // the wave's reserve (wave-uniform)
    bool drained = gridDim.x * (uint32_t)kBlock >= n;      // the head is at or past n (wave-uniform)
    uint32_t waveIterations = 0, laneIterations = 0, dequeues = 0;

    for (;;) {
        // ---- refill the dead lanes ----
        unsigned long long dead = __builtin_amdgcn_ballot_w64(!ray.active);
        for (int step = 0; step < 2 && dead != 0ull; ++step) {
            if (next == end) {
                if (drained) break;
                uint32_t h = 0;
                if (lane == 0) h = atomicAdd(head, kRefillChunk);
                h = __builtin_amdgcn_readfirstlane(h);
                ++dequeues;
                drained = h >= n || n - h <= kRefillChunk;
                if (h >= n) break;
                next = h;
                end = drained ? n : h + kRefillChunk;
            }
            const uint32_t rank = rankBelow(dead);
            const uint32_t mine = next + rank;
            if (!ray.active && mine < end) {
                i = mine;
                ray.o = xyz(rays[2 * (size_t)i]);
                ray.d = xyz(rays[2 * (size_t)i + 1]);
                const uint32_t* s = rng + 6 * (size_t)i;
#pragma unroll
                for (int w = 0; w < 5; ++w) ray.rng.v[w] = s[w];
                ray.rng.d = s[5];
                ray.L0 = v3(0, 0, 0);
                ray.T = v3(1, 1, 1);
                entered = 0;
                ray.active = true;
            }
            const uint32_t wanted = (uint32_t)__builtin_popcountll(dead), left = end - next;
            next += wanted < left ? wanted : left;
            dead = __builtin_amdgcn_ballot_w64(!ray.active);
        }
        const bool live = ray.active;
        const unsigned long long liveMask = __builtin_amdgcn_ballot_w64(live);
        if (liveMask == 0ull) break;
        ++waveIterations;
        laneIterations += (uint32_t)__builtin_popcountll(liveMask);
        const bool last = entered == (uint32_t)maxIterations - 1u;   // per lane: it gates the lane's own scatter() only

        // ---- closest hit + surfel (pathTraceKernel :121-163) ----
        const QueryHit q = closestQuery(sc, sceneBlob, L, ray.o, ray.d, ptm::inf(), live);
        const bool hit = live && q.kind != 0;
        const vec3 point = q.point, normal = q.normal;
        const float cosI = hit ? dot(-ray.d, normal) : 0.0f;
        const bool inside = cosI <= 0.0f;
        const bool lit = hit && !inside;   // shade() runs, :166-169
        const float4* mat = sc + L.offMaterial + 5 * (hit ? q.materialIdx : 0);

        // ---- shade(), CudaTracer.cu:345-390: one light at a time, one shadow segment per lit lane ----
        vec3 radiance = v3(0, 0, 0);
        for (int li = 0; li < numLights; ++li) {
            bool need = false;
            float cosL = 0, distance2 = 0, distance = 0;
            vec3 lo = v3(0, 0, 0), w_i = v3(0, 0, 0);
            if (lit) {
                vec3 lightPoint;
                if (li < L.numPointLights) {
                    lightPoint = xyz(loadRow16(sc + L.offPointLight + 2 * li));
                } else {  // getAreaLightPoint :392-418 — four draws whether or not the light ends up visible
                    const float4 light = sc[L.offAreaLight + 2 * (li - L.numPointLights)];
                    const float u1 = ptrng::uniform(ray.rng);
                    const float u2 = ptrng::uniform(ray.rng);
                    const float u3 = ptrng::uniform(ray.rng);
                    const float inverseTotal = ptm::rcp_in_range(u1 + u2 + u3);   // the sum lies in [2^-32, 3] (bounceTile)
                    const float weight0 = u1 * inverseTotal, weight1 = u2 * inverseTotal, weight2 = u3 * inverseTotal;
                    const int tri = (ptrng::uniform(ray.rng) > .5f) ? (int)asU(light.w) : (int)asU(sc[L.offAreaLight + 2 * (li - L.numPointLights) + 1].x);
                    const vec3 a = xyz(loadRow16(td + L.offTri + 3 * tri));
                    const vec3 b = xyz(loadRow16(td + L.offTriVert + 2 * tri));
                    const vec3 c = xyz(loadRow16(td + L.offTriVert + 2 * tri + 1));
                    lightPoint = (a * weight0 + b * weight1) + c * weight2;
                }
                // head of lineOfSight :423-432
                const vec3 offset = lightPoint - point;
                lightSample(offset, distance2, distance, w_i);
                cosL = ptm::max(0.0f, dot(normal, w_i));
                const bool zeroTerm = L.neeSkipSafe && (distance2 > 0.0f) && (distance2 < ptm::inf()) && (cosL == 0.0f || mat[0].w == 0.0f);
                need = !zeroTerm;
                lo = point + (ptm::kRayBump * normal);
                distance -= 2 * ptm::kRayBump;
            }
            bool blocked = false;
            if (waveAny(need)) blocked = anyQuery(sc, sceneBlob, L, mesh, lo, w_i, distance, need);
            if (need && !blocked) {
                const vec3 power = (li < L.numPointLights) ? xyz(loadRow16(sc + L.offPointLight + 2 * li + 1))
                                                           : xyz(loadRow16(sc + L.offAreaLight + 2 * (li - L.numPointLights)));
                addLambertTerm(radiance, cosL, power, distance2, mat[0], (guardFlags & kGuardLightPowers) != 0u);
            }
        }

        // ---- scatter + radiance update (pathTraceKernel :172-198), then retire ----
        if (live) {
            ++entered;
            if (hit) {
                vec3 directRadiance = v3(0, 0, 0) + xyz(mat[3]);   // emmitance, :163
                if (lit) directRadiance = directRadiance + radiance;
                vec3 indirectRadiance = v3(1, 1, 1);
                if (!last) indirectRadiance = scatter(mat, ray, point, normal, cosI, guardFlags);
                if (inside) {  // Beer-Lambert, :179-185
                    const float4 ab = mat[2];
                    ray.T = ray.T * v3(ptm::exp(-q.dist * ab.x), ptm::exp(-q.dist * ab.y), ptm::exp(-q.dist * ab.z));
                }
                ray.L0 = ray.L0 + ray.T * directRadiance;
                ray.T = ray.T * indirectRadiance;
            } else {  // :193-198
                ray.L0 = ray.L0 + defaultColor * ray.T;
                ray.active = false;
            }
            if (!ray.active || entered >= (uint32_t)maxIterations) {   // the rows pathQueryKernel writes for ray i
                out[i] = float4{ray.L0.x, ray.L0.y, ray.L0.z, asF(entered)};
                uint32_t* s = rng + 6 * (size_t)i;
#pragma unroll
                for (int w = 0; w < 5; ++w) s[w] = ray.rng.v[w];
                s[5] = ray.rng.d;
                ray.active = false;
            }
        }
    }
    if (lane == 0) {
        atomicAdd(&counters[0], (unsigned long long)waveIterations);
        atomicAdd(&counters[1], (unsigned long long)laneIterations);
        atomicAdd(&counters[2], (unsigned long long)dequeues);
    }
}

static inline unsigned pathBlocksFor(uint32_t n, unsigned block) { return (n + block - 1) / block; }

hipError_t launchPathRngSeed(hipStream_t st, void* rng, uint32_t n, uint64_t seed, uint32_t firstSequence, uint32_t skip, const uint32_t* jumpTable) {
    hipLaunchKernelGGL(pathRngSeedKernel, dim3(pathBlocksFor(n, 256)), dim3(256), 0, st, static_cast<uint32_t*>(rng), n, seed, firstSequence, skip,
                       jumpTable);
    return hipGetLastError();
}

// the path kernel: queryKernel's grid. It owns no bit of ptss_launched_kernels; launches[inLds] counts instead (ptss_path_launches)
hipError_t launchPathQuery(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* rng, void* out,
                           uint32_t n, int maxIterations, ptss_vec3 defaultColor, uint32_t guardFlags, int maxBlocks, unsigned long long* launches) {
    unsigned blocks = pathBlocksFor(n, kBlock);
    if (maxBlocks > 0 && blocks > (unsigned)maxBlocks) blocks = (unsigned)maxBlocks;
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? pathQueryKernel<true> : pathQueryKernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, static_cast<const float4*>(rays), static_cast<uint32_t*>(rng),
                       static_cast<float4*>(out), n, maxIterations, defaultColor, guardFlags);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++launches[sceneInLds ? 1 : 0];
    return e;
}

// the refill kernel: min(ceil(n / kBlock), cap) workgroups, cap = maxWorkgroups or, when that is 0, the workgroups of this instantiation
// the device holds at once (nothing in the kernel waits, so an over-estimate costs nothing). state: the context's four 64-bit device words,
// [0] the queue head (its low 32 bits; set to grid * kBlock by a memset node in front of the kernel), [1..3] the counters. The grid is
// also kept small enough that the head cannot wrap: every wave adds at most one chunk past n.
hipError_t launchPathRefill(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* rng, void* out,
                            uint32_t n, int maxIterations, ptss_vec3 defaultColor, uint32_t guardFlags, int maxWorkgroups, int numCUs,
                            unsigned long long* state, unsigned long long* launches) {
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? pathRefillKernel<true> : pathRefillKernel<false>;
    unsigned cap = (unsigned)maxWorkgroups;
    if (cap == 0) {
        int perCU = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, kBlock, lds) != hipSuccess || perCU < 1) perCU = 1;
        cap = (unsigned)perCU * (unsigned)(numCUs > 0 ? numCUs : 1);
    }
    const unsigned wrapCap = (unsigned)((0xFFFFFFFFull - n) / ((unsigned long long)kWaves * kRefillChunk));
    unsigned blocks = pathBlocksFor(n, kBlock);
    if (blocks > cap) blocks = cap;
    if (blocks > wrapCap) blocks = wrapCap;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(state), (int)(blocks * (unsigned)kBlock), 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, static_cast<const float4*>(rays), static_cast<uint32_t*>(rng),
                       static_cast<float4*>(out), n, maxIterations, defaultColor, guardFlags, reinterpret_cast<uint32_t*>(state), state + 1);
    e = hipGetLastError();
    if (e == hipSuccess) ++launches[sceneInLds ? 1 : 0];
    return e;
}

}  // namespace ptss
