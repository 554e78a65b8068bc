// ptss_chain.hip — the kernels behind ptss_intersect_chain (include/ptss.h): ptss_intersect carried through the delta
// lobes of what the caller's rays meet. Device code over the layer headers (ptwave.h .. pthit.h), which are private to each translation
// unit that includes them: this file gets its own copy of closestQuery, the function queryKernel and specularFeatureKernel are built
// from, so a link here is the query ptss_intersect makes for the same ray, and the step and its factor are csrc/ptspecular.h's
// (ptsp::step, ptsp::linkFactor), which the host probe ptss_probe_specular_link compiles as well.
//
// A chain: closestQuery with the caller's tmax on the first link and +inf on later ones; at a hit, while fewer than maxSteps links have
// been followed, ptsp::step from the material's words; a link that follows multiplies the throughput by its factor and continues the
// ray. The chain ends at a terminal material, a miss, a direction that is not finite or maxSteps, and the lane then writes the rows of
// its ray at once: the ptss_ray_hit of the last query (three 16-byte rows, the miss row included) and, when the caller wants them, the
// two rows of ptss_chain_result. Per lane only the ray, its tmax, the throughput, the running length and the step count live across
// a query.
//
// Two schedules with the same bytes (every chain runs on its own values; closestQuery's wave-uniform choices pick between forms that
// end on the same hit, pthit.h):
//   chainKernel        specularFeatureKernel's shape: kBlock lanes per workgroup, grid-strided, one lane per ray. A lane whose chain has
//                      ended rides along as a dead lane of closestQuery until a ballot finds the wave empty.
//   chainRefillKernel  pathRefillKernel's schedule (ptss_paths.hip): a static first fill, then chunks of kChainChunk
//                      rays claimed with one atomic add per wave and handed to the dead lanes in lane order before every link. The
//                      head is a device word of its own, so chain calls and path queries do not disturb each other. No wave waits
//                      for another.
#include "ptss_device.h"
#include "pthit.h"
#include "ptspecular.h"

namespace ptss {

constexpr uint32_t kChainChunk = 64;   // rays per dequeue: one wave's worth, so a refill takes at most two steps

struct ChainLane {
    vec3 o, d, T;
    float tmax, length;
    uint32_t taken;
    bool active;
};

__device__ __forceinline__ void chainStart(ChainLane& c, const float4* __restrict__ rays, uint32_t i) {
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
    c.o = xyz(r0);
    c.d = xyz(r1);
    c.tmax = r0.w;
    c.T = v3(1, 1, 1);
    c.length = ptm::inf();
    c.taken = 0;
    c.active = true;
}

// One link for every lane of the wave (all of them call it; a lane that is not active is a dead lane of the query). i: the lane's ray.
__device__ __forceinline__ void chainLink(const float4* sc, const float4* __restrict__ sceneBlob, const SceneLayout& L, ChainLane& c, uint32_t i,
                                          int maxSteps, float4* __restrict__ hits, float4* __restrict__ chain) {
    const bool live = c.active;
    const QueryHit q = closestQuery(sc, sceneBlob, L, c.o, c.d, c.tmax, live);
    if (!live) return;
    const bool hit = q.kind != 0;
    c.length = hit ? (c.taken == 0u ? q.dist : c.length + q.dist) : ptm::inf();
    if (hit && c.taken < (uint32_t)maxSteps) {
        const float4* mat = sc + L.offMaterial + 5 * q.materialIdx;
        const float4 specular = loadRow16(mat + 1);   // specularColor, specAvg
        const float4 misc = loadRow16(mat + 4);       // specularExponent, indexOfRefraction, flags
        const ptsp::Material m{loadRow16(mat).w, specular.w, loadRow16(mat + 2).w, misc.x, misc.y, (int)asU(misc.z)};
        const ptsp::Step s = ptsp::step(m, c.d, q.point, q.normal);
        if (s.follows) {
            c.T = c.T * ptsp::linkFactor(m, xyz(specular), c.d, q.normal);
            c.o = s.o;
            c.d = s.d;
            c.tmax = ptm::inf();
            ++c.taken;
            return;
        }
    }
    // the chain has ended: queryKernel's rows for the last link's ray, then the chain's own
    float4* h = hits + 3 * (size_t)i;
    h[0] = float4{q.point.x, q.point.y, q.point.z, q.dist};
    h[1] = float4{q.normal.x, q.normal.y, q.normal.z, asF((uint32_t)q.materialIdx)};
    h[2] = float4{asF((uint32_t)q.kind), asF((uint32_t)q.prim), q.w1, q.w2};
    if (chain) {
        chain[2 * (size_t)i] = float4{c.T.x, c.T.y, c.T.z, asF(c.taken)};
        chain[2 * (size_t)i + 1] = float4{c.d.x, c.d.y, c.d.z, c.length};
    }
    c.active = false;
}

template <bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void chainKernel(const float4* __restrict__ sceneBlob, SceneLayout L, const float4* __restrict__ rays,
                                                       float4* __restrict__ hits, float4* __restrict__ chain, uint32_t n, int maxSteps) {
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
        ChainLane c;
        c.o = c.d = v3(0, 0, 0);
        c.T = v3(1, 1, 1);
        c.tmax = c.length = ptm::inf();
        c.taken = 0;
        c.active = false;
        if (i < n) chainStart(c, rays, i);
        while (waveAny(c.active)) chainLink(sc, sceneBlob, L, c, i, maxSteps, hits, chain);   // at most maxSteps + 1 links per lane
    }
}

// Claiming, as pathRefillKernel claims: lane t of workgroup b starts with ray b * kBlock + t (the launcher keeps gridDim.x <=
// ceil(n / kBlock)); *head, set to gridDim.x * kBlock in front of the kernel, is the first ray nobody owns. A wave keeps a claimed chunk
// as a reserve [next, end) in scalar registers; before every link its dead lanes, ranked in lane order, take next, next + 1, .. from
// the reserve, then, if that ran out, from one new chunk. A wave that has seen the head at or past n claims no more and leaves the loop
// when none of its lanes is live.
template <bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void chainRefillKernel(const float4* __restrict__ sceneBlob, SceneLayout L, const float4* __restrict__ rays,
                                                             float4* __restrict__ hits, float4* __restrict__ chain, uint32_t n, int maxSteps,
                                                             uint32_t* __restrict__ head) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    const float4* sc;
    if constexpr (kSceneInLds) {   // every workgroup has rays of the static fill: whether it stages does not depend on the head
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    const uint32_t lane = laneId();
    uint32_t i = blockIdx.x * kBlock + threadIdx.x;   // the ray this lane runs
    ChainLane c;
    c.o = c.d = v3(0, 0, 0);
    c.T = v3(1, 1, 1);
    c.tmax = c.length = ptm::inf();
    c.taken = 0;
    c.active = false;
    if (i < n) chainStart(c, rays, i);
    uint32_t next = 0, end = 0;                         // the wave's reserve (wave-uniform)
    bool drained = gridDim.x * (uint32_t)kBlock >= n;   // the head is at or past n (wave-uniform)
    for (;;) {
        unsigned long long dead = __builtin_amdgcn_ballot_w64(!c.active);
        for (int step = 0; step < 2 && dead != 0ull; ++step) {
            if (next == end) {
                if (drained) break;
                uint32_t h = 0;
                if (lane == 0) h = atomicAdd(head, kChainChunk);
                h = __builtin_amdgcn_readfirstlane(h);
                drained = h >= n || n - h <= kChainChunk;
                if (h >= n) break;
                next = h;
                end = drained ? n : h + kChainChunk;
            }
            const uint32_t mine = next + rankBelow(dead);
            if (!c.active && mine < end) {   // mine < end <= n
                i = mine;
                chainStart(c, rays, i);
            }
            const uint32_t wanted = (uint32_t)__builtin_popcountll(dead), left = end - next;
            next += wanted < left ? wanted : left;
            dead = __builtin_amdgcn_ballot_w64(!c.active);
        }
        if (!waveAny(c.active)) break;
        chainLink(sc, sceneBlob, L, c, i, maxSteps, hits, chain);
    }
}

static inline unsigned chainBlocksFor(uint32_t n) { return (n + (unsigned)kBlock - 1u) / (unsigned)kBlock; }

// queryKernel's grid. No bit of ptss_launched_kernels: *launches counts instead (ptss_chain_launches)
hipError_t launchChain(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* hits, void* chain,
                       uint32_t n, int maxSteps, int maxBlocks, unsigned long long* launches) {
    unsigned blocks = chainBlocksFor(n);
    if (maxBlocks > 0 && blocks > (unsigned)maxBlocks) blocks = (unsigned)maxBlocks;
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? chainKernel<true> : chainKernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, static_cast<const float4*>(rays), static_cast<float4*>(hits),
                       static_cast<float4*>(chain), n, maxSteps);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

// launchPathRefill's grid: min(ceil(n / kBlock), cap) workgroups, cap = maxWorkgroups or, when that is 0, the workgroups of this
// instantiation the device holds at once; kept small enough that the head cannot wrap (every wave adds at most one chunk past n).
// head: the context's device word for this kernel, set to grid * kBlock by a memset node in front of it.
hipError_t launchChainRefill(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays, void* hits, void* chain,
                             uint32_t n, int maxSteps, int maxWorkgroups, int numCUs, uint32_t* head, unsigned long long* launches) {
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? chainRefillKernel<true> : chainRefillKernel<false>;
    unsigned cap = (unsigned)maxWorkgroups;
    if (cap == 0) {
        int perCU = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, kernel, kBlock, lds) != hipSuccess || perCU < 1) perCU = 1;
        cap = (unsigned)perCU * (unsigned)(numCUs > 0 ? numCUs : 1);
    }
    const unsigned wrapCap = (unsigned)((0xFFFFFFFFull - n) / ((unsigned long long)kWaves * kChainChunk));
    unsigned blocks = chainBlocksFor(n);
    if (blocks > cap) blocks = cap;
    if (blocks > wrapCap) blocks = wrapCap;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(head), (int)(blocks * (unsigned)kBlock), 1, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, static_cast<const float4*>(rays), static_cast<float4*>(hits),
                       static_cast<float4*>(chain), n, maxSteps, head);
    e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

}  // namespace ptss
