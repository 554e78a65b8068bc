// ptaccel.h — layer 2 of the device code of ptss_kernels.hip: the traversals that decide WHICH primitives a ray is tested against.
// The chunked many-sphere image (plain per-lane walk, regrouped across the wave, hybrid for shadow rays) and the two-level mesh
// image; every test they end in is ptprim.h's. They restate the sphere and triangle loops of intersectScene / lineOfSight
// (CudaTracer.cu:121-141, :437-452) for those two images. Also the home of the diagnostic counters (ptss_diag.h), which use the
// chunk-bound helpers below.
#pragma once
#include "ptprim.h"

namespace ptss {
namespace {

// what closestHit (pthit.h) returns and the many-sphere traversal fills in
struct Hit {
    float distance;
    int kind, idx;  // kind: 0 none, 1 sphere, 2 triangle
    float w0, w1, w2;
};

// ---- Scenes with many spheres (SceneLayout::accelSpheres; derivation of the test and of its constants: at the top of
// ptpack.h). The spheres sit in spatially sorted chunks of kChunkSpheres with a bounding sphere each. chunkMask is
// the wave-uniform pass over 32 chunk bounds: bit k = "this lane's ray may touch chunk k" — a conservative test that
// only ever skips spheres whose reference discriminant is certainly negative. Each lane then walks ITS chunks (per-lane
// gathers) with the reference's own tests. The visiting order is no longer the reference's, which matters only when two
// spheres are hit at exactly the same distance: the sequential `<=` rule ends on the HIGHEST index among them, so the
// closest hit keeps (minimum distance, highest original index) — identical for the finite distances this mode is
// restricted to.
constexpr int kQueueCapConst = 2 * 64;  // = kQueueCap (static_assert on the next line): segments per wave queue plane
// (the LDS work area behind the scene image — kNeeLights, kQueueCap, kWaveLdsWords, kBlockLdsVec4 — is laid out in ptscene.h)
static_assert(kQueueCap == kQueueCapConst, "anySpheresHybrid's plane stride");
constexpr float kAccelMu = 5e-3f + 5e-3f * 5e-3f;   // m + m^2
constexpr float kAccelDirEps = 1e-5f;               // | |d|^2 - 1 | up to which a direction counts as unit
constexpr float kAccelQ = 0.25f * (1.0f + 2e-5f) / (1.0f - kAccelMu) * (1.0f + 1e-6f);   // (1 + 2 eps) / (4 (1 - mu)), rounded up

// One chunk bound's verdict ("this lane's ray may touch the chunk") shifted into `rev` through the carry, as shiftInSphere does
// for spheres. ONE test (derivation: ptpack.h): with t = dv - |dv| = 2 min(dv, 0) — exact, no compare, no select —
// vv - kAccelQ t^2 is (a lower bound of) the squared distance of the chunk's centre from the RAY, the half line t >= 0: the
// line's distance while the closest approach lies ahead of the origin, the origin's own distance once it lies behind. The
// chunk is skipped when that exceeds the stored bound; the compare's wave mask is handed to v_addc as its carry-in SGPR
// pair: no v_cndmask, no v_or, no v_mov for the bit. (Until round 3 the line and a separate "wholly behind the origin's
// plane" test — two more compares, a multiply, an fma and three scalar instructions per bound, and a looser verdict: a ray
// leaving a chunk it starts beside was still sent into it.)
__device__ __forceinline__ void shiftInChunk(uint32_t& rev, float4 b, vec3 o, vec3 d) {
    const vec3 v = o - xyz(b);
    const float dv = dot(d, v);
    const float vv = dot(v, v);
    const float t = dv - ptm::abs(dv);
    const unsigned long long may = ~maskOf(ptm::fma(-kAccelQ, t * t, vv) > b.w);   // not provably out of reach (a NaN lands here too)
    asm("v_addc_co_u32 %0, vcc, %0, %0, %1" : "+v"(rev) : "s"(may) : "vcc");
}
// The same for a ray that starts at the camera (bounce 0): the row holds v = o - C and vv - bound, evaluated once per camera by
// primaryPrepKernel with the very same subtraction (the difference rounded DOWN: it can only keep a chunk) — 8 instructions
// instead of 14 per bound.
__device__ __forceinline__ void shiftInChunkPrimary(uint32_t& rev, float4 pv, vec3 d) {
    const float dv = dot(d, xyz(pv));
    const float t = dv - ptm::abs(dv);
    const unsigned long long may = ~maskOf(ptm::fma(-kAccelQ, t * t, pv.w) > 0.0f);
    asm("v_addc_co_u32 %0, vcc, %0, %0, %1" : "+v"(rev) : "s"(may) : "vcc");
}
// four bounds per trip (one address, immediate offsets; the host pads the bound rows to a multiple of four and the padding's
// bits are dropped here)
template <bool kPrimary>
__device__ __forceinline__ uint32_t chunkMask(const float4* bounds, int cnt, vec3 o, vec3 d, bool unitDir) {
    const int trips = (cnt + 3) >> 2;  // wave-uniform, 1..8
    uint32_t rev = 0;
    for (int g = 0; g < trips; ++g) {
        const float4 b0 = bounds[4 * g], b1 = bounds[4 * g + 1], b2 = bounds[4 * g + 2], b3 = bounds[4 * g + 3];
        if constexpr (kPrimary) {
            shiftInChunkPrimary(rev, b0, d);
            shiftInChunkPrimary(rev, b1, d);
            shiftInChunkPrimary(rev, b2, d);
            shiftInChunkPrimary(rev, b3, d);
        } else {
            shiftInChunk(rev, b0, o, d);
            shiftInChunk(rev, b1, o, d);
            shiftInChunk(rev, b2, o, d);
            shiftInChunk(rev, b3, o, d);
        }
    }
    const uint32_t all = (cnt >= 32) ? 0xffffffffu : ((1u << cnt) - 1u);
    return unitDir ? ((__builtin_bitreverse32(rev) >> (32 - 4 * trips)) & all) : all;
}

#include "ptss_diag.h"
#include "ptmesh.h"

// Candidate mask of ONE chunk for a lane that gathers its own rows (lanes sit in different chunks): visit i reads slot
// i ^ (chunk mod kChunkSpheres), so that the 16-byte gathers of a wave spread over the LDS banks; verdicts enter through
// the carry (shiftInSphere), so visit i lands in bit kChunkSpheres - 1 - i. chunkSlot() turns a bit of that mask back into
// the sphere's slot inside the chunk. The traversal is order-free (ties go by original index). Where the image is staged in
// LDS and the sphere rows start on a 256-byte boundary (they do: ptpack.h puts them first, the dynamic LDS is aligned), a
// row's address is (chunk's address ^ (chunk mod 16) << 4) ^ (i << 4): ONE v_xor with a constant per row instead of add, and,
// shift-add (round 3; -2 of 16 instructions per sphere).
__device__ __forceinline__ uint32_t chunkCandidates(const float4* spheres /* sc + L.offSphere */, int base, int chunk, vec3 o, vec3 d) {
    static_assert(kChunkSpheres * sizeof(float4) <= 256, "a chunk's rows must not straddle the 256-byte window the XOR walks");
    uint32_t rev = 0;
    const int twist = chunk & (kChunkSpheres - 1);
#if __HIP_DEVICE_COMPILE__   // (the host pass of this file only parses device functions; it has no LDS address space)
    if (__builtin_amdgcn_is_shared(spheres)) {   // decided at compile time wherever the image's address space is known
        const uint32_t first = (uint32_t)(uintptr_t)(LdsRow*)spheres;
        if ((first & 255u) == 0u) {   // wave-uniform
            uint32_t x = (first + (uint32_t)base * (uint32_t)sizeof(float4)) ^ ((uint32_t)twist << 4);
            asm volatile("" : "+v"(x));   // keep it one value: the compiler would re-associate it into (i ^ twist) << 4 ^ base per row
#pragma unroll
            for (int i = 0; i < kChunkSpheres; ++i) shiftInSphere<true, true>(rev, *(LdsRow*)(uintptr_t)(x ^ ((uint32_t)i << 4)), o, d);
            return rev;
        }
    }
#endif
#pragma unroll 4
    for (int i = 0; i < kChunkSpheres; ++i) shiftInSphere<true, true>(rev, spheres[base + (i ^ twist)], o, d);
    return rev;
}
__device__ __forceinline__ int chunkSlot(int bit, int chunk) { return ((kChunkSpheres - 1 - bit) ^ chunk) & (kChunkSpheres - 1); }

// The chunk bits of up to 128 chunks (4 words) are gathered first and walked in ONE per-lane loop: the wave then runs as
// long as its busiest lane's TOTAL, not the sum over 32-chunk groups of each group's busiest lane.
struct ChunkBits {
    uint32_t w[4];
};
template <bool kPrimary = false>
__device__ __forceinline__ ChunkBits chunkBits128(const float4* sc, const SceneLayout& L, int g0, vec3 o, vec3 d, bool unitDir, bool live) {
    ChunkBits b;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int g = g0 + 32 * q;
        const int left = L.numChunks - g;  // wave-uniform
        b.w[q] = (left > 0) ? chunkMask<kPrimary>(sc + (kPrimary ? L.offPrimChunk : L.offChunk) + g, left < 32 ? left : 32, o, d, unitDir) : 0u;
        if (!live) b.w[q] = 0u;
    }
    return b;
}
__device__ __forceinline__ bool anyChunk(const ChunkBits& b) { return (b.w[0] | b.w[1] | b.w[2] | b.w[3]) != 0u; }
__device__ __forceinline__ int popChunk(ChunkBits& b) {  // lowest set bit, removed
    const int q = b.w[0] ? 0 : (b.w[1] ? 1 : (b.w[2] ? 2 : 3));
    const uint32_t word = q == 0 ? b.w[0] : (q == 1 ? b.w[1] : (q == 2 ? b.w[2] : b.w[3]));
    const int k = __builtin_ctz(word);
    const uint32_t rest = word & (word - 1u);
    b.w[0] = q == 0 ? rest : b.w[0];
    b.w[1] = q == 1 ? rest : b.w[1];
    b.w[2] = q == 2 ? rest : b.w[2];
    b.w[3] = q == 3 ? rest : b.w[3];
    return 32 * q + k;
}


__device__ __forceinline__ bool anySphereChunked(const float4* sc, const SceneLayout& L, vec3 lo, vec3 w_i, float distance, bool live) {
    const bool unitDir = ptm::abs(dot(w_i, w_i) - 1.0f) <= kAccelDirEps;
    bool occluded = false;
    for (int g0 = 0; g0 < L.numChunks; g0 += 128) {
        ChunkBits chunks = chunkBits128(sc, L, g0, lo, w_i, unitDir, live && !occluded);
        while (anyChunk(chunks)) {
            const int chunk = g0 + popChunk(chunks);
            const int base = chunk * kChunkSpheres;
            uint32_t mask = chunkCandidates(sc + L.offSphere, base, chunk, lo, w_i);
            while (mask != 0) {
                const int j = chunkSlot(__builtin_ctz(mask), chunk);
                mask &= mask - 1;
                float t;
                if (sphereTest(sc[L.offSphere + base + j], lo, w_i, distance, t)) {
                    occluded = true;
                    mask = 0;
                    chunks.w[0] = chunks.w[1] = chunks.w[2] = chunks.w[3] = 0u;
                }
            }
        }
    }
    return occluded;
}

// ---- The same traversal with the work REGROUPED across the wave. In a dense scene an incoherent ray touches 30-50 chunks
// and the counts differ widely between lanes: walking them lane by lane keeps 34 % of the lanes busy
// (tools/stress_counters.sh). Here every lane publishes its ray in the wave's LDS area, an exclusive scan of the chunk
// counts numbers all (ray, chunk) pairs of the wave, every lane writes its pairs into a list at its scan position, and
// each pass hands 64 consecutive pairs to the 64 lanes: lane l reads pair q = (owner, chunk), tests the chunk's
// spheres against the OWNER's ray, and folds what it finds into the owner's slot with one 64-bit LDS minimum on the key
// (the shadow passes' regrouped part, anySpheresHybrid, still FINDS pair q: owner by bisection over the scan, chunk as the
// owner's r-th set bit — its tables sit in strided half planes of the segment queue)
// (distance bits, ~original index): minimum distance first, highest original index among equals — the order-free form
// of the reference's sequential rule (distances are >= 0 here, so their bit patterns order like the values; -0 counts as
// +0, all-NaN rays tie on the distance and end on the highest index, as the sequential loop does). The owner finally
// recomputes the winner's distance with the reference's own test, so the value it keeps has the reference's bits.
// (Shadow rays keep the per-lane walk: most of them are blocked within their first chunks, and that early exit beats
// balanced scheduling — the regrouped any-hit measured 15.2 against 11.0 ms per pass on the configs[5] scene.)
__device__ __forceinline__ uint32_t nthSetBit(uint32_t word, uint32_t r) {  // position of the r-th (0-based) set bit
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t width = 16; width >= 1; width >>= 1) {
        const uint32_t low = (uint32_t)__builtin_popcount(word & ((1u << width) - 1u));
        const bool up = r >= low;
        r -= up ? low : 0u;
        word = up ? (word >> width) : word;
        pos += up ? width : 0u;
    }
    return pos;
}

constexpr uint32_t kPairCap = 2 * 5 * 64;   // 16-bit words in the five 64-word tables between the rays and the keys
constexpr uint32_t kCandCap = 8 * kQueueCapConst + kQueueCapConst / 4 - 13 * 64;   // what the wave's LDS area holds behind the tables: 224 words
static_assert(kCandCap >= 128, "the candidate queue must take a full trip after a drain");

template <bool kPrimary>
__device__ __forceinline__ void closestSpheresRegrouped(const float4* sc, const float4* cold, const SceneLayout& L, vec3 o, vec3 d,
                                                        bool live, Hit& h, uint32_t* ws) {
    const uint32_t lane = __lane_id();
    float* rayTab = reinterpret_cast<float*>(ws);                                    // [6][64]
    uint16_t* pairQ = reinterpret_cast<uint16_t*>(ws + 6 * 64);                      // [kPairCap]: owner lane | chunk (of this group of 128) << 6
    unsigned long long* best = reinterpret_cast<unsigned long long*>(ws + 11 * 64);  // [64]
    uint32_t* candQ = ws + 13 * 64;                                                  // [kCandCap]: owner lane | sorted sphere position << 8
    const int* orig = reinterpret_cast<const int*>(cold + L.offSphereOrig);  // global memory (SceneLayout::ldsVec4)
    const int* posOf = reinterpret_cast<const int*>(cold + L.offSpherePos);
    const bool unitDir = ptm::abs(dot(d, d) - 1.0f) <= kAccelDirEps;
    // CANDIDATES, second regrouping (round 3). A (ray, chunk) pair finds few candidates among its 16 spheres — the line of a
    // ray that touches a chunk's bound meets 0.3 of the chunk's spheres on average — so resolving them where they are found
    // (a per-lane loop inside every pass: as many trips as the busiest lane has candidates, a tenth of the lanes working) was
    // the largest single piece of a mid-bounce launch (ablation builds, profiles/README.md). Instead every pass only APPENDS
    // its candidates — (owner, sphere) words, ranked by ballot — to a queue in the wave's LDS area, and the queue is resolved
    // 64 at a time with every lane busy: square root, roots, key, one LDS minimum into the owner's slot. Any order is fine
    // (the merge is a minimum on (distance, ~original index)); the queue is drained whenever a trip might not fit, and at the
    // end. (The shadow passes' regrouped part keeps resolving in place: the same queue there measured +-0 — a blocked segment
    // leaves at its first hit, and most do.)
    uint32_t candCount = 0;   // wave-uniform
    auto resolveCandidates = [&](uint32_t n) {   // the last n <= 64 entries of the queue
        const bool have = lane < n;
        const uint32_t e = candQ[candCount - n + (have ? lane : 0u)];
        const uint32_t owner = e & 63u;
        const int pos = (int)(e >> 8);
        const vec3 ro = v3(rayTab[0 * 64 + owner], rayTab[1 * 64 + owner], rayTab[2 * 64 + owner]);
        const vec3 rd = v3(rayTab[3 * 64 + owner], rayTab[4 * 64 + owner], rayTab[5 * 64 + owner]);
        float t;
        if (have && sphereTest(sc[L.offSphere + pos], ro, rd, ptm::inf(), t)) {
            const uint32_t tb = (t != t) ? 0u : asU(t + 0.0f);
            atomicMin(&best[owner], ((unsigned long long)tb << 32) | (unsigned long long)(0xffffffffu - (uint32_t)orig[pos]));
        }
        candCount -= n;
    };
    rayTab[0 * 64 + lane] = o.x;
    rayTab[1 * 64 + lane] = o.y;
    rayTab[2 * 64 + lane] = o.z;
    rayTab[3 * 64 + lane] = d.x;
    rayTab[4 * 64 + lane] = d.y;
    rayTab[5 * 64 + lane] = d.z;
    best[lane] = ~0ull;
    for (int g0 = 0; g0 < L.numChunks; g0 += 128) {
        ChunkBits mine = chunkBits128<kPrimary>(sc, L, g0, o, d, unitDir, live);
        // PAIRS. Every lane writes its (owner lane, chunk) pairs — 16-bit words, ascending chunks — into the wave's pair list
        // at the position an exclusive scan of the counts gives it; a pass then reads one word per lane. (Until round 3 a pass
        // FOUND its pairs: bisection over the scan for the owner, the owner's four bit words, the r-th set bit — 120 vector
        // instructions and eleven dependent LDS round trips per pass; the expansion is one loop per 128 chunks with as many
        // trips as the busiest lane has chunks.) A list holds kPairCap pairs; what does not fit stays in the lanes' bits for
        // the next round.
        for (;;) {
            const uint32_t cnt = (uint32_t)(__builtin_popcount(mine.w[0]) + __builtin_popcount(mine.w[1]) + __builtin_popcount(mine.w[2]) +
                                            __builtin_popcount(mine.w[3]));
            uint32_t incl = cnt;  // inclusive scan over the lanes
#pragma unroll
            for (uint32_t off = 1; off < 64; off <<= 1) {
                const uint32_t below = (uint32_t)__shfl_up((int)incl, off);
                incl += (lane >= off) ? below : 0u;
            }
            const uint32_t total = (uint32_t)__shfl((int)incl, 63);  // wave-uniform
            if (total == 0u) break;
            uint32_t pos = incl - cnt;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                while (waveAny(mine.w[w] != 0u && pos < kPairCap)) {
                    if (mine.w[w] != 0u && pos < kPairCap) {
                        const uint32_t k = (uint32_t)__builtin_ctz(mine.w[w]);
                        mine.w[w] &= mine.w[w] - 1u;
                        pairQ[pos++] = (uint16_t)(lane | ((32u * (uint32_t)w + k) << 6));
                    }
                }
            }
            const uint32_t n = total < kPairCap ? total : kPairCap;
            waveLdsFence();
            for (uint32_t q0 = 0; q0 < n; q0 += 64) {
                const bool work = q0 + lane < n;
                const uint32_t e = pairQ[work ? q0 + lane : 0u];
                const uint32_t owner = e & 63u;
                const int chunk = g0 + (int)(e >> 6);
                const int base = chunk * kChunkSpheres;
                const vec3 ro = v3(rayTab[0 * 64 + owner], rayTab[1 * 64 + owner], rayTab[2 * 64 + owner]);
                const vec3 rd = v3(rayTab[3 * 64 + owner], rayTab[4 * 64 + owner], rayTab[5 * 64 + owner]);
                uint32_t mask = chunkCandidates(sc + L.offSphere, base, chunk, ro, rd);
                if (!work) mask = 0;
                while (waveAny(mask != 0)) {   // one trip per candidate of the busiest lane: append, do not resolve
                    if (candCount + 64u > kCandCap) {   // wave-uniform: make room first
                        waveLdsFence();
                        while (candCount >= 64u) resolveCandidates(64u);
                        waveLdsFence();
                    }
                    const bool has = mask != 0;
                    const unsigned long long m = __ballot(has);
                    if (has) {
                        const int j = chunkSlot(__builtin_ctz(mask), chunk);
                        mask &= mask - 1;
                        candQ[candCount + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = owner | ((uint32_t)(base + j) << 8);
                    }
                    candCount += (uint32_t)__popcll(m);
                }
            }
            waveLdsFence();
            if (total <= kPairCap) break;
        }
        waveLdsFence();
        while (candCount != 0u) resolveCandidates(candCount < 64u ? candCount : 64u);
        waveLdsFence();
    }
    const unsigned long long won = best[lane];
    PTSS_DIAG_CULL(sc, L, o, d, unitDir, live, won);
    if (live && won != ~0ull) {
        const int pos = posOf[0xffffffffu - (uint32_t)won];
        float t;
        (void)sphereTest(sc[L.offSphere + pos], o, d, ptm::inf(), t);  // the winner's distance, with the reference's bits
        h.distance = t;
        h.kind = 1;
        h.idx = pos;
    }
    waveLdsFence();
}

// ---- Shadow rays of a dense queue pass, hybrid: a blocked segment is usually blocked within its first chunks, so every
// lane walks up to kWarmChunks of its own chunks first (cheap early exits); what is left belongs to the long walkers —
// the segments that reach their light have to visit all 30-50 chunks — and is regrouped across the wave like the closest
// hit's work (closestSpheresRegrouped), the merge being "set the owner's blocked flag". The tables live in the half of
// the wave's queue planes that the current pass does not read (tab[plane] = that half of plane `plane`), which is why
// the caller uses this only for a pass whose other half is free.
// chunks of 16 in kd order, configs[4]'s scene at S = 4, same box: 0: 4,571, 1: 4,589, 2: 4,597-4,605, 3: 4,585, 4: 4,535,
// 8: 4,270, 16: 4,189 Mrays/s; again with round 3's tighter bounds: 0: 5,866, 1: 5,901, 2: 5,931, 3: 5,835, 4: 5,738
constexpr int kWarmChunks = 2;

__device__ __forceinline__ bool anySpheresHybrid(const float4* sc, const SceneLayout& L, const float* seg, float* tab, vec3 lo,
                                                 vec3 w_i, float distance, bool have) {
    const uint32_t lane = __lane_id();
    uint32_t* bits0 = reinterpret_cast<uint32_t*>(tab + 0 * kQueueCapConst);
    uint32_t* bits1 = reinterpret_cast<uint32_t*>(tab + 1 * kQueueCapConst);
    uint32_t* bits2 = reinterpret_cast<uint32_t*>(tab + 2 * kQueueCapConst);
    uint32_t* bits3 = reinterpret_cast<uint32_t*>(tab + 3 * kQueueCapConst);
    uint32_t* startTab = reinterpret_cast<uint32_t*>(tab + 4 * kQueueCapConst);
    uint32_t* blocked = reinterpret_cast<uint32_t*>(tab + 5 * kQueueCapConst);
    const bool unitDir = ptm::abs(dot(w_i, w_i) - 1.0f) <= kAccelDirEps;
    bool occluded = false;
    for (int g0 = 0; g0 < L.numChunks; g0 += 128) {
        ChunkBits mine = chunkBits128(sc, L, g0, lo, w_i, unitDir, have && !occluded);
        for (int it = 0; it < kWarmChunks; ++it) {  // own walk
            if (!waveAny(anyChunk(mine))) break;
            if (anyChunk(mine)) {
                const int chunk = g0 + popChunk(mine);
                const int base = chunk * kChunkSpheres;
                uint32_t mask = chunkCandidates(sc + L.offSphere, base, chunk, lo, w_i);
                while (mask != 0) {
                    const int j = chunkSlot(__builtin_ctz(mask), chunk);
                    mask &= mask - 1;
                    float t;
                    if (sphereTest(sc[L.offSphere + base + j], lo, w_i, distance, t)) {
                        occluded = true;
                        mask = 0;
                        mine.w[0] = mine.w[1] = mine.w[2] = mine.w[3] = 0u;
                    }
                }
            }
        }
        if (!waveAny(anyChunk(mine))) continue;
        // the rest, regrouped
        bits0[lane] = mine.w[0];
        bits1[lane] = mine.w[1];
        bits2[lane] = mine.w[2];
        bits3[lane] = mine.w[3];
        blocked[lane] = occluded ? 1u : 0u;
        const uint32_t cnt = (uint32_t)(__builtin_popcount(mine.w[0]) + __builtin_popcount(mine.w[1]) + __builtin_popcount(mine.w[2]) +
                                        __builtin_popcount(mine.w[3]));
        uint32_t incl = cnt;
#pragma unroll
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint32_t below = (uint32_t)__shfl_up((int)incl, off);
            incl += (lane >= off) ? below : 0u;
        }
        startTab[lane] = incl - cnt;
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        waveLdsFence();
        for (uint32_t q0 = 0; q0 < total; q0 += 64) {
            const uint32_t q = q0 + lane;
            const bool valid = q < total;
            uint32_t a = 0, b = 64;
#pragma unroll
            for (int step = 0; step < 6; ++step) {
                const uint32_t mid = (a + b) >> 1;
                const bool right = startTab[mid] <= q;
                a = right ? mid : a;
                b = right ? b : mid;
            }
            const uint32_t owner = valid ? a : lane;
            uint32_t r = valid ? q - startTab[owner] : 0u;
            uint32_t word = 0, wordIdx = 0;
            bool found = false;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t bits = (w == 0 ? bits0 : (w == 1 ? bits1 : (w == 2 ? bits2 : bits3)))[owner];
                const uint32_t pc = (uint32_t)__builtin_popcount(bits);
                const bool here = !found && r < pc;
                word = here ? bits : word;
                wordIdx = here ? (uint32_t)w : wordIdx;
                found = found || here;
                r -= (!found) ? pc : 0u;
            }
            const bool work = valid && found && blocked[owner] == 0u;
            const int chunk = g0 + (int)(32u * wordIdx + nthSetBit(word, r));
            const int base = (work ? chunk : 0) * kChunkSpheres;
            const vec3 so = v3(seg[0 * kQueueCapConst + owner], seg[1 * kQueueCapConst + owner], seg[2 * kQueueCapConst + owner]);
            const vec3 sd = v3(seg[3 * kQueueCapConst + owner], seg[4 * kQueueCapConst + owner], seg[5 * kQueueCapConst + owner]);
            const float reach = seg[6 * kQueueCapConst + owner];
            uint32_t mask = chunkCandidates(sc + L.offSphere, base, chunk, so, sd);
            if (!work) mask = 0;
            while (mask != 0) {
                const int j = chunkSlot(__builtin_ctz(mask), chunk);
                mask &= mask - 1;
                float t;
                if (sphereTest(sc[L.offSphere + base + j], so, sd, reach, t)) {
                    blocked[owner] = 1u;
                    mask = 0;
                }
            }
        }
        waveLdsFence();
        occluded = blocked[lane] != 0u;
        waveLdsFence();
    }
    return occluded;
}

// ---- The mesh image (SceneLayout::mesh; the bound: ptmesh.h, its derivation: ptpack.h packMeshBounds). The
// triangles sit in a kd order of their centroids: every kMeshLeaf consecutive positions a leaf, every kMeshLeaf leaves a group,
// each with a conservative bound. A wave-uniform pass over the group bounds (four per trip, verdicts through the carry as in
// chunkMask) gives every lane the groups its ray may touch; each lane then walks ITS groups, tests their leaf bounds, and walks
// its leaves' triangles (per-lane gathers from global memory) with the keyed general body: the order-free minimum of
// (distance, 0xFFFFFFFE - original index) is what the reference's sequential `dist <= distance` rule ends on.
// What the bound needs of a query, tested once per wave (its live lanes): |d|^2 within kMeshDirEps of 1, |o|^2 < 2^80 (finite). Together with the
// image's |coordinate| <= 2^40 that also keeps |det| < 2^126 (the reciprocal's fast range) and e2 . r finite. A wave with
// any other lane walks every triangle in the caller's order with the guarded test (closestHit's last loop).
__device__ __forceinline__ bool meshQueryOk(vec3 o, vec3 d, bool live) {   // (lanes without a query do not count)
    return waveAll(!live || (ptm::abs(dot(d, d) - 1.0f) <= ptmesh::kMeshDirEps && dot(o, o) < 0x1p80f));
}
__device__ __forceinline__ bool meshMay(const float4* b, vec3 o, vec3 d) {
    const float4 r0 = loadRow16(b), r1 = loadRow16(b + 1), r2 = loadRow16(b + 2);
    return ptmesh::mayTouch(xyz(r0), r0.w, xyz(r1), r1.w, r2.x, r2.y, r2.z, r2.w, o, d, 1.0f);
}
// bit k = "the ray may touch group g0 + k", k < cnt <= 32 (the host pads the group rows to a multiple of four bounds)
__device__ __forceinline__ uint32_t meshGroupMask(const float4* groups, int cnt, vec3 o, vec3 d) {
    const int trips = (cnt + 3) >> 2;
    uint32_t rev = 0;
    for (int g = 0; g < trips; ++g) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long may = maskOf(meshMay(groups + 3 * (4 * g + k), o, d));
            asm("v_addc_co_u32 %0, vcc, %0, %0, %1" : "+v"(rev) : "s"(may) : "vcc");
        }
    }
    return (__builtin_bitreverse32(rev) >> (32 - 4 * trips)) & lowBits(cnt);
}
// bit j = "the ray may touch leaf kMeshLeaf * g + j" (per lane: lanes sit in different groups)
__device__ __forceinline__ uint32_t meshLeafMask(const float4* leaves, int g, int numLeaves, vec3 o, vec3 d) {
    const int first = g * kMeshLeaf;
    const int cnt = numLeaves - first < kMeshLeaf ? numLeaves - first : kMeshLeaf;
    uint32_t m = 0;
    for (int j = 0; j < cnt; ++j) m |= meshMay(leaves + 3 * (first + j), o, d) ? (1u << j) : 0u;
    return m;
}
__device__ __forceinline__ const float4* meshLeaves(const float4* sc, const float4* cold, const SceneLayout& L) {
    return (L.mesh.offLeaf < L.ldsVec4 ? sc : cold) + L.mesh.offLeaf;   // staged when they fit (ptpack.h layoutMesh)
}
template <bool kPrimary>
__device__ __forceinline__ void closestTrianglesMesh(const float4* sc, const float4* cold, const SceneLayout& L, vec3 o, vec3 d, bool live,
                                                     TriBest& best) {
    const float4* leaves = meshLeaves(sc, cold, L);
    for (int g0 = 0; g0 < L.mesh.numGroups; g0 += 32) {
        const int left = L.mesh.numGroups - g0;   // wave-uniform
        uint32_t groups = meshGroupMask(sc + L.mesh.offGroup + 3 * g0, left < 32 ? left : 32, o, d);
        if (!live) groups = 0u;
        while (groups != 0u) {
            const int g = g0 + __builtin_ctz(groups);
            groups &= groups - 1u;
            uint32_t leafBits = meshLeafMask(leaves, g, L.mesh.numLeaves, o, d);
            while (leafBits != 0u) {
                const int t0 = (g * kMeshLeaf + __builtin_ctz(leafBits)) * kMeshLeaf;
                leafBits &= leafBits - 1u;
                const int t1 = L.numTriangles - t0 < kMeshLeaf ? L.numTriangles : t0 + kMeshLeaf;
                for (int t = t0; t < t1; ++t)
                    triangleClassed<kPrimary, 0, 0, true>(cold + L.offTri + 3 * t, cold + L.offPrimTri + 2 * t, 0u, o, d, ~0ull, best);
            }
        }
    }
}
// the triangle half of lineOfSight on the mesh image: the same two levels against the segment, each lane stopping at its first
// blocker (an OR over independent tests: any order); outside the derivation's domain, every triangle with the guarded test
__device__ __forceinline__ bool anyTrianglesMesh(const float4* sc, const float4* cold, const SceneLayout& L, vec3 o, vec3 d, float limit, bool live) {
    if (!meshQueryOk(o, d, live)) {
        unsigned long long need = maskOf(live), blocked = 0ull;
        for (int i = 0; i < L.numTriangles; ++i) {
            if (need == 0ull) break;
            const TriHit th = triangleTest(loadTri(cold + L.offTri + 3 * i), o, d, limit, need);
            blocked |= th.hitMask;
            need &= ~th.hitMask;
        }
        return __builtin_amdgcn_inverse_ballot_w64(blocked);
    }
    const float4* leaves = meshLeaves(sc, cold, L);
    bool blocked = false;
    for (int g0 = 0; g0 < L.mesh.numGroups; g0 += 32) {
        if (!waveAny(live && !blocked)) break;
        const int left = L.mesh.numGroups - g0;
        uint32_t groups = meshGroupMask(sc + L.mesh.offGroup + 3 * g0, left < 32 ? left : 32, o, d);
        if (!live || blocked) groups = 0u;
        while (groups != 0u) {
            const int g = g0 + __builtin_ctz(groups);
            groups &= groups - 1u;
            uint32_t leafBits = meshLeafMask(leaves, g, L.mesh.numLeaves, o, d);
            while (leafBits != 0u) {
                const int t0 = (g * kMeshLeaf + __builtin_ctz(leafBits)) * kMeshLeaf;
                leafBits &= leafBits - 1u;
                const int t1 = L.numTriangles - t0 < kMeshLeaf ? L.numTriangles : t0 + kMeshLeaf;
                for (int t = t0; t < t1; ++t) {
                    const float4* r = cold + L.offTri + 3 * t;
                    const pttri::Head hh = pttri::head<0, 0, false>(xyz(loadRow16(r)), xyz(loadRow16(r + 1)), xyz(loadRow16(r + 2)), v3(0, 0, 0),
                                                                    v3(0, 0, 0), 0.0f, o, d);
                    if (pttri::passesHead(hh, limit)) {
                        float b0, b1, b2;
                        pttri::weights<0, 0>(hh, d, b0, b1, b2);
                        if (pttri::passesWeights(b0, b1, b2)) {
                            blocked = true;
                            break;
                        }
                    }
                }
                if (blocked) leafBits = 0u;
            }
            if (blocked) groups = 0u;
        }
    }
    return blocked;
}

}  // namespace
}  // namespace ptss
