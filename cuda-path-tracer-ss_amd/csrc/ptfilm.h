// ptfilm.h — what the film kernels of a path query share (ptss_film.hip, ptss_adaptive.hip, ptss_linear.hip, ptss_splat.hip, ptss_meter.hip,
// ptss_glare.hip, ptss_resolve.hip): the tail of a launch function, the count of an index's dropped
// entries, the resolve of an 8-bit film entry, the read of a glare pyramid's entry, the reduction that sums a wave's runs of equal
// pixels into each run's head lane, and a wave's sum and inclusive scan. Like the layer headers it is private to the one translation unit that includes it.
#pragma once
#include "ptwave.h"
#include "ptdenoise.h"

namespace ptss {
namespace {

inline unsigned filmBlocksFor(uint32_t n, unsigned block) { return (n + block - 1) / block; }

// the tail of a launch function: the error of the launch just enqueued, which is counted if it succeeded
inline hipError_t counted(unsigned long long* launches) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) ++*launches;
    return e;
}

// dropped entries of one wave, counted with one atomic: `dropped` is the lane's own verdict
__device__ __forceinline__ void countDropped(bool dropped, unsigned long long* rejected) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(dropped);
    if (m == 0ull) return;
    const uint32_t before = rankBelow(m);   // dropped lanes below this one
    if (dropped && before == 0u) atomicAdd(rejected, (unsigned long long)__popcll(m));
}

// finishPath's display pixel and ptdn::displayValue of one film entry
__device__ __forceinline__ void resolveEntry(uint4 e, uint32_t p, ptss_uchar4* __restrict__ pixels, float4* __restrict__ history) {
    const float inv = ptm::rcp((float)e.w);   // 1.f / (float)samples, correctly rounded
    if (pixels) {
        const uint32_t px = (uint32_t)(unsigned char)(e.x * inv + 0.5f) | ((uint32_t)(unsigned char)(e.y * inv + 0.5f) << 8) |
                            ((uint32_t)(unsigned char)(e.z * inv + 0.5f) << 16) | (255u << 24);
        reinterpret_cast<uint32_t*>(pixels)[p] = px;   // uchar4 {x, y, z, w = 255}
    }
    if (history) {
        const vec3 c = ptdn::displayValue(e.x, e.y, e.z, inv);
        history[p] = float4{c.x, c.y, c.z, (float)e.w};
    }
}

// the three channels of entry e of a glare level (ptss_glare_entry: 32 B, read as two 16-byte rows)
__device__ __forceinline__ void loadEntry(const ulonglong2* __restrict__ level, size_t e, unsigned long long* v) {
    const ulonglong2 rg = level[2 * e], bz = level[2 * e + 1];
    v[0] = rg.x, v[1] = rg.y, v[2] = bz.x;
}

// The segmented reduction of the scatter kernels: the lanes of a wave that hold one key side by side are summed towards the run's first
// lane. step(d, joins) is called for d = 1, 2, .. 32 by every lane; it shuffles its own words down by d (every lane must, whatever
// `joins` says) and adds them where `joins` is set — lane + d then belongs to this lane's run. Words and packing are the caller's.
// Returns "this lane is the first of its run": after the last step such a lane holds its run's sums. A run is split at the wave's edge.
template <class Step>
__device__ __forceinline__ bool sumRunsToHead(uint32_t key, Step step) {
    const uint32_t lane = laneId();
    const uint32_t before = (uint32_t)__shfl_up((int)key, 1, 64);
    const bool head = lane == 0u || key != before;
    const unsigned long long heads = __builtin_amdgcn_ballot_w64(head);
    // heads strictly above this lane, bit k - 1 = lane + k: lane + d joins while none of lanes lane + 1 .. lane + d starts a run
    const unsigned long long above = lane < 63u ? heads >> (lane + 1u) : ~0ull;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) step(d, lane + d < 64u && (above & ((1ull << d) - 1ull)) == 0ull);
    return head;
}

// the sum of v over the lanes of a wave, in every lane
__device__ __forceinline__ uint32_t waveSum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// inclusive sum over the lanes of a wave: lane `lane` gets the sum of lanes 0 .. lane (Word: unsigned, 32 or 64 bits)
template <class Word>
__device__ __forceinline__ Word waveScan(Word v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const Word o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

}  // namespace
}  // namespace ptss
