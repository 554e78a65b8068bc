// ptss_lightmap.hip — the kernels behind ptss_lookup_lightmap (include/ptss.h): from hits and the block tables of a
// baked light map to linear film rows. The arithmetic is csrc/ptlightmap.h, shared with the host probe (ptss_probe_lookup_lightmap:
// the specification); this file only moves the data.
//
// Per hit: rows 1 and 2 of the ptss_ray_hit (16 B each), one block row, up to four scattered texels of the map (two 16-byte rows each),
// up to twelve 64-bit divisions (a texel's integer means; gfx950 has no 64-bit division, and a texel with samples == 1 needs none), up
// to two material rows, one 32-byte store. Nothing is staged in LDS: the gathers are per hit. Every address is formed from an index
// that ptlightmap.h has held against the caller's counts first (tableRow, blockVerdict): a bad hit or block row is counted, never
// dereferenced. Two forms with the same bytes:
//   <kQuad = false>   one lane per hit: all four taps and all divisions
//   <kQuad = true>    four adjacent lanes per hit, lane t of the quad reads tap t and divides its three means; W and the three
//                     two-word sums travel across the quad through two DPP quad permutes each (no LDS); lane 0 of the quad divides
//                     by W, shades and stores
// Which one ships is kLightmapQuad below. lightmapChainKernel (ptss_lookup_lightmap_chain) is the one-lane form with the
// header's step 6, a tint by a chain's throughput, behind the lookup. Verdicts are counted with one atomic per wave and count; no bit of ptss_launched_kernels.
#include <hip/hip_runtime.h>

#include "ptss_device.h"
#include "ptlightmap.h"
#include "ptfilm.h"

namespace ptss {

constexpr int kLightmapBlock = 256;

// The form the library ships: one lane per hit. Measured over the 2,073,600 hits of a 1080p camera (tools/lightmap_bench.py;
// profiles/lightmap/), five interleaved pairs of windows per filter and scene: 0.046 ms against 0.090 ms (bilinear, the
// 1,296-triangle mesh scene), 0.049 against 0.102 ms (`mixed`), one lane faster in every pair. The hits of neighbouring pixels share
// their texels, so the four-lane form's gain — a quarter of the divisions per lane — buys nothing a cache hit had not already paid for,
// and it launches four times the waves, each repeating the hit's loads and the place. It lost and stays compiled for the tests and the tool.
constexpr bool kLightmapQuad = false;

struct LightmapArgs {
    ptlm::Rule rule;
    int offMaterial;   // the image's material rows
};

__device__ __forceinline__ ptlm::Hit hitOf(const float4* __restrict__ hits, uint32_t i) {
    const float4 r1 = hits[3 * (size_t)i + 1], r2 = hits[3 * (size_t)i + 2];
    return ptlm::Hit{xyz(r1), (int)asU(r1.w), (int)asU(r2.x), (int)asU(r2.y), r2.z, r2.w};
}

__device__ __forceinline__ ptlm::Block blockOf(const int4* __restrict__ table, int row) {
    const int4 b = table[row];
    return ptlm::Block{b.x, b.y, b.z, b.w};
}

__device__ __forceinline__ ptlm::Texel texelAt(const ulonglong2* __restrict__ map, uint32_t texel) {
    const ulonglong2 rg = map[2 * (size_t)texel], bw = map[2 * (size_t)texel + 1];
    return ptlm::Texel{rg.x, rg.y, bw.x, (uint32_t)bw.y};
}

// the verdicts of a wave, one atomic per count that is not zero; every lane of the wave calls it (counts = false: not this lane's to count)
__device__ __forceinline__ void countVerdicts(bool counts, int verdict, uint32_t* __restrict__ info) {
    if (!info) return;   // (wave-uniform: a kernel argument)
    const uint32_t lane = laneId();
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(counts && verdict == v);
        if (m != 0ull && lane == 0u) atomicAdd(info + v, (uint32_t)__popcll(m));
    }
}

__device__ __forceinline__ void storeRow(ulonglong2* __restrict__ out, uint32_t i, int verdict, const unsigned long long* m) {
    out[2 * (size_t)i] = ulonglong2{m[0], m[1]};
    out[2 * (size_t)i + 1] = ulonglong2{m[2], verdict == ptlm::kFiltered ? 1ull : 0ull};   // samples = 1, clamped = 0
}

// lane ^ 1 and lane ^ 2 of a quad: quad_perm [1, 0, 3, 2] and [2, 3, 0, 1]
template <int kCtrl>
__device__ __forceinline__ uint32_t quadRead(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xf, 0xf, true);
}

template <int kCtrl>
__device__ __forceinline__ void quadAdd(ptlm::Sums& S) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long lo = (unsigned long long)quadRead<kCtrl>((uint32_t)S.s[c].lo) |
                                      ((unsigned long long)quadRead<kCtrl>((uint32_t)(S.s[c].lo >> 32)) << 32);
        const unsigned long long hi = quadRead<kCtrl>((uint32_t)S.s[c].hi);   // a term's high word is below 2^16
        S.s[c] = ptlm::add128(S.s[c], ptlm::U128{lo, hi});
    }
    S.W += quadRead<kCtrl>(S.W);
}

template <bool kQuad>
__global__ __launch_bounds__(kLightmapBlock) void lightmapKernel(const float4* __restrict__ blob, LightmapArgs A, const int4* __restrict__ blocksTri,
                                                                 const int4* __restrict__ blocksSph, const ulonglong2* __restrict__ map,
                                                                 const float4* __restrict__ hits, uint32_t n, ulonglong2* __restrict__ out,
                                                                 uint32_t* __restrict__ info) {
    const ptlm::Rule& R = A.rule;
    auto material = [&](int idx, int row) { return xyz(blob[A.offMaterial + 5 * (size_t)idx + row]); };
    unsigned long long m[3] = {0ull, 0ull, 0ull};
    if constexpr (!kQuad) {
        const uint32_t i = blockIdx.x * kLightmapBlock + threadIdx.x;
        const bool inBatch = i < n;
        int verdict = ptlm::kRejected;
        if (inBatch) {
            verdict = ptlm::lookup(
                hitOf(hits, i), R, [&](int row) { return blockOf(blocksTri, row); }, [&](int row) { return blockOf(blocksSph, row); },
                [&](uint32_t texel) { return texelAt(map, texel); }, material, m);
            storeRow(out, i, verdict, m);
        }
        countVerdicts(inBatch, verdict, info);
    } else {
        const uint32_t i = blockIdx.x * (kLightmapBlock / 4) + (threadIdx.x >> 2);   // a quad is wholly inside the batch or outside
        const int t = (int)(threadIdx.x & 3u);
        const bool inBatch = i < n;
        int verdict = ptlm::kRejected;
        ptlm::Hit h{};
        ptlm::Sums S = ptlm::noSums();
        if (inBatch) {
            h = hitOf(hits, i);
            bool sphere;
            int row;
            verdict = ptlm::tableRow(h, R, &sphere, &row);
            if (verdict == ptlm::kFiltered) {
                const ptlm::Block b = blockOf(sphere ? blocksSph : blocksTri, row);
                verdict = ptlm::blockVerdict(b, h, R);
                if (verdict == ptlm::kFiltered) {
                    const ptlm::Place p = ptlm::placeOf(h, sphere, b, R.filter);
                    uint32_t texel;
                    const uint32_t w = ptlm::tapOf(p, t, R.atlasWidth, &texel);
                    if (w != 0u) ptlm::addTap(S, w, texelAt(map, texel));
                }
            }
        }
        // every lane of the wave is here: the permutes read whole quads
        quadAdd<0xB1>(S);
        quadAdd<0x4E>(S);
        if (verdict == ptlm::kFiltered && S.W == 0u) verdict = ptlm::kEmpty;
        const bool mine = inBatch && t == 0;
        if (mine) {
            if (verdict == ptlm::kFiltered) {
                vec3 diffuse = v3(0, 0, 0), emission = v3(0, 0, 0);
                if (R.flags & PTSS_LIGHTMAP_MODULATE) diffuse = material(h.materialIdx, 0);
                if (R.flags & PTSS_LIGHTMAP_EMISSION) emission = material(h.materialIdx, 3);
                m[0] = ptlm::shade(ptlm::divRound(S.s[0], S.W), R.flags, diffuse.x, emission.x, R);
                m[1] = ptlm::shade(ptlm::divRound(S.s[1], S.W), R.flags, diffuse.y, emission.y, R);
                m[2] = ptlm::shade(ptlm::divRound(S.s[2], S.W), R.flags, diffuse.z, emission.z, R);
            }
            storeRow(out, i, verdict, m);
        }
        countVerdicts(mine, verdict, info);
    }
}

// ptss_lookup_lightmap_chain: the one-lane form with ptlightmap.h's step 6 behind the lookup — the first row of the
// hit's ptss_chain_result (16 B: the throughput, never trusted: ptlm::tint clamps it) tints a FILTERED row. A kernel of its own, so that
// lightmapKernel's two instantiations stay what they were.
__global__ __launch_bounds__(kLightmapBlock) void lightmapChainKernel(const float4* __restrict__ blob, LightmapArgs A, const int4* __restrict__ blocksTri,
                                                                      const int4* __restrict__ blocksSph, const ulonglong2* __restrict__ map,
                                                                      const float4* __restrict__ hits, const float4* __restrict__ chain, uint32_t n,
                                                                      ulonglong2* __restrict__ out, uint32_t* __restrict__ info) {
    const ptlm::Rule& R = A.rule;
    auto material = [&](int idx, int row) { return xyz(blob[A.offMaterial + 5 * (size_t)idx + row]); };
    unsigned long long m[3] = {0ull, 0ull, 0ull};
    const uint32_t i = blockIdx.x * kLightmapBlock + threadIdx.x;
    const bool inBatch = i < n;
    int verdict = ptlm::kRejected;
    if (inBatch) {
        verdict = ptlm::lookup(
            hitOf(hits, i), R, [&](int row) { return blockOf(blocksTri, row); }, [&](int row) { return blockOf(blocksSph, row); },
            [&](uint32_t texel) { return texelAt(map, texel); }, material, m);
        if (verdict == ptlm::kFiltered) {
            const float4 t = chain[2 * (size_t)i];
            m[0] = ptlm::tint(m[0], t.x);
            m[1] = ptlm::tint(m[1], t.y);
            m[2] = ptlm::tint(m[2], t.z);
        }
        storeRow(out, i, verdict, m);
    }
    countVerdicts(inBatch, verdict, info);
}

hipError_t launchLookupLightmapChain(hipStream_t st, const float4* sceneBlob, const SceneLayout& L, const ptss_lightmap_params& params,
                                     const ptss_linear_params& film, const void* blocksTri, const void* blocksSph, const void* map, const void* hits,
                                     const void* chain, uint32_t n, void* out, void* info, unsigned long long* launches) {
    LightmapArgs A;
    A.rule = ptlm::ruleOf(params, film, L.numMaterials);
    A.offMaterial = L.offMaterial;
    hipLaunchKernelGGL(lightmapChainKernel, dim3(filmBlocksFor(n, kLightmapBlock)), dim3(kLightmapBlock), 0, st, sceneBlob, A,
                       static_cast<const int4*>(blocksTri), static_cast<const int4*>(blocksSph), static_cast<const ulonglong2*>(map),
                       static_cast<const float4*>(hits), static_cast<const float4*>(chain), n, static_cast<ulonglong2*>(out),
                       static_cast<uint32_t*>(info));
    return counted(launches);
}

hipError_t launchLookupLightmap(hipStream_t st, const float4* sceneBlob, const SceneLayout& L, const ptss_lightmap_params& params,
                                const ptss_linear_params& film, const void* blocksTri, const void* blocksSph, const void* map, const void* hits,
                                uint32_t n, int form, void* out, void* info, unsigned long long* launches) {
    const bool quad = form == 2 || (form == 0 && kLightmapQuad);   // form: 0 the shipped one, 1 one lane per hit, 2 four lanes per hit
    LightmapArgs A;
    A.rule = ptlm::ruleOf(params, film, L.numMaterials);
    A.offMaterial = L.offMaterial;
    const dim3 grid(filmBlocksFor(n, quad ? kLightmapBlock / 4 : kLightmapBlock)), block(kLightmapBlock);
    hipLaunchKernelGGL(quad ? lightmapKernel<true> : lightmapKernel<false>, grid, block, 0, st, sceneBlob, A, static_cast<const int4*>(blocksTri),
                       static_cast<const int4*>(blocksSph), static_cast<const ulonglong2*>(map), static_cast<const float4*>(hits), n,
                       static_cast<ulonglong2*>(out), static_cast<uint32_t*>(info));
    return counted(launches);
}

}  // namespace ptss
