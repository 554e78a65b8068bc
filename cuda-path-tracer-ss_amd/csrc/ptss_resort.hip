// ptss_resort.hip — the kernels behind ptss_resort_triangles (include/ptss.h): the triangles of a live mesh image
// are put back into the kd order a fresh pack of their CURRENT vertices would give them, on the device, with no host round trip.
// The rule is csrc/ptorder.h, shared with the host probe (ptss_probe_kd_order); this file lays it over the device:
//   resortInitKernel      the three centroid codes of every original index, the identity order, one segment [0, T)
//   per level:            resortExtentKernel   segmented minima / maxima of the codes -> each segment's axis
//                         resortKeyKernel      (segment, code along the axis) keys by ORIGINAL index; every position's child segment
//                         rocprim::radix_sort_pairs of (key, original index) from the identity order: stable, so ties fall in index order
//   resortGatherKernel    the rows of offTri, offTriNormal and offTriVert gathered into scratch in the new order
//   resortLightsKernel    the two stored positions of every area-light row renamed
//   resortScatterKernel   scratch -> image, offTriPos rewritten
// and the caller then refits the bounds with the existing meshRefitKernel. Every index that was read from device memory is
// compared with T before it addresses anything: a wrong sort gives a wrong image, never a fault.
#include <cstring>

#include <hip/hip_runtime.h>

#include <rocprim/rocprim.hpp>

#include "ptorder.h"
#include "ptss_device.h"

namespace ptss {

namespace {
constexpr int kResortBlock = 256;
constexpr int kRowsPerTri = 8;   // 3 of offTri, 3 of offTriNormal, 2 of offTriVert

}  // namespace

// One thread per ORIGINAL index i: the codes of its centroid (v0 from row 0 of offTri, v1 and v2 from offTriVert — the caller's
// exact vertices), and the start of the level loop: order[i] = iota[i] = i, segment [0, T).
__global__ __launch_bounds__(kResortBlock) void resortInitKernel(const float4* __restrict__ blob, int T, int offTri, int offTriVert, int offTriPos,
                                                                 uint32_t* __restrict__ codes, int* __restrict__ iota, int* __restrict__ order,
                                                                 int2* __restrict__ seg, int* __restrict__ newPos) {
    const int i = blockIdx.x * kResortBlock + threadIdx.x;
    if (i >= T) return;
    const uint32_t pos = reinterpret_cast<const uint32_t*>(blob + offTriPos)[i];
    float4 v0 = float4{0, 0, 0, 0}, v1 = v0, v2 = v0;
    if (pos < (uint32_t)T) {
        v0 = blob[offTri + 3 * (size_t)pos];
        v1 = blob[offTriVert + 2 * (size_t)pos];
        v2 = blob[offTriVert + 2 * (size_t)pos + 1];
    }
    codes[i] = ptorder::orderCode(ptorder::centroid(v0.x, v1.x, v2.x));
    codes[(size_t)T + i] = ptorder::orderCode(ptorder::centroid(v0.y, v1.y, v2.y));
    codes[2 * (size_t)T + i] = ptorder::orderCode(ptorder::centroid(v0.z, v1.z, v2.z));
    iota[i] = i;
    order[i] = i;
    seg[i] = int2{0, T};
    newPos[i] = pos < (uint32_t)T ? (int)pos : i;   // (overwritten by the gather; never left unset, whatever the sort delivers)
}

// extent[6 s + a] = min code along a, extent[6 s + 3 + a] = min of ~code (the maximum, so that one fill with 0xFF resets both), s =
// lo >> 4 of the segment. One lane per POSITION, a wave walking kExtentRuns consecutive runs of 64 positions. Segments begin at
// multiples of 16, so the 16 lanes of an aligned group always share one: they reduce by lane exchange and their first lane sends
// the atomics. A run that lies inside ONE segment — every run of the upper levels — is instead merged lane by lane into what the
// wave holds for that segment, reduced and sent once when the segment changes or the wave ends: at the root level that is one set
// of atomics per 512 positions instead of one per lane (the six addresses of a large segment take every wave's atomics in turn).
constexpr int kExtentRuns = 8;
__global__ __launch_bounds__(kResortBlock) void resortExtentKernel(int T, const uint32_t* __restrict__ codes, const int* __restrict__ order,
                                                                   const int2* __restrict__ seg, uint32_t* __restrict__ extent) {
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * kResortBlock + threadIdx.x) >> 6;
    auto exchange = [](uint32_t (&v)[6], int first, int last) {   // minima across lanes that differ in the bits first .. last
        for (int mask = first; mask <= last; mask *= 2)
            for (int k = 0; k < 6; ++k) {
                const uint32_t o = (uint32_t)__shfl_xor((int)v[k], mask, 64);
                v[k] = o < v[k] ? o : v[k];
            }
    };
    int heldLo = -1;   // wave-uniform: the segment whose partial minima the lanes hold, or -1
    bool heldAny = false;
    uint32_t held[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
    auto flush = [&]() {   // (wave-uniform control flow: every lane calls it)
        if (heldLo >= 0 && heldAny) {
            exchange(held, 1, 32);
            if (lane == 0)
                for (int k = 0; k < 6; ++k) atomicMin(extent + 6 * (size_t)((uint32_t)heldLo >> ptorder::kSegShift) + k, held[k]);
        }
        heldLo = -1;
        heldAny = false;
        for (int k = 0; k < 6; ++k) held[k] = ~0u;
    };
    for (int run = 0; run < kExtentRuns; ++run) {
        const size_t at = (wave * kExtentRuns + run) * 64 + lane;
        int lo = -1;
        bool active = false;
        uint32_t v[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
        if (at < (size_t)T) {
            const int2 s = seg[at];
            const uint32_t i = (uint32_t)order[at];
            lo = (uint32_t)s.x < (uint32_t)T ? s.x : -1;
            active = lo >= 0 && i < (uint32_t)T && ptorder::lowerCount(s.y - s.x) > 0;
            if (active)
                for (int a = 0; a < 3; ++a) {
                    const uint32_t c = codes[(size_t)a * T + i];
                    v[a] = c;
                    v[3 + a] = ~c;
                }
        }
        const int lo0 = __shfl(lo, 0, 64);
        const bool oneSegment = lo0 >= 0 && __all(lo == lo0);
        if (!(oneSegment && lo0 == heldLo)) flush();
        if (oneSegment) {
            heldLo = lo0;
            heldAny = heldAny || __any(active);
            for (int k = 0; k < 6; ++k) held[k] = v[k] < held[k] ? v[k] : held[k];
        } else if (__any(active)) {
            exchange(v, 1, 8);
            const bool groupActive = __shfl(active ? 1 : 0, lane & ~15, 64) != 0;   // (a group is one segment: all of it active or none)
            if ((lane & 15) == 0 && lo >= 0 && groupActive)
                for (int k = 0; k < 6; ++k) atomicMin(extent + 6 * (size_t)((uint32_t)lo >> ptorder::kSegShift) + k, v[k]);
        }
    }
    flush();
}

// One thread per position p: the key of its member, stored by the member's ORIGINAL index (the sort starts from the identity
// order), and the child segment the position belongs to after this level's sort.
__global__ __launch_bounds__(kResortBlock) void resortKeyKernel(int T, const uint32_t* __restrict__ codes, const int* __restrict__ order,
                                                                int2* __restrict__ seg, const uint32_t* __restrict__ extent,
                                                                unsigned long long* __restrict__ keys) {
    const int p = blockIdx.x * kResortBlock + threadIdx.x;
    if (p >= T) return;
    int2 s = seg[p];
    const uint32_t i = (uint32_t)order[p];
    if (i >= (uint32_t)T || (uint32_t)s.x >= (uint32_t)T) return;
    const int left = ptorder::lowerCount(s.y - s.x);
    uint32_t code = 0u;
    if (left > 0) {
        const uint32_t* e = extent + 6 * (size_t)((uint32_t)s.x >> ptorder::kSegShift);
        const uint32_t mn[3] = {e[0], e[1], e[2]}, mx[3] = {~e[3], ~e[4], ~e[5]};
        code = codes[(size_t)ptorder::splitAxis(mn, mx) * T + i];
    }
    keys[i] = ptorder::sortKey(s.x, code);
    if (left > 0) {
        ptorder::childSegment(p, left, s.x, s.y);
        seg[p] = s;
    }
}

// One thread per NEW position p: the eight rows of its member, fetched from the member's old position, and the member's new position.
__global__ __launch_bounds__(kResortBlock) void resortGatherKernel(const float4* __restrict__ blob, int T, int offTri, int offTriNormal, int offTriVert,
                                                                   int offTriPos, const int* __restrict__ order, float4* __restrict__ rows,
                                                                   int* __restrict__ newPos) {
    const int p = blockIdx.x * kResortBlock + threadIdx.x;
    if (p >= T) return;
    const uint32_t i = (uint32_t)order[p];
    uint32_t old = (uint32_t)p;   // (a member that cannot be found stays where it is)
    if (i < (uint32_t)T) {
        old = reinterpret_cast<const uint32_t*>(blob + offTriPos)[i];
        newPos[i] = p;
    }
    if (old >= (uint32_t)T) old = (uint32_t)p;
    float4* dst = rows + (size_t)kRowsPerTri * p;
    for (int k = 0; k < 3; ++k) dst[k] = blob[offTri + 3 * (size_t)old + k];
    for (int k = 0; k < 3; ++k) dst[3 + k] = blob[offTriNormal + 3 * (size_t)old + k];
    for (int k = 0; k < 2; ++k) dst[6 + k] = blob[offTriVert + 2 * (size_t)old + k];
}

// One thread per area light: its two triangles are named by stored position (packMaterialsAndLights). The original index behind an
// old position is in the key word of the OLD row there (0xFFFFFFFE - original index); its new position is newPos'.
__global__ __launch_bounds__(64) void resortLightsKernel(float4* __restrict__ blob, int T, int offTri, int offAreaLight, int numAreaLights,
                                                         const int* __restrict__ newPos) {
    const int l = blockIdx.x * 64 + threadIdx.x;
    if (l >= numAreaLights) return;
    float4* row = blob + offAreaLight + 2 * (size_t)l;
    auto renamed = [&](float word) {
        const uint32_t old = __builtin_bit_cast(uint32_t, word);
        if (old >= (uint32_t)T) return word;
        const uint32_t orig = 0xfffffffeu - __builtin_bit_cast(uint32_t, blob[offTri + 3 * (size_t)old + 1].w);
        if (orig >= (uint32_t)T) return word;
        const uint32_t now = (uint32_t)newPos[orig];
        return now < (uint32_t)T ? __builtin_bit_cast(float, now) : word;
    };
    const float a = renamed(row[0].w), b = renamed(row[1].x);
    row[0].w = a;
    row[1].x = b;
}

// One thread per new position: its rows back into the image; one thread per original index: its stored position.
__global__ __launch_bounds__(kResortBlock) void resortScatterKernel(float4* __restrict__ blob, int T, int offTri, int offTriNormal, int offTriVert,
                                                                    int offTriPos, const float4* __restrict__ rows, const int* __restrict__ newPos) {
    const int p = blockIdx.x * kResortBlock + threadIdx.x;
    if (p >= T) return;
    const float4* src = rows + (size_t)kRowsPerTri * p;
    for (int k = 0; k < 3; ++k) blob[offTri + 3 * (size_t)p + k] = src[k];
    for (int k = 0; k < 3; ++k) blob[offTriNormal + 3 * (size_t)p + k] = src[3 + k];
    for (int k = 0; k < 2; ++k) blob[offTriVert + 2 * (size_t)p + k] = src[6 + k];
    reinterpret_cast<int*>(blob + offTriPos)[p] = newPos[p];
}

// ---- scratch ---------------------------------------------------------------------------------------------------------------------
// Per triangle: codes 12 B, iota 4, order 4, segment 8, keys 8 + 8, new position 4, rows 128, extents 24 per leaf = 1.5:
// 177.5 B, plus the sort's temporary (what rocPRIM asks for at this size and key width).
namespace {
using Key = unsigned long long;
hipError_t sortTemporaryBytes(int T, size_t* bytes) {
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, static_cast<Key*>(nullptr), static_cast<Key*>(nullptr), static_cast<int*>(nullptr),
                                     static_cast<int*>(nullptr), (size_t)T, 0u, (unsigned)ptorder::kKeyBits, hipStream_t(nullptr));
}
size_t alignUp(size_t b) { return (b + 255) / 256 * 256; }
}  // namespace

void releaseResortScratch(ResortScratch& s) {
    (void)hipFree(s.base);
    s = ResortScratch{};
}

hipError_t reserveResortScratch(ResortScratch& s, int T) {
    if (s.base && s.capacity == T) return hipSuccess;   // (the sort's temporary is laid out for exactly this size)
    size_t temp = 0;
    if (hipError_t e = sortTemporaryBytes(T, &temp)) return e;
    const size_t n = (size_t)T, leaves = (n + ptorder::kLeaf - 1) / ptorder::kLeaf;
    const size_t sizes[9] = {kRowsPerTri * sizeof(float4) * n, sizeof(Key) * n, sizeof(Key) * n, sizeof(int2) * n, 3 * sizeof(uint32_t) * n,
                             sizeof(int) * n, sizeof(int) * n, sizeof(int) * n, 6 * sizeof(uint32_t) * leaves};
    size_t total = alignUp(temp);
    for (size_t b : sizes) total += alignUp(b);
    char* base = nullptr;
    if (hipError_t e = hipMalloc(&base, total)) return e;
    if (s.base) (void)hipFree(s.base);   // (synchronises with whatever still reads the smaller scratch)
    char* at = base;
    auto take = [&](size_t b) { char* p = at; at += alignUp(b); return p; };
    s = ResortScratch{};
    s.base = base;
    s.rows = reinterpret_cast<float4*>(take(sizes[0]));
    s.keysIn = reinterpret_cast<Key*>(take(sizes[1]));
    s.keysOut = reinterpret_cast<Key*>(take(sizes[2]));
    s.seg = reinterpret_cast<int2*>(take(sizes[3]));
    s.codes = reinterpret_cast<uint32_t*>(take(sizes[4]));
    s.iota = reinterpret_cast<int*>(take(sizes[5]));
    s.order = reinterpret_cast<int*>(take(sizes[6]));
    s.newPos = reinterpret_cast<int*>(take(sizes[7]));
    s.extent = reinterpret_cast<uint32_t*>(take(sizes[8]));
    s.extentBytes = sizes[8];
    s.temp = take(temp);
    s.tempBytes = temp;
    s.capacity = T;
    return hipSuccess;
}

hipError_t launchResort(hipStream_t st, float4* blob, const SceneLayout& L, const ResortScratch& s) {
    const int T = L.numTriangles;
    if (T <= 0 || T != s.capacity) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((T + kResortBlock - 1) / kResortBlock)), block(kResortBlock);
    hipLaunchKernelGGL(resortInitKernel, grid, block, 0, st, blob, T, L.offTri, L.offTriVert, L.offTriPos, s.codes, s.iota, s.order, s.seg,
                       s.newPos);
    const int levels = ptorder::levelsOf(T);
    for (int level = 0; level <= levels; ++level) {   // the last level only puts the leaves into index order
        if (level < levels) {
            if (hipError_t e = hipMemsetAsync(s.extent, 0xff, s.extentBytes, st)) return e;
            const int perBlock = kResortBlock * kExtentRuns;
            hipLaunchKernelGGL(resortExtentKernel, dim3((unsigned)((T + perBlock - 1) / perBlock)), block, 0, st, T, s.codes, s.order, s.seg, s.extent);
        }
        hipLaunchKernelGGL(resortKeyKernel, grid, block, 0, st, T, s.codes, s.order, s.seg, s.extent, s.keysIn);
        size_t tempBytes = s.tempBytes;
        // the last level's keys are segment numbers alone
        if (hipError_t e = rocprim::radix_sort_pairs(s.temp, tempBytes, s.keysIn, s.keysOut, s.iota, s.order, (size_t)T,
                                                     level < levels ? 0u : 32u, (unsigned)ptorder::kKeyBits, st))
            return e;
    }
    hipLaunchKernelGGL(resortGatherKernel, grid, block, 0, st, blob, T, L.offTri, L.offTriNormal, L.offTriVert, L.offTriPos, s.order, s.rows, s.newPos);
    if (L.numAreaLights > 0)
        hipLaunchKernelGGL(resortLightsKernel, dim3((unsigned)((L.numAreaLights + 63) / 64)), dim3(64), 0, st, blob, T, L.offTri, L.offAreaLight,
                           L.numAreaLights, s.newPos);
    hipLaunchKernelGGL(resortScatterKernel, grid, block, 0, st, blob, T, L.offTri, L.offTriNormal, L.offTriVert, L.offTriPos, s.rows, s.newPos);
    return hipGetLastError();
}

}  // namespace ptss
