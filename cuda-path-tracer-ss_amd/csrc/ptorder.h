// ptorder.h — the kd order of a mesh image's triangles, restated LEVEL BY LEVEL so that a device can produce it
// (ptss_resort_triangles, ptss_resort.hip). Written once for the gfx950 kernels and for the host
// (host_capi.cpp ptss_probe_kd_order), both built with -ffp-contract=off. The yardstick is the packer: ptpack.h kdOrder on the
// centroids orderTriangles computes, with (leaf, coarse) = (16, 256). This header yields the same LEAVES — every 16 consecutive
// positions hold the same set of original indices — which is all the image depends on (the closest hit is keyed by original index).
//
// Why the leaves agree. kdOrder splits a segment [lo, hi) of n positions at `left`, a function of n alone, along the axis of
// largest float extent of the members' centroids (strict >, from x: ties go to the lower axis), and std::nth_element puts the
// `left` members smallest by (centroid[axis], original index) into the lower part: WHICH members those are is fixed by the
// comparator, whatever order nth_element leaves them in. Minima and maxima do not depend on the members' order either. So the
// member SET of every segment of every level is determined, by induction from the root; the rule below names the same sets. The
// order inside a finished segment is left open by the packer; here it is ascending original index.
//
// The comparator is `ka < kb || (ka == kb && a < b)` on floats: -0.0 and +0.0 tie, and the original index decides. orderCode maps
// a float to an unsigned integer with the same order and gives both zeros ONE code; with distinct codes a grid through the origin
// would sort differently from the packer (tests/test_resort_cpu.py shows such a grid). Every stored coordinate is finite and
// within 2^40 (meshEligible, sceneUpdateKernel), so no centroid is a NaN.
#pragma once
#include <stdint.h>

#include "ptmath.h"

#if !defined(__HIPCC__)
#include <algorithm>
#include <utility>
#include <vector>
#endif

namespace ptorder {

constexpr int kLeaf = 16;      // ptss::kMeshLeaf
constexpr int kCoarse = 256;   // kMeshLeaf^2: a group
constexpr int kSegShift = 4;   // every segment begins at a multiple of kLeaf: lo >> kSegShift names it in 16 bits (T <= 2^20)
constexpr int kKeyBits = 48;   // (lo >> 4) << 32 | code

// orderTriangles' centroid of one axis: summed left to right in double, divided, rounded once
PTM_HD float centroid(float v0, float v1, float v2) { return (float)(((double)v0 + v1 + v2) / 3); }

// Order-preserving code of a finite float (a < b  <=>  code(a) < code(b), a == b  <=>  code(a) == code(b)). canonicalZero = false
// keeps -0.0 below +0.0: NOT the packer's order — it exists so that a test can show that the canonical form matters.
PTM_HD uint32_t orderCode(float f, bool canonicalZero = true) {
    uint32_t u = __builtin_bit_cast(uint32_t, f);
    if (canonicalZero && (u << 1) == 0u) u = 0u;
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
PTM_HD float orderDecode(uint32_t c) { return __builtin_bit_cast(float, (c >> 31) ? (c ^ 0x80000000u) : ~c); }

// Members of the lower child of a segment of n positions; 0: the segment is finished (a leaf, or nothing to split off).
PTM_HD int lowerCount(int n) {
    if (n <= kLeaf) return 0;
    const int unit = n > kCoarse ? kCoarse : kLeaf;
    int left = ((n / 2 + unit - 1) / unit) * unit;
    if (left >= n) left -= unit;
    return left <= 0 ? 0 : left;
}
// The split axis from the codes of the members' minima and maxima: largest float extent, strict >, starting at x.
PTM_HD int splitAxis(const uint32_t mn[3], const uint32_t mx[3]) {
    int axis = 0;
    float best = orderDecode(mx[0]) - orderDecode(mn[0]);
    for (int a = 1; a < 3; ++a) {
        const float e = orderDecode(mx[a]) - orderDecode(mn[a]);
        if (e > best) { best = e; axis = a; }
    }
    return axis;
}
// The sort key of a member of segment lo: members of a finished segment carry code 0 and so keep their segment, in index order.
PTM_HD uint64_t sortKey(int lo, uint32_t code) { return ((uint64_t)(uint32_t)(lo >> kSegShift) << 32) | code; }
// The child segment of the member that the level's sort put at position p of [lo, hi); left = lowerCount(hi - lo) > 0.
PTM_HD void childSegment(int p, int left, int& lo, int& hi) {
    if (p - lo < left) hi = lo + left;
    else lo += left;
}
// Levels until every segment of T positions is finished (a function of T alone, as every segment boundary is).
// Host only: both children are walked (at most T / 8 segments).
inline int levelsOf(int n) {
    const int left = lowerCount(n);
    if (left <= 0) return 0;
    const int a = levelsOf(left), b = levelsOf(n - left);
    return 1 + (a > b ? a : b);
}

#if !defined(__HIPCC__)
// The rule on the host, level by level, with the sort the kernels run: every level sorts (key, original index) pairs of ALL
// members from the identity order. tri9v: n triangles as {v0, v1, v2}, nine floats each (the caller's exact vertices).
// position[original index] = stored position.
inline void kdPositions(const float* tri9v, int n, int* position, bool canonicalZero = true) {
    std::vector<uint32_t> code((size_t)n * 3);
    for (int i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a)
            code[(size_t)i * 3 + a] = orderCode(centroid(tri9v[9 * (size_t)i + a], tri9v[9 * (size_t)i + 3 + a], tri9v[9 * (size_t)i + 6 + a]), canonicalZero);
    std::vector<int> order((size_t)n), segLo((size_t)n, 0), segHi((size_t)n, n);   // order[p] = member at position p; its segment
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::vector<std::pair<uint64_t, int>> keyed((size_t)n);
    const int levels = levelsOf(n);
    for (int level = 0; level <= levels; ++level) {   // the last level only puts the leaves into index order
        for (int p = 0; p < n;) {
            const int lo = segLo[(size_t)p], hi = segHi[(size_t)p], left = lowerCount(hi - lo);
            int axis = 0;
            if (left > 0) {
                uint32_t mn[3] = {~0u, ~0u, ~0u}, mx[3] = {0u, 0u, 0u};
                for (int q = lo; q < hi; ++q)
                    for (int a = 0; a < 3; ++a) {
                        const uint32_t c = code[(size_t)order[(size_t)q] * 3 + a];
                        mn[a] = c < mn[a] ? c : mn[a];
                        mx[a] = c > mx[a] ? c : mx[a];
                    }
                axis = splitAxis(mn, mx);
            }
            for (int q = lo; q < hi; ++q) {
                const int i = order[(size_t)q];
                keyed[(size_t)i] = {sortKey(lo, left > 0 ? code[(size_t)i * 3 + axis] : 0u), i};
                if (left > 0) childSegment(q, left, segLo[(size_t)q], segHi[(size_t)q]);
            }
            p = hi;
        }
        std::sort(keyed.begin(), keyed.end());   // (key, index): what a stable sort from the identity order gives
        for (int p = 0; p < n; ++p) order[(size_t)p] = keyed[(size_t)p].second;
    }
    for (int p = 0; p < n; ++p) position[(size_t)order[(size_t)p]] = p;
}
#endif

}  // namespace ptorder
