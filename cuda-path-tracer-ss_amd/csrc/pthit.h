// pthit.h — layer 3 of the device code of ptss_kernels.hip: the drivers that answer a whole query. closestHit is intersectScene
// (CudaTracer.cu:121-141) for a path's ray; anyHit, anyHitSplit and pairAnyHit are lineOfSight's loops (CudaTracer.cu:437-452) for
// shadow segments — one per lane, split over lanes, or two per surface point; closestQuery is intersectScene in the caller's order
// for ptss_intersect and ptss_render_features; anyQuery is lineOfSight's loop on whichever image, for ptss_occluded and the shadow
// segments of ptss_trace_paths.
#pragma once
#include "ptaccel.h"

namespace ptss {
namespace {

// ---- closest hit over spheres then triangles, CudaTracer.cu:121-141 ---------------------------
// Spheres, 32 at a time: a uniform pass records in a per-lane bit mask which spheres survive the
// discriminant test; then every lane resolves ITS OWN candidates in index order. A sphere that
// fails the discriminant test never changes `distance`, so visiting only the candidates, in the
// same order, accepts exactly what the reference's full loop accepts — but the square-root path
// runs a few times per lane instead of once per sphere for the whole wave.
// kPrimary on a plain bounded image (kStrips): `strip` is the word of the wave's 64 pixels (ptstrip.h) — bits 0-31 the stored spheres,
// bits 32-63 the stored triangles its eye rays can reach at all; wave-uniform, all ones where the caller has no words. A clear bit
// says that the reference's test rejects that primitive for every ray of the strip, and a rejected primitive
// changes nothing: the sphere trips and triangle bodies of clear bits are skipped on scalar tests, the accepted hits are the same.
template <bool kPrimary, bool kAccel, bool kBounded, bool kMesh = false>
__device__ __forceinline__ Hit closestHit(const float4* sc, const float4* cold, const SceneLayout& L, vec3 o, vec3 d, bool live, uint32_t* ws,
                                          unsigned long long strip = ~0ull) {
    constexpr bool kStrips = kPrimary && !kAccel && kBounded && !kMesh;
    const uint32_t stripSpheres = kStrips ? (uint32_t)strip : ~0u, stripTriangles = kStrips ? (uint32_t)(strip >> 32) : ~0u;
    Hit h;
    h.distance = ptm::inf();
    h.kind = 0;
    h.idx = 0;
    h.w0 = h.w1 = h.w2 = 0;
    if constexpr (kAccel) closestSpheresRegrouped<kPrimary>(sc, cold, L, o, d, live, h, ws);
    for (int base = 0; base < (kAccel ? 0 : L.numSpheres); base += 32) {
        const int cnt = (L.numSpheres - base < 32) ? (L.numSpheres - base) : 32;
        uint32_t mask = sphereCandidates<kPrimary, kBounded, kStrips>(sc, (kPrimary ? L.offPrimSphere : L.offSphere) + base, cnt, o, d, stripSpheres);
        mask &= live ? (lowBits(cnt) & stripSpheres) : 0u;   // (more than 32 spheres: no words, all ones for every block)
        PTSS_DIAG_CANDIDATES(mask, live, 0);
        while (mask != 0) {
            const int j = __builtin_ctz(mask);
            mask &= mask - 1;
            float t;
            const bool acc = kPrimary ? sphereTestPrimary(sc[L.offPrimSphere + base + j], d, h.distance, t)
                                      : sphereTest(sc[L.offSphere + base + j], o, d, h.distance, t);
            if (acc) {
                h.distance = t;
                h.kind = 1;
                h.idx = base + j;
            }
        }
    }
    const unsigned long long liveMask = maskOf(live);
    if constexpr (kMesh) {
        if (meshQueryOk(o, d, live)) {
            // (the general body throughout: its weights are the reference's, so no zero-weight re-evaluation is needed)
            TriBest best{h.distance, kNoTriangle, 0.0f, 0.0f};
            closestTrianglesMesh<kPrimary>(sc, cold, L, o, d, live, best);
            if (best.key != kNoTriangle) {
                h.distance = best.dist;
                h.kind = 2;
                h.idx = reinterpret_cast<const int*>(cold + L.offTriPos)[0xfffffffeu - best.key];   // per-lane gather
                h.w1 = best.w1;
                h.w2 = best.w2;
                h.w0 = 1.0f - (best.w1 + best.w2);  // Primitives.h:64, from the kept pair
            }
            return h;
        }
    } else if (L.triClassed) {
        // The triangles are stored grouped by edge class. One test per query (not per triangle) admits the class bodies:
        // |d|^2 < 2^30 bounds |det| below the reciprocal's fast range, and with a finite origin every product the class
        // forms leave out is an exact zero (pttri.h). A wave that fails it (a NaN or enormous ray) walks the triangles in the
        // CALLER's order with the guarded general test below: the reference's sequential rule, NaNs included.
        if (classedQueryOk(o, d)) {
            TriBest best{h.distance, kNoTriangle, 0.0f, 0.0f};
            // one vector byte address for the triangle rows (the head and the weights block of a body read through the same
            // register) and, at bounce 0, one for the camera-origin rows: ptwave.h vectorRow
            uint32_t triAt = vectorRow(sc, L.offTri), primAt = vectorRow(sc, L.offPrimTri);
#define PTSS_CLOSEST_BODY(c1, c2, t)                                                                   \
    if (!kStrips || ((stripTriangles >> ((uint32_t)(t) & 31u)) & 1u) != 0u) /* t < 32 wherever a bit is clear */ \
        triangleClassed<kPrimary, c1, c2, true>(rowAt(sc, triAt), rowAt(sc, primAt), 0u, o, d, liveMask, best);
            PTSS_FOR_TRIANGLES_BY_CLASS(L, PTSS_CLOSEST_BODY, (triAt += 3 * kRowBytes, primAt += 2 * kRowBytes));
#undef PTSS_CLOSEST_BODY
            if (waveAny(best.key != kNoTriangle)) {
                const int* posOf = reinterpret_cast<const int*>(sc + L.offTriPos);
                int pos = 0;
                if (best.key != kNoTriangle) pos = posOf[0xfffffffeu - best.key];   // per-lane gather
                // A kept weight that is exactly zero (the hit lies on an edge of the triangle) may carry the other sign in a
                // class form (pttri.h): those lanes — hardly ever one — take the general form's weights, so that even the sign
                // of a zero normal component is the reference's. The general form accepts the same hit at the same distance.
                const bool zeroWeight = best.key != kNoTriangle && (best.w1 == 0.0f || best.w2 == 0.0f);
                if (waveAny(zeroWeight)) {
                    if (zeroWeight) {
                        const float4* rows = sc + L.offTri + 3 * pos;   // per-lane gathers
                        const float4* prim = sc + L.offPrimTri + 2 * pos;
                        const pttri::Head g = pttri::head<0, 0, kPrimary>(xyz(rows[0]), xyz(rows[1]), xyz(rows[2]), xyz(prim[0]), xyz(prim[1]), prim[0].w, o, d);
                        float b0;
                        pttri::weights<0, 0>(g, d, b0, best.w1, best.w2);
                    }
                }
                if (best.key != kNoTriangle) {
                    h.distance = best.dist;
                    h.kind = 2;
                    h.idx = pos;
                    h.w1 = best.w1;
                    h.w2 = best.w2;
                    h.w0 = 1.0f - (best.w1 + best.w2);  // Primitives.h:64, from the kept pair
                }
            }
            return h;
        }
    } else if (L.triDetBounded && waveAll(dot(d, d) < 0x1p30f)) {
        // the caller's order, the general body, the sequential rule; the reciprocal's range guard proven once per query
        TriBest best{h.distance, kNoTriangle, 0.0f, 0.0f};
        uint32_t triAt = vectorRow(sc, L.offTri), primAt = vectorRow(sc, L.offPrimTri);   // as above
        for (int i = 0; i < L.numTriangles; ++i, triAt += 3 * kRowBytes, primAt += 2 * kRowBytes)
            triangleClassed<kPrimary, 0, 0, false>(rowAt(sc, triAt), rowAt(sc, primAt), (uint32_t)i, o, d, liveMask, best);
        if (best.key != kNoTriangle) {
            h.distance = best.dist;
            h.kind = 2;
            h.idx = (int)best.key;
            h.w1 = best.w1;
            h.w2 = best.w2;
            h.w0 = 1.0f - (best.w1 + best.w2);  // Primitives.h:64, from the kept pair
        }
        return h;
    }
    const float4* td = kMesh ? cold : sc;   // the triangle tables (global memory in the mesh image)
    const int* posOfOriginal = reinterpret_cast<const int*>(td + L.offTriPos);
    for (int k = 0; k < L.numTriangles; ++k) {   // the guarded loop, in the caller's order: unbounded edges, or a ray of enormous length
        const int i = (kMesh || L.triClassed) ? posOfOriginal[k] : k;   // where original triangle k is stored
        const TriRows tcur = kPrimary ? loadTriEdges(td + L.offTri + 3 * i) : loadTri(td + L.offTri + 3 * i);
        const TriHit th = kPrimary ? triangleTestPrimary(tcur, td[L.offPrimTri + 2 * i], loadRow16(td + L.offPrimTri + 2 * i + 1), d,
                                                         h.distance, liveMask)
                                   : triangleTest(tcur, o, d, h.distance, liveMask);
        if (th.hit) {
            h.distance = th.dist;
            h.kind = 2;
            h.idx = i;
            h.w0 = th.w0;
            h.w1 = th.w1;
            h.w2 = th.w2;
        }
    }
    return h;
}

// the triangle half of lineOfSight for a wave whose lanes all test the same triangle at a time: `need` = lanes that still want an
// answer, `blocked` collects the verdicts. Grouped storage (SceneLayout::triClassed): one loop per edge class with its shorter
// body, the reciprocal's guard proven once per pass; otherwise, and for non-finite or enormous segments, the guarded general test.
__device__ __forceinline__ void anyTriangleLoop(const float4* sc, const SceneLayout& L, vec3 lo, vec3 w_i, float distance, unsigned long long& need,
                                                unsigned long long& blocked) {
    if (L.triClassed && classedQueryOk(lo, w_i)) {
        uint32_t triAt = vectorRow(sc, L.offTri);   // one vector byte address through all the class loops (ptwave.h)
#define PTSS_ANY_BODY(c1, c2, t)   \
    if (need == 0ull) break;      \
    triangleClassedAny<c1, c2>(rowAt(sc, triAt), lo, w_i, distance, need, blocked);
        PTSS_FOR_TRIANGLES_BY_CLASS(L, PTSS_ANY_BODY, triAt += 3 * kRowBytes);
#undef PTSS_ANY_BODY
        return;
    }
    for (int i = 0; i < L.numTriangles; ++i) {
        if (need == 0ull) break;
        const TriRows tcur = loadTri(sc + L.offTri + 3 * i);
        const TriHit th = triangleTest(tcur, lo, w_i, distance, need);
        blocked |= th.hitMask;
        need &= ~th.hitMask;
    }
}

// the triangle half of lineOfSight alone (the sphere half having been answered by anySpheresHybrid)
__device__ __forceinline__ bool anyTriangles(const float4* sc, const SceneLayout& L, vec3 lo, vec3 w_i, float distance, bool live) {
    unsigned long long need = maskOf(live), blocked = 0ull;
    anyTriangleLoop(sc, L, lo, w_i, distance, need, blocked);
    return __builtin_amdgcn_inverse_ballot_w64(blocked);
}

// ---- the any-hit loops of lineOfSight, CudaTracer.cu:437-452: true when some primitive blocks the
// segment. Order-independent (the reference returns at the first accepted primitive and no test
// depends on another). `live`: this lane carries a segment. -----------------------------------------
template <bool kAccel, bool kBounded, bool kMesh = false>
__device__ __forceinline__ bool anyHit(const float4* sc, const SceneLayout& L, vec3 lo, vec3 w_i, float distance,
                                       bool live, const float4* cold = nullptr) {
    bool occluded = false;
    if constexpr (kAccel) occluded = anySphereChunked(sc, L, lo, w_i, distance, live);
    for (int base = 0; base < (kAccel ? 0 : L.numSpheres); base += 32) {
        const int cnt = (L.numSpheres - base < 32) ? (L.numSpheres - base) : 32;
        uint32_t mask = sphereCandidatesPairs<kBounded>(sc, L.offSphere + base, cnt, lo, w_i);
        mask &= (live && !occluded) ? lowBits(cnt) : 0u;
        PTSS_DIAG_CANDIDATES(mask, live, 4);
        while (mask != 0) {
            const int j = __builtin_ctz(mask);
            mask &= mask - 1;
            float t;
            if (sphereTest(sc[L.offSphere + base + j], lo, w_i, distance, t)) {
                occluded = true;
                mask = 0;
            }
        }
    }
    if constexpr (kMesh) return anyTrianglesMesh(sc, cold, L, lo, w_i, distance, live && !occluded) || occluded;
    unsigned long long need = maskOf(live) & ~maskOf(occluded);  // lanes that still want an answer
    unsigned long long blocked = 0ull;
    anyTriangleLoop(sc, L, lo, w_i, distance, need, blocked);
    return occluded || __builtin_amdgcn_inverse_ballot_w64(blocked);
}

// ---- the same any-hit with the primitive list SPLIT over g = 1 << shift lanes per segment: lane `sub` of a
// segment's group visits primitives sub, sub + g, sub + 2g, ...; the caller ORs the group's verdicts. Every test is
// the scalar test on the same operands, and lineOfSight's answer is an OR over independent tests, so the verdict is
// the one anyHit gives. Used when a pass over the wave's queue holds fewer than 64 segments: 8 segments x 8 lanes
// cost an eighth of a dense pass instead of a whole one. Rows are gathered per lane here (no broadcast). ------------
template <bool kBounded>
__device__ __forceinline__ bool anyHitSplit(const float4* sc, const SceneLayout& L, vec3 lo, vec3 w_i, float distance,
                                            bool live, int shift, int sub) {
    bool occluded = false;
    const int g = 1 << shift;
    const int sphereSteps = (L.numSpheres + g - 1) >> shift;
    for (int base = 0; base < sphereSteps; base += 32) {
        const int cnt = (sphereSteps - base < 32) ? (sphereSteps - base) : 32;
        uint32_t mask = sphereCandidatesStridedPairs<kBounded>(sc + L.offSphere + (base << shift) + sub, g, cnt, lo, w_i);
        // this lane's spheres are sub, sub + g, ...: step j exists for it iff (j << shift) + sub < numSpheres
        mask &= (live && !occluded) ? lowBitsClamped(((L.numSpheres - sub + g - 1) >> shift) - base) : 0u;
        while (mask != 0) {
            const int j = __builtin_ctz(mask);
            mask &= mask - 1;
            float t;
            if (sphereTest(sc[L.offSphere + ((base + j) << shift) + sub], lo, w_i, distance, t)) {
                occluded = true;
                mask = 0;
            }
        }
    }
    const int triSteps = (L.numTriangles + g - 1) >> shift;
    unsigned long long need = maskOf(live) & ~maskOf(occluded);
    unsigned long long blocked = 0ull;
    for (int k = 0; k < triSteps; ++k) {
        if (need == 0ull) break;
        const int idx = (k << shift) + sub;
        const bool in = idx < L.numTriangles;
        const TriRows tcur = loadTri(sc + L.offTri + 3 * (in ? idx : 0));
        const TriHit th = triangleTest(tcur, lo, w_i, distance, need & maskOf(in));
        blocked |= th.hitMask;
        need &= ~th.hitMask;
    }
    return occluded || __builtin_amdgcn_inverse_ballot_w64(blocked);
}

// ---- lineOfSight for the TWO segments a surface point sends to the two lights of an NEE round. They share their origin,
// and so everything the tests compute from origin and primitive alone: a sphere's v = o - centre and c = |v|^2 - r^2
// (7 of its 13 / 15 instructions), a triangle's s = o - v0, r = s x e1 and e2 . r (12 of the ~32 up to the distance test).
// Each segment's own part is the scalar test's, on the same operands in the same order, so the two verdicts are the ones
// two separate queue entries would get. kSplit: 1 << shift lanes share an entry, lane `sub` takes primitives sub, sub + g, ...
// (anyHitSplit's scheme); otherwise one lane per entry and broadcast rows. liveA / liveB: the segment exists and is needed.
template <bool kBounded, bool kSplit>
__device__ __forceinline__ void pairAnyHit(const float4* sc, const SceneLayout& L, vec3 lo, vec3 wA, float dA, bool liveA, vec3 wB, float dB,
                                           bool liveB, int shift, int sub, bool& occA, bool& occB) {
    occA = false;
    occB = false;
    const int g = kSplit ? (1 << shift) : 1;
    const int sphereSteps = kSplit ? ((L.numSpheres + g - 1) >> shift) : L.numSpheres;
    for (int base = 0; base < sphereSteps; base += 32) {
        const int cnt = (sphereSteps - base < 32) ? (sphereSteps - base) : 32;
        const int trips = (cnt + 1) >> 1;
        uint32_t revA = 0, revB = 0;
        for (int t = 0; t < trips; ++t) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int step = base + 2 * t + u;
                const float4 sp = kSplit ? sc[L.offSphere + ((step << shift) + sub)] : sc[L.offSphere + step];
                const vec3 v = lo - xyz(sp);
                const float c = dot(v, v) - sp.w;
                const float hA = dot(wA, v), hB = dot(wB, v);
                if constexpr (kBounded) {
                    shiftInMayHit(revA, hA * hA, c);
                    shiftInMayHit(revB, hB * hB, c);
                } else {
                    const float c4 = 4 * c, bA = hA * 2, bB = hB * 2;
                    shiftInMayHit(revA, bA * bA, c4);
                    shiftInMayHit(revB, bB * bB, c4);
                }
            }
        }
        const uint32_t valid = kSplit ? lowBitsClamped(((L.numSpheres - sub + g - 1) >> shift) - base) : lowBits(cnt);
        uint32_t maskA = (__builtin_bitreverse32(revA) >> (32 - 2 * trips)) & ((liveA && !occA) ? valid : 0u);
        uint32_t maskB = (__builtin_bitreverse32(revB) >> (32 - 2 * trips)) & ((liveB && !occB) ? valid : 0u);
        while (maskA != 0) {
            const int j = __builtin_ctz(maskA);
            maskA &= maskA - 1;
            float t;
            if (sphereTest(sc[L.offSphere + (kSplit ? (((base + j) << shift) + sub) : (base + j))], lo, wA, dA, t)) {
                occA = true;
                maskA = 0;
            }
        }
        while (maskB != 0) {
            const int j = __builtin_ctz(maskB);
            maskB &= maskB - 1;
            float t;
            if (sphereTest(sc[L.offSphere + (kSplit ? (((base + j) << shift) + sub) : (base + j))], lo, wB, dB, t)) {
                occB = true;
                maskB = 0;
            }
        }
    }
    unsigned long long needA = __ballot(liveA && !occA), needB = __ballot(liveB && !occB);
    unsigned long long blockedA = 0ull, blockedB = 0ull;
    const int triSteps = kSplit ? ((L.numTriangles + g - 1) >> shift) : L.numTriangles;
    if constexpr (!kSplit) {   // every lane at the same triangle: one loop per edge class (grouped storage), origin part shared
        if (L.triClassed && classedQueryOk(lo, wA) && waveAll(dot(wB, wB) < 0x1p30f)) {
            uint32_t triAt = vectorRow(sc, L.offTri);   // one vector byte address through all the class loops (ptwave.h)
#define PTSS_PAIR_BODY(c1, c2, t)            \
    if ((needA | needB) == 0ull) break;     \
    triangleClassedPair<c1, c2>(rowAt(sc, triAt), lo, wA, dA, wB, dB, needA, needB, blockedA, blockedB);
            PTSS_FOR_TRIANGLES_BY_CLASS(L, PTSS_PAIR_BODY, triAt += 3 * kRowBytes);
#undef PTSS_PAIR_BODY
            occA = occA || __builtin_amdgcn_inverse_ballot_w64(blockedA);
            occB = occB || __builtin_amdgcn_inverse_ballot_w64(blockedB);
            return;
        }
    }
    for (int k = 0; k < triSteps; ++k) {
        if ((needA | needB) == 0ull) break;
        const int idx = kSplit ? ((k << shift) + sub) : k;
        const bool in = !kSplit || idx < L.numTriangles;
        const TriRows tr = loadTri(sc + L.offTri + 3 * (in ? idx : 0));
        const unsigned long long inMask = kSplit ? maskOf(in) : ~0ull;
        const vec3 v0 = xyz(tr.a), e1 = xyz(tr.b), e2 = xyz(tr.c);
        const vec3 sv = lo - v0;               // shared by the two segments (Primitives.h:46-49)
        const vec3 r = cross(sv, e1);
        const float e2r = dot(e2, r);
        if (needA != 0ull) {
            const vec3 q = cross(wA, e2);
            const float det = dot(e1, q);
            const float inverseDet = triRcp(det);
            const float dist = e2r * inverseDet;
            const unsigned long long pass = needA & inMask & maskOf(!(ptm::abs(det) <= 1e-7f)) & maskOf(!(dist <= 0.0f)) & maskOf(!(dist > dA));
            if (pass != 0ull) {
                const float b1 = dot(sv, q) * inverseDet;
                const float b2 = dot(wA, r) * inverseDet;
                const float b0 = 1.0f - (b1 + b2);
                const unsigned long long hit = pass & maskOf(!(b0 < 0)) & maskOf(!(b1 < 0)) & maskOf(!(b2 < 0));
                blockedA |= hit;
                needA &= ~hit;
            }
        }
        if (needB != 0ull) {
            const vec3 q = cross(wB, e2);
            const float det = dot(e1, q);
            const float inverseDet = triRcp(det);
            const float dist = e2r * inverseDet;
            const unsigned long long pass = needB & inMask & maskOf(!(ptm::abs(det) <= 1e-7f)) & maskOf(!(dist <= 0.0f)) & maskOf(!(dist > dB));
            if (pass != 0ull) {
                const float b1 = dot(sv, q) * inverseDet;
                const float b2 = dot(wB, r) * inverseDet;
                const float b0 = 1.0f - (b1 + b2);
                const unsigned long long hit = pass & maskOf(!(b0 < 0)) & maskOf(!(b1 < 0)) & maskOf(!(b2 < 0));
                blockedB |= hit;
                needB &= ~hit;
            }
        }
    }
    occA = occA || __builtin_amdgcn_inverse_ballot_w64(blockedA);
    occB = occB || __builtin_amdgcn_inverse_ballot_w64(blockedB);
}

// ---- The closest hit of one ray per lane, shared by queryKernel (ptss_intersect) and featureKernel (ptss_render_features): one
// body, two callers. sc: the scene image as staged (LDS or global), sceneBlob: the same in global memory.
// Closest hit: intersectScene (CudaTracer.cu:120-141) with `distance` starting at the ray's tmax. Spheres in the CALLER's order
// with the reference's own test (a sorted many-sphere image maps caller index k to its stored position, offSpherePos), then
// triangles: on the mesh image, when every live lane of the wave meets the two-level traversal's preconditions (meshQueryOk: a unit
// direction, a bounded origin) and carries a running distance > 0 into it (the keyed minimum of closestTrianglesMesh orders
// (distance, ~index) by bit pattern, which holds for positive distances only — no NaN, no -0, no negative tmax), that traversal;
// otherwise the caller's order with the guarded test (closestHit's last loop). Both end on what the sequential
// `dist <= distance` rule ends on; every NaN, infinite, huge or zero input takes the literal loops, which ARE the reference's.
struct QueryHit {
    vec3 point, normal;
    float dist;
    int materialIdx, kind, prim;
    float w1, w2;
};
__device__ __forceinline__ QueryHit closestQuery(const float4* sc, const float4* __restrict__ sceneBlob, const SceneLayout& L, vec3 o, vec3 d, float tmax,
                                                 bool live) {
    const bool mesh = meshImage(L);
    const float4* td = mesh ? sceneBlob : sc;   // the triangle tables (global memory in the mesh image)
    const int* spherePos = reinterpret_cast<const int*>(sceneBlob + L.offSpherePos);   // (read only with accelSpheres)
    const int* triPos = reinterpret_cast<const int*>(sceneBlob + L.offTriPos);         // (read only for classed and mesh images)
    const bool triStoredElsewhere = mesh || L.triClassed;
    const unsigned long long liveMask = maskOf(live);
    float dist = tmax;
    int kind = 0, prim = -1, pos = 0;
    float w0 = 0, w1 = 0, w2 = 0;
    for (int k = 0; k < L.numSpheres; ++k) {   // the caller's order, the reference's test
        const int p = L.accelSpheres ? spherePos[k] : k;
        float t;
        if (live && sphereTest(sc[L.offSphere + p], o, d, dist, t)) {
            dist = t;
            kind = 1;
            prim = k;
            pos = p;
        }
    }
    if (mesh && meshQueryOk(o, d, live) && waveAll(!live || dist > 0.0f)) {
        TriBest best{dist, kNoTriangle, 0.0f, 0.0f};
        closestTrianglesMesh<false>(sc, sceneBlob, L, o, d, live, best);
        if (best.key != kNoTriangle) {
            dist = best.dist;
            kind = 2;
            prim = (int)(0xfffffffeu - best.key);
            pos = triPos[prim];   // per-lane gather
            w1 = best.w1;
            w2 = best.w2;
            w0 = 1.0f - (w1 + w2);  // Primitives.h:64, from the kept pair
        }
    } else {
        for (int k = 0; k < L.numTriangles; ++k) {   // the guarded loop, in the caller's order
            const int p = triStoredElsewhere ? triPos[k] : k;
            const TriHit th = triangleTest(loadTri(td + L.offTri + 3 * p), o, d, dist, liveMask);
            if (th.hit) {
                dist = th.dist;
                kind = 2;
                prim = k;
                pos = p;
                w0 = th.w0;
                w1 = th.w1;
                w2 = th.w2;
            }
        }
    }
    // the SurfaceElement, with bounceTile's operations after its closest hit (Primitives.h:74, :100)
    vec3 point = v3(0, 0, 0), normal = v3(0, 0, 0);
    int materialIdx = -1;
    if (kind != 0) {
        point = o + d * dist;
        if (kind == 1) {
            normal = normalize(point - xyz(loadRow16(sc + L.offSphere + pos)));
            materialIdx = reinterpret_cast<const int*>(sceneBlob + L.offSphereMat)[pos];
        } else {
            const float4* nn = td + L.offTriNormal + 3 * pos;
            normal = (xyz(loadRow16(nn)) * w0 + xyz(loadRow16(nn + 1)) * w1) + xyz(loadRow16(nn + 2)) * w2;
            materialIdx = (int)asU(td[L.offTri + 3 * pos].w);
        }
    } else {
        w1 = w2 = 0.0f;
    }
    if (kind == 1) w1 = w2 = 0.0f;
    return QueryHit{point, normal, dist, materialIdx, kind, prim, w1, w2};
}

// ---- Is the segment (o, d, tmax) of each live lane blocked, on ANY image and for every input (ptss_occluded; the shadow segments of
// ptss_trace_paths): lineOfSight's loop (CudaTracer.cu:434-452) is an OR over independent tests, so anyHit's order-free loops answer it
// for the images whose sphere tests are the literal ones (plain, mesh); the sorted many-sphere image's chunk tests assume origins in
// the scene's range, so there the same loop walks every STORED sphere row instead of the chunks (the sorted spheres and their padding
// copies: any order and repeats answer an OR) — literal discriminant masks, then the reference's test.
__device__ __forceinline__ bool anyQuery(const float4* sc, const float4* __restrict__ sceneBlob, const SceneLayout& L, bool mesh, vec3 o, vec3 d,
                                         float tmax, bool live) {
    if (L.accelSpheres) {
        SceneLayout Ls = L;
        Ls.numSpheres = L.numChunks * kChunkSpheres;
        return anyHit<false, false, false>(sc, Ls, o, d, tmax, live);
    }
    if (mesh) return anyHit<false, false, true>(sc, L, o, d, tmax, live, sceneBlob);
    return anyHit<false, false, false>(sc, L, o, d, tmax, live);
}

}  // namespace
}  // namespace ptss
