// ptprim.h — layer 1 of the device code of ptss_kernels.hip: the primitive tests. Sphere::intersectRay (Primitives.h:107-175) and
// Triangle::intersectRay (Primitives.h:25-83) in their wave forms — the guarded general tests, the edge-class bodies (pttri.h) with
// their one-loop-per-class macro, the camera-origin (bounce 0) variants, and the sphere candidate masks (CudaTracer.cu:127-133 /
// :438-444 through Primitives.h:107-118).
#pragma once
#include "ptscene.h"
#include "pttri.h"
#include "ptwave.h"

namespace ptss {
namespace {

// ---- Sphere::intersectRay, Primitives.h:107-175. sp = {centre, radius^2}. ---------------------
// The reference's first exit, `discriminent < 0` (Primitives.h:117-118), is what the candidate masks below decide for up to
// 32 spheres at a time (shiftInSphere); sphereTest is the whole test, for the candidates. Both evaluate b, c and the
// discriminant with the same operations.
// Returns the accepted distance in t; `limit` is the running `distance`.
__device__ __forceinline__ bool sphereTest(float4 sp, vec3 o, vec3 d, float limit, float& t) {
    const vec3 v = o - xyz(sp);
    const float b = dot(d, v) * 2;
    const float c = dot(v, v) - sp.w;
    float disc = (b * b) - 4 * c;
    if (disc < 0) return false;
    disc = ptm::sqrt(disc);
    float t0 = (-b + disc) * 0.5f;
    float t1 = (-b - disc) * 0.5f;
    if (t0 < 0 && t1 < 0) return false;
    if (t0 > t1) {
        const float tmp = t0;
        t0 = t1;
        t1 = tmp;
    }
    const float cand = (t0 < 0) ? t1 : t0;
    if (cand > limit) return false;
    t = cand;
    return true;
}

// ---- Triangle::intersectRay, Primitives.h:25-83, with the per-lane exits replaced by ONE
// wave-uniform exit: every lane computes det, 1/det and dist (selects instead of divergent
// branches: no exec-mask bookkeeping, and the straight-line code lets the scheduler overlap the
// long division chain with the cross products); the barycentric part runs only if some lane of
// the wave passed both early tests. `live` marks lanes whose result matters. Same operations on
// the same values as the reference for every lane that the reference would carry that far;
// lanes it would have dropped compute values that are discarded. -----------------------------------
struct TriHit {
    bool hit;
    unsigned long long hitMask;  // the same verdicts as a wave mask
    float dist, w0, w1, w2;
};

struct TriRows {  // one staged triangle: {v0, bits(materialIdx)}, {e1, 0}, {e2, 0}
    float4 a, b, c;
};
// The tests use three of a row's four words, and hipcc narrows each fetch to ds_read_b96 — for these broadcast reads the
// faster form (8.4 against 14 SIMD-cycles per wave-read for ds_read_b128, tools/microbench/loops.hip: the LDS-to-VGPR
// return path moves bytes, and 768 are fewer than 1,024).
__device__ __forceinline__ float4 loadRow16(const float4* p) { return *p; }
__device__ __forceinline__ TriRows loadTri(const float4* tr) { return TriRows{loadRow16(tr), loadRow16(tr + 1), loadRow16(tr + 2)}; }
// the camera-origin test (triangleTestPrimary) never looks at v0
__device__ __forceinline__ TriRows loadTriEdges(const float4* tr) { return TriRows{float4{0, 0, 0, 0}, loadRow16(tr + 1), loadRow16(tr + 2)}; }

__device__ __forceinline__ float triRcp(float det) { return ptm::rcp_if_above_1em7(det); }


__device__ __forceinline__ TriHit triangleTest(const TriRows& tr, vec3 o, vec3 d, float limit, unsigned long long liveMask) {
    const vec3 v0 = xyz(tr.a), e1 = xyz(tr.b), e2 = xyz(tr.c);
    const vec3 q = cross(d, e2);
    const float det = dot(e1, q);
    const float inverseDet = triRcp(det);  // 1 / det, Primitives.h:44; unused when |det| <= 1e-7
    const vec3 s = o - v0;
    const vec3 r = cross(s, e1);
    const float dist = dot(e2, r) * inverseDet;
    // pass = live && !(|det| <= 1e-7) && !(dist <= 0 || dist > limit), Primitives.h:41-42, :51-52
    const unsigned long long passMask = liveMask & maskOf(!(ptm::abs(det) <= 1e-7f)) & maskOf(!(dist <= 0.0f)) & maskOf(!(dist > limit));
    TriHit h;
    h.hit = false;
    h.hitMask = 0ull;
    h.dist = dist;
    h.w0 = h.w1 = h.w2 = 0;
    if (passMask != 0ull) {
        const float b1 = dot(s, q) * inverseDet;
        const float b2 = dot(d, r) * inverseDet;
        const float b0 = 1.0f - (b1 + b2);
        h.hitMask = passMask & maskOf(!(b0 < 0)) & maskOf(!(b1 < 0)) & maskOf(!(b2 < 0));
        h.hit = __builtin_amdgcn_inverse_ballot_w64(h.hitMask);
        h.w0 = b0;
        h.w1 = b1;
        h.w2 = b2;
    }
    return h;
}

// ---- The closest hit's triangle loop, lean form (triangleTest stays for the any-hit loops and as the fallback). Same
// operations on the same values as triangleTest for every lane whose result is used; what changes:
//   * The reciprocal's range guard moves out of the loop: |det| = |e1 . (d x e2)| <= |e1| |e2| |d| (1 + 4 ulp); the host
//     bounds |e1| |e2| <= 2^100 (SceneLayout::triDetBounded) and the caller tests |d|^2 < 2^30 once per query, so
//     |det| < 2^126; below, results with |det| <= 1e-7 are discarded (Primitives.h:41) — exactly the operand range on which
//     ptm::rcp's fast path is proven equal to 1.0f / x. Queries that fail the test take the guarded loop.
//   * `b0 < 0 || b1 < 0 || b2 < 0` is decided as min3(b0, b1, b2) < 0: v_min3_f32 passes over NaN operands (a NaN weight
//     fails `< 0` in the reference too) and returns NaN only when all three are NaN (again no rejection); -0 is not < 0
//     either way.
//   * Only (distance, index, w1, w2) of the best hit travel through the loop, merged with selects (no exec-masked accept
//     block); w0 = 1 - (w1 + w2) is recomputed from the kept pair by the caller — the same operation on the same values.
//   * triangleTest's ONE wave-uniform exit (after the distance test) stays: tiles of the early bounces are coherent —
//     neighbouring pixels — and then whole waves do reject a triangle early. (No exit at all is the faster loop on
//     incoherent rays, tools/microbench/loops.hip: 157 -> 138 SIMD-cycles per triangle per wave, and the slower kernel:
//     same-box A/B -1.6 %.)
//   * EDGE CLASSES (kC1, kC2; pttri.h). A triangle whose edges run along coordinate axes (every wall and light panel of the
//     presets but two) loses the products with the exact zeros: 13 instead of 25 operations up to the distance test with two
//     such edges, 19 with one. Every lane of the wave tests the SAME triangle, so the body could be chosen per triangle
//     without divergence — but a scalar branch tree per triangle (35 scalar instructions, 9 branches) cost more than the
//     shorter bodies saved (same-box A/B -2.5 %: scalar instructions are not free beside vector ones,
//     tools/microbench/vgpr_banks.hip). So the host stores the triangles GROUPED BY CLASS (SceneLayout::triClassed /
//     triClassPack) and the loop becomes one loop per class: no dispatch at all. The visiting order is then no longer the
//     caller's, which matters where the reference's sequential rule `dist <= distance` (Primitives.h:52) decides between two
//     triangles hit at exactly the same distance: it ends on the HIGHEST index among them. kKeyed keeps (distance,
//     0xFFFFFFFE - original index) as one 64-bit key — distances that pass `dist > 0` order like their bit patterns — and
//     accepts a hit iff its key is SMALLER than the kept one: minimum distance, then highest original index; the initial key
//     (sphere distance, 0xFFFFFFFF) lets a triangle at exactly the sphere's distance win, as `<=` does. One v_cmp_lt_u64 in
//     place of one v_cmp_ngt_f32: the same issue cost. Exactness of the class forms, preconditions and the one case the
//     caller re-evaluates (a kept weight of exactly zero): pttri.h.
struct TriBest {
    float dist;    // the running `distance` (Primitives.h:52), shared with the sphere phase
    uint32_t key;  // 0xFFFFFFFF: no triangle accepted; kKeyed: 0xFFFFFFFE - original index; else the triangle's index
    float w1, w2;
};
constexpr uint32_t kNoTriangle = 0xffffffffu;
template <bool kPrimary, int kC1, int kC2, bool kKeyed>
__device__ __forceinline__ void triangleClassed(const float4* rows /* {v0, mat}, {e1, key}, {e2} */, const float4* prim /* {s, e2 . r}, {r} */,
                                                uint32_t index, vec3 o, vec3 d, unsigned long long liveMask, TriBest& best) {
    vec3 v0 = v3(0, 0, 0), ps = v3(0, 0, 0), pr = v3(0, 0, 0);
    float pe2r = 0;
    if constexpr (kPrimary) {   // the camera-origin test never looks at v0
        const float4 a = prim[0];
        ps = xyz(a);
        pe2r = a.w;
        pr = xyz(loadRow16(prim + 1));
    } else {
        v0 = xyz(loadRow16(rows));
    }
    const float4 rowE1 = rows[1];
    const pttri::Head h = pttri::head<kC1, kC2, kPrimary>(v0, xyz(rowE1), xyz(loadRow16(rows + 2)), ps, pr, pe2r, o, d);
    const uint32_t key = kKeyed ? asU(rowE1.w) : index;
    unsigned long long passMask = liveMask & maskOf(!(ptm::abs(h.det) <= 1e-7f)) & maskOf(!(h.dist <= 0.0f));
    if constexpr (kKeyed) {
        const unsigned long long mine = ((unsigned long long)asU(h.dist) << 32) | key, kept = ((unsigned long long)asU(best.dist) << 32) | best.key;
        passMask &= maskOf(mine < kept);
    } else {
        passMask &= maskOf(!(h.dist > best.dist));
    }
    if (passMask != 0ull) {
        float b0, b1, b2;
        pttri::weights<kC1, kC2>(h, d, b0, b1, b2);
        const unsigned long long hitMask = passMask & maskOf(!(__builtin_fminf(__builtin_fminf(b0, b1), b2) < 0));
        const bool hit = __builtin_amdgcn_inverse_ballot_w64(hitMask);
        best.dist = hit ? h.dist : best.dist;
        best.key = hit ? key : best.key;
        best.w1 = hit ? b1 : best.w1;
        best.w2 = hit ? b2 : best.w2;
    }
}
// One loop per edge class over the triangles stored for it; BODY(c1, c2, t) tests stored triangle t. The 17 class bounds travel
// as bytes in five scalar registers (SceneLayout::triClassPack) and every loop header extracts its two with s_bfe: as seventeen
// kernel-argument words the compiler evaluated all thirteen "is this class empty" conditions once per kernel, kept them as lane
// masks, spilled those to VGPR lanes and read them back with two v_readlane per loop header — 26 per query. The empty asm
// statements make the packed words opaque at each header, so that nothing about them is hoisted or kept.
struct ClassBounds {
    uint32_t w[5];
};
__device__ __forceinline__ ClassBounds classBounds(const SceneLayout& L) {
    return ClassBounds{{L.triClassPack[0], L.triClassPack[1], L.triClassPack[2], L.triClassPack[3], L.triClassPack[4]}};
}
template <int kCode>
__device__ __forceinline__ int classBegin(ClassBounds& b) {
    asm volatile("" : "+s"(b.w[kCode / 4]));
    return (int)((b.w[kCode / 4] >> (8 * (kCode % 4))) & 255u);
}
// The thirteen loops visit the stored positions 0 .. T - 1 in order, each once (begin(0) = 0, begin(16) = T, the codes 5, 10 and 15
// are empty: pttri.h triangleClass), so ONE running row address serves them all: STEP is evaluated after each triangle and advances
// the caller's vector byte addresses (ptwave.h vectorRow) by one triangle; the loop bounds stay scalar. A BODY that leaves a loop
// with `break` leaves the addresses behind — only the any-hit bodies do, on a condition (nothing left to answer) that stays true and
// makes every later loop leave before it reads a row.
#define PTSS_FOR_TRIANGLES_BY_CLASS(L, BODY, STEP)                                                                  \
    do {                                                                                                            \
        ClassBounds _cb = classBounds(L);                                                                           \
        PTSS_TRI_CLASS_LOOP(_cb, 0, 0, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 0, 1, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 0, 2, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 0, 3, BODY, STEP) \
        PTSS_TRI_CLASS_LOOP(_cb, 1, 0, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 1, 2, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 1, 3, BODY, STEP)      \
        PTSS_TRI_CLASS_LOOP(_cb, 2, 0, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 2, 1, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 2, 3, BODY, STEP)      \
        PTSS_TRI_CLASS_LOOP(_cb, 3, 0, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 3, 1, BODY, STEP) PTSS_TRI_CLASS_LOOP(_cb, 3, 2, BODY, STEP)      \
    } while (0)
#define PTSS_TRI_CLASS_LOOP(cb, c1, c2, BODY, STEP) \
    for (int t = classBegin<(c1) * 4 + (c2)>(cb), tEnd = classBegin<(c1) * 4 + (c2) + 1>(cb); t < tEnd; ++t, STEP) { BODY(c1, c2, t) }

// the any-hit form of the same bodies (lineOfSight is an OR over independent tests: any order)
template <int kC1, int kC2>
__device__ __forceinline__ void triangleClassedAny(const float4* rows, vec3 o, vec3 d, float limit, unsigned long long& need, unsigned long long& blocked) {
    const pttri::Head h = pttri::head<kC1, kC2, false>(xyz(loadRow16(rows)), xyz(loadRow16(rows + 1)), xyz(loadRow16(rows + 2)), v3(0, 0, 0), v3(0, 0, 0), 0.0f, o, d);
    const unsigned long long passMask = need & maskOf(!(ptm::abs(h.det) <= 1e-7f)) & maskOf(!(h.dist <= 0.0f)) & maskOf(!(h.dist > limit));
    if (passMask != 0ull) {
        float b0, b1, b2;
        pttri::weights<kC1, kC2>(h, d, b0, b1, b2);
        const unsigned long long hitMask = passMask & maskOf(!(__builtin_fminf(__builtin_fminf(b0, b1), b2) < 0));
        blocked |= hitMask;
        need &= ~hitMask;
    }
}
// ... and for the TWO segments of a surface point (pairAnyHit): the origin part once, a direction part per segment
template <int kC1, int kC2>
__device__ __forceinline__ void triangleClassedPair(const float4* rows, vec3 o, vec3 dA, float limitA, vec3 dB, float limitB, unsigned long long& needA,
                                                    unsigned long long& needB, unsigned long long& blockedA, unsigned long long& blockedB) {
    const vec3 e1 = xyz(loadRow16(rows + 1)), e2 = xyz(loadRow16(rows + 2));
    const pttri::OriginPart p = pttri::originPart<kC1, kC2>(xyz(loadRow16(rows)), e1, e2, o);
    if (needA != 0ull) {
        const pttri::Head h = pttri::headFrom<kC1, kC2>(p, e1, e2, dA);
        const unsigned long long pass = needA & maskOf(!(ptm::abs(h.det) <= 1e-7f)) & maskOf(!(h.dist <= 0.0f)) & maskOf(!(h.dist > limitA));
        if (pass != 0ull) {
            float b0, b1, b2;
            pttri::weights<kC1, kC2>(h, dA, b0, b1, b2);
            const unsigned long long hit = pass & maskOf(!(__builtin_fminf(__builtin_fminf(b0, b1), b2) < 0));
            blockedA |= hit;
            needA &= ~hit;
        }
    }
    if (needB != 0ull) {
        const pttri::Head h = pttri::headFrom<kC1, kC2>(p, e1, e2, dB);
        const unsigned long long pass = needB & maskOf(!(ptm::abs(h.det) <= 1e-7f)) & maskOf(!(h.dist <= 0.0f)) & maskOf(!(h.dist > limitB));
        if (pass != 0ull) {
            float b0, b1, b2;
            pttri::weights<kC1, kC2>(h, dB, b0, b1, b2);
            const unsigned long long hit = pass & maskOf(!(__builtin_fminf(__builtin_fminf(b0, b1), b2) < 0));
            blockedB |= hit;
            needB &= ~hit;
        }
    }
}
// what the class bodies need of a query (pttri.h): a finite direction short enough to bound |det|, a finite origin
__device__ __forceinline__ bool classedQueryOk(vec3 o, vec3 d) { return waveAll(dot(d, d) < 0x1p30f) && waveAll(dot(o, o) < 0x1p100f); }
// ---- Primary (bounce 0) variants. Every eye ray starts at camera.position, so whatever the tests
// compute from the ORIGIN and the primitive alone is the same for all lanes and all pixels of a frame:
//   sphere:   v = o - centre,  c = dot(v,v) - r^2                    (Primitives.h:109,113)
//   triangle: s = o - v0,  r = cross(s, e1),  dot(e2, r)             (Primitives.h:46-49)
// primaryPrepKernel evaluates these once per camera with the very same operations; the per-lane work
// that is left is identical to the generic tests (same values, same order), minus 8 of 15 / 12 of 55
// instructions.

__device__ __forceinline__ bool sphereTestPrimary(float4 pv, vec3 d, float limit, float& t) {
    const float b = dot(d, xyz(pv)) * 2;
    float disc = (b * b) - 4 * pv.w;
    if (disc < 0) return false;
    disc = ptm::sqrt(disc);
    float t0 = (-b + disc) * 0.5f;
    float t1 = (-b - disc) * 0.5f;
    if (t0 < 0 && t1 < 0) return false;
    if (t0 > t1) {
        const float tmp = t0;
        t0 = t1;
        t1 = tmp;
    }
    const float cand = (t0 < 0) ? t1 : t0;
    if (cand > limit) return false;
    t = cand;
    return true;
}

__device__ __forceinline__ TriHit triangleTestPrimary(const TriRows& tr, float4 ps /* s, dot(e2,r) */, float4 pr /* r */,
                                                      vec3 d, float limit, unsigned long long liveMask) {
    const vec3 e1 = xyz(tr.b), e2 = xyz(tr.c);
    const vec3 q = cross(d, e2);
    const float det = dot(e1, q);
    const float inverseDet = triRcp(det);  // 1 / det, Primitives.h:44; unused when |det| <= 1e-7
    const float dist = ps.w * inverseDet;
    const unsigned long long passMask = liveMask & maskOf(!(ptm::abs(det) <= 1e-7f)) & maskOf(!(dist <= 0.0f)) & maskOf(!(dist > limit));
    TriHit h;
    h.hit = false;
    h.hitMask = 0ull;
    h.dist = dist;
    h.w0 = h.w1 = h.w2 = 0;
    if (passMask != 0ull) {
        const float b1 = dot(xyz(ps), q) * inverseDet;
        const float b2 = dot(d, xyz(pr)) * inverseDet;
        const float b0 = 1.0f - (b1 + b2);
        h.hitMask = passMask & maskOf(!(b0 < 0)) & maskOf(!(b1 < 0)) & maskOf(!(b2 < 0));
        h.hit = __builtin_amdgcn_inverse_ballot_w64(h.hitMask);
        h.w0 = b0;
        h.w1 = b1;
        h.w2 = b2;
    }
    return h;
}

// ---- sphere candidate masks, CudaTracer.cu:127-133 / :438-444 through Primitives.h:107-118 -------------------------
// bit j of the result = "sphere j of this block of up to 32 passes the reference's discriminant test" — the very
// operations of the test above (Primitives.h:109-118), four spheres per trip: the four rows are fetched with one address and immediate offsets
// (the host pads the sphere rows to a multiple of four, ptpack.h layoutPlain; a padding row's bit is dropped by the caller's `keep`
// mask), and each verdict enters the mask through the carry of one add (mask = 2 * mask + verdict: v_cmp + v_addc
// instead of v_cmp + v_cndmask + v_or and a v_mov for the bit). That leaves the first sphere in the highest bit; one
// v_bfrev + shift puts sphere j at bit j, which the candidate loops need (they walk in index order).
// rev = 2 * rev + !(disc < 0) for one sphere, disc = b * b - 4 * c (Primitives.h:115-118). `disc < 0` is decided as
// `b * b < 4 * c`: a correctly rounded difference of two floats is negative exactly when the first is the smaller
// (gradual underflow: it is zero only for equal operands; inf - inf = NaN and a NaN operand make both forms false) —
// hipcc performs the same fold on its own. The verdict goes from VCC into the mask as the carry of one add.
__device__ __forceinline__ void shiftInMayHit(uint32_t& rev, float bb, float c4) {
    asm("v_cmp_nlt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(rev) : "v"(bb), "v"(c4) : "vcc");
}
// kBounded: the same verdict from two instructions less, on bounded geometry (SceneLayout::sphereBounded, set by
// ptss_create: every |coordinate| <= 1e15 and every sphere radius in [1e-12, 1e15]; the camera is checked per frame; ray
// origins — the camera or points on primitives — are then bounded as well). With h = d.v the reference compares
// RN((2h)^2) with 4c; doubling and quadrupling are exact, so that is 4 RN(h^2) < 4c, i.e. RN(h^2) < c, unless (a) 4c
// overflows — c < 2^105 here —, (b) 4 h^2 overflows — then h^2 >= 2^126 > c and both forms say "may hit" —, or (c) h^2 is
// subnormal and loses bits that 4 h^2 keeps — then h^2 < 2^-126, while c is zero or at least an ulp of r^2 >= 1e-24 in
// magnitude (a difference of two floats), so its sign decides both forms alike (c = 0: neither `<` holds). NaN or
// infinite operands make both compares false. Pinned on adversarial operands by tests/test_sphere_forms.py.
// kCull (the closest hit's masks and the many-sphere visits) also drops the spheres BEHIND the origin, which the reference rejects two lines further down (both roots negative,
// Primitives.h:126-127) — the sphere a reflected ray has just left above all (origin bumped 1e-4 off it: c ~ 2e-4 r, h ~ r), a
// candidate of every such ray otherwise, and every sphere the ray's line meets behind it. The mask compares h * m with c,
// m = min(h * 2^-18, h): h for h <= 0 — the very product h * h, nothing changes ahead of the origin — and 2^-18 h for h > 0.
// A sphere dropped that way has h > 0 and c > 2^-18 RN(h^2) =: k H. Then the reference computes disc = 4 RN(H - c) <
// 4 H (1 - k)(1 + 2^-24), s = RN(sqrt(disc)) < 2 h (1 + 2^-25)(1 - 2^-19 + 2^-24)(1 + 2^-24) < 2 h = b (exact doubling), so
// t0 = RN(-b + s) / 2 < 0 and t1 = RN(-b - s) / 2 < 0: rejected whatever the running distance — or disc < 0 and it was
// rejected before. (Scaling by 2^-18 is exact; where it underflows, floats are 2^-149 apart and c > RN(k H) still means
// c > k H. A NaN h stays a NaN m: kept, as before.) Pinned on corner operands, random bit patterns and operands a few ulps
// around the threshold by tests/test_sphere_behind.py. Same-box A/B: c3 +1.2 ... +2.0 %, c5 +1.7 %, c2 +0.6 %; in the 38-primitive
// scenes' shadow passes as well it bought nothing more (a blocked segment leaves at its first hit): they keep the plain mask.
// h for h <= 0, h * 2^-18 for h > 0 (one multiply, one v_min_f32)
template <bool kCull>
__device__ __forceinline__ float aheadFactor(float h) {
    if constexpr (kCull) {
        const float hk = h * 0x1p-18f;
        float m;
        asm("v_min_f32 %0, %1, %2" : "=v"(m) : "v"(hk), "v"(h));
        return m;
    } else {
        return h;
    }
}
template <bool kBounded, bool kCull = false>
__device__ __forceinline__ void shiftInSphere(uint32_t& rev, float4 sp, vec3 o, vec3 d) {  // Primitives.h:109-118
    const vec3 v = o - xyz(sp);
    if constexpr (kBounded) {
        const float h = dot(d, v);
        const float c = dot(v, v) - sp.w;
        shiftInMayHit(rev, h * aheadFactor<kCull>(h), c);
    } else {
        const float b = dot(d, v) * 2;
        const float c = dot(v, v) - sp.w;
        shiftInMayHit(rev, b * b, 4 * c);
    }
}
template <bool kBounded>
__device__ __forceinline__ void shiftInSpherePrimary(uint32_t& rev, float4 pv, vec3 d) {  // the same from the camera-origin precomputes
    if constexpr (kBounded) {
        const float h = dot(d, xyz(pv));
        shiftInMayHit(rev, h * h, pv.w);
    } else {
        const float b = dot(d, xyz(pv)) * 2;
        shiftInMayHit(rev, b * b, 4 * pv.w);
    }
}
// kStrips (bounce 0 with strip words, pthit.h closestHit): `wanted` is wave-uniform, bit j set unless sphere j is known to be rejected for
// every lane; a trip whose four bits are clear shifts four "no" verdicts in instead of testing (the caller drops the clear bits of
// the other trips from the finished mask).
template <bool kPrimary, bool kBounded, bool kStrips = false>
__device__ __forceinline__ uint32_t sphereCandidates(const float4* image, int firstRow, int cnt, vec3 o, vec3 d, uint32_t wanted = ~0u) {
    const int trips = (cnt + 3) >> 2;  // wave-uniform, 1..8
    uint32_t rev = 0;
    uint32_t at = vectorRow(image, firstRow);   // the trip's four rows through one vector address (ptwave.h)
    for (int g = 0; g < trips; ++g, at += 4 * kRowBytes) {
        if constexpr (kStrips) {
            if (((wanted >> (4 * g)) & 15u) == 0u) {
                rev <<= 4;
                continue;
            }
        }
        const float4* p = rowAt(image, at);
        const float4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
        if constexpr (kPrimary) {
            shiftInSpherePrimary<kBounded>(rev, r0, d);
            shiftInSpherePrimary<kBounded>(rev, r1, d);
            shiftInSpherePrimary<kBounded>(rev, r2, d);
            shiftInSpherePrimary<kBounded>(rev, r3, d);
        } else {
            shiftInSphere<kBounded, true>(rev, r0, o, d);
            shiftInSphere<kBounded, true>(rev, r1, o, d);
            shiftInSphere<kBounded, true>(rev, r2, o, d);
            shiftInSphere<kBounded, true>(rev, r3, o, d);
        }
    }
    return __builtin_bitreverse32(rev) >> (32 - 4 * trips);
}
// two spheres per trip: for the shadow passes, where the registers are needed elsewhere (four rows in flight there
// push the 72-VGPR kernel into scratch)
template <bool kBounded>
__device__ __forceinline__ uint32_t sphereCandidatesPairs(const float4* image, int firstRow, int cnt, vec3 o, vec3 d) {
    const int trips = (cnt + 1) >> 1;  // 1..16
    uint32_t rev = 0;
    uint32_t at = vectorRow(image, firstRow);
    for (int g = 0; g < trips; ++g, at += 2 * kRowBytes) {
        const float4* p = rowAt(image, at);
        const float4 r0 = p[0], r1 = p[1];
        shiftInSphere<kBounded>(rev, r0, o, d);
        shiftInSphere<kBounded>(rev, r1, o, d);
    }
    return __builtin_bitreverse32(rev) >> (32 - 2 * trips);
}
template <bool kBounded>
__device__ __forceinline__ uint32_t sphereCandidatesStridedPairs(const float4* first, int stride, int cnt, vec3 o, vec3 d) {
    const int trips = (cnt + 1) >> 1;
    uint32_t rev = 0;
    for (int g = 0; g < trips; ++g) {
        const float4* p = first + 2 * g * stride;
        const float4 r0 = p[0], r1 = p[stride];
        shiftInSphere<kBounded>(rev, r0, o, d);
        shiftInSphere<kBounded>(rev, r1, o, d);
    }
    return __builtin_bitreverse32(rev) >> (32 - 2 * trips);
}

}  // namespace
}  // namespace ptss
