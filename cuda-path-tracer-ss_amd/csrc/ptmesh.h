// ptmesh.h — the conservative bound of the mesh image (SceneLayout::mesh): "may this ray be accepted by Triangle::intersectRay
// (Primitives.h:25-83) for some triangle inside this leaf or group?" Written once for the gfx950 kernels (ptss_kernels.hip) and for
// a host probe (host_capi.cpp ptss_probe_mesh_bound, tests/test_mesh_bound.py). The derivation of the predicate and of its
// constants sits at the construction of the bounds (ptpack.h packMeshBounds); DESIGN.md §3.15 summarises it.
//
// A bound is three rows of four floats:
//   {C, R}                  a ball that holds every vertex v0, v0 + e1, v0 + e2 of its triangles (e1, e2 as stored)
//   {a, cosA}               a unit axis and the cosine of the half-angle of a double cone that holds every unit normal
//   {sinA, Nmin, Lmax, B}   the sine of that angle, min |e1 x e2|, the longest side, and B = 64 u |d|max Lmax^2 (rounded up)
// The verdict is "may touch" unless the ray's half line provably passes farther from C than R + infl, where infl grows
// with 1 / D, D a lower bound of |det| that the cone gives for this direction, or the 1e-7 floor the reference's own test
// puts on |det|. When D cannot be shown to exceed 4 eta (eta = the bound on the rounding error of det), the ray may graze
// a triangle so flatly that its computed weights say nothing about where it passes: the verdict is then "may touch".
// Preconditions, checked by the caller once per query: |d|^2 within kMeshDirEps of 1 and a finite origin with |o|^2 < 2^100;
// every vertex of the image within |coordinate| <= 2^40 (packScene).
#pragma once
#include "ptmath.h"

namespace ptmesh {
using namespace ptv;

constexpr float kU = 0x1p-24f;                 // unit roundoff of float32
constexpr float kMeshDirEps = 1e-5f;           // | |d|^2 - 1 | up to which a direction counts as unit
constexpr float kDirNorm = 1.00001f;           // >= |d| for such a direction
constexpr float kInvDir2 = 1.0000101f;         // >= 1 / |d|^2 for such a direction
constexpr double kBPerL2 = 64.0 * 0x1p-24 * 1.00001;     // B = this * Lmax^2: the coefficient of sigma / D in infl (60 u |d| Lmax^2)
constexpr float kEtaOfB = 0.1875f;             // eta = kEtaOfB * B = 12 u |d|max Lmax^2 >= the rounding error of det (9.1 u |e1||e2||d|)
constexpr float kDetFloor = 1e-7f;             // Primitives.h:41, the reference's |det| <= 1e-7 (a float literal)
constexpr float kSlackDir = 0x1p-20f;          // the cone term's allowance for rounding (|d . a| and the float axis)
constexpr float kRel = 0x1p-16f;               // relative allowance of the float evaluation below
constexpr float kInflRel = 1.0f + 0x1p-10f;    // ... and of infl's positive terms

// margin = 1 in the kernels (every multiplication by it folds away). The probe takes smaller values, which scale every rounding-error
// allowance of the bound — eta, the B term, the cone's slack, infl — so that a test can show that an under-inflated bound fails
// (margin = 0: the bare ball).
PTM_HD bool mayTouch(vec3 C, float R, vec3 a, float cosA, float sinA, float nmin, float lmax, float B, vec3 o, vec3 d, float margin) {
    const vec3 v = o - C;
    const float vv = dot(v, v);
    const float dv = dot(d, v);
    const float t = dv < 0.0f ? dv : 0.0f;                        // the closest approach of the LINE, if it lies ahead
    const float away2 = vv * (1.0f - kRel) - kInvDir2 * (t * t);  // <= (distance of C from the half line)^2
    const float sigma = ptm::sqrt(vv) * (1.0f + kRel) + R;        // >= |o - v0| for every vertex v0 of the bound
    const float da = ptm::abs(dot(d, a));
    const float coneD = nmin * ((da * cosA - kDirNorm * sinA) - kSlackDir * margin);   // <= |det| of every triangle, by the cone
    const float Bm = B * margin;
    const float eta = kEtaOfB * Bm;
    const float floorD = kDetFloor - eta;                         // an accepted det has |det_f| > 1e-7, so |det| >= 1e-7 - eta
    const float D = (coneD > floorD ? coneD : floorD) * (1.0f - kRel);
    const float invD = ptm::rcp_in_range(D);                      // used only when D >= 4 eta (then 2^-25 < D < 2^126)
    const float infl = kInflRel * (lmax * (4.0f * kU * margin + 1.02f * eta * invD) + Bm * sigma * invD + 1e-30f * margin);
    const float reach = R + infl;
    const bool far = away2 > reach * reach * (1.0f + kRel);
    return !(D >= 4.0f * eta) || !far;                            // NaN anywhere: "may touch"
}

// The twelve floats of the bound around n triangles given as {v0, e1, e2} (nine floats each, as the image stores them), computed
// in double from the exact float inputs and rounded outwards (host only: ptpack.h packMeshBounds and the probe).
inline void buildBound(const float* tri9, int n, float out[12]) {
    auto up = [](double x) { float f = (float)(x * (1 + 1e-12)); return f < x * (1 + 1e-12) ? __builtin_nextafterf(f, __builtin_inff()) : f; };
    auto down = [](double x) { float f = (float)(x * (1 - 1e-12)); return (double)f > x * (1 - 1e-12) ? __builtin_nextafterf(f, -__builtin_inff()) : f; };
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    auto vertex = [&](int i, int k, double p[3]) {   // v0, v0 + e1, v0 + e2 (exact in double)
        const float* t = tri9 + 9 * i;
        for (int c = 0; c < 3; ++c) p[c] = (double)t[c] + (k == 0 ? 0.0 : (double)t[3 * k + c]);
    };
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            double p[3];
            vertex(i, k, p);
            for (int c = 0; c < 3; ++c) { lo[c] = p[c] < lo[c] ? p[c] : lo[c]; hi[c] = p[c] > hi[c] ? p[c] : hi[c]; }
        }
    float Cf[3];
    for (int c = 0; c < 3; ++c) Cf[c] = (float)(0.5 * (lo[c] + hi[c]));
    double R = 0, lmax = 0, nmin = __builtin_inf(), sum[3] = {0, 0, 0}, ref[3] = {0, 0, 0}, refLen = 0;
    for (int i = 0; i < n; ++i) {
        const float* t = tri9 + 9 * i;
        for (int k = 0; k < 3; ++k) {
            double p[3];
            vertex(i, k, p);
            const double dx = p[0] - Cf[0], dy = p[1] - Cf[1], dz = p[2] - Cf[2];
            R = __builtin_fmax(R, __builtin_sqrt(dx * dx + dy * dy + dz * dz));
        }
        const double e1[3] = {t[3], t[4], t[5]}, e2[3] = {t[6], t[7], t[8]}, e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
        for (const double* e : {e1, e2, e3}) lmax = __builtin_fmax(lmax, __builtin_sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]));
        const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = __builtin_sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
        nmin = __builtin_fmin(nmin, len);
        if (len > refLen) { refLen = len; for (int c = 0; c < 3; ++c) ref[c] = N[c] / len; }
    }
    for (int i = 0; i < n && refLen > 0; ++i) {   // the unit normals, each turned to the side of the largest triangle's
        const float* t = tri9 + 9 * i;
        const double N[3] = {(double)t[4] * t[8] - (double)t[5] * t[7], (double)t[5] * t[6] - (double)t[3] * t[8], (double)t[3] * t[7] - (double)t[4] * t[6]};
        const double len = __builtin_sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
        if (!(len > 0)) continue;
        const double s = (N[0] * ref[0] + N[1] * ref[1] + N[2] * ref[2]) < 0 ? -1.0 : 1.0;
        for (int c = 0; c < 3; ++c) sum[c] += s * N[c] / len;
    }
    double a[3] = {1, 0, 0}, cosA = 0;
    const double sl = __builtin_sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
    if (sl > 0 && nmin > 0) {
        for (int c = 0; c < 3; ++c) a[c] = sum[c] / sl;
        cosA = 1;
        for (int i = 0; i < n; ++i) {
            const float* t = tri9 + 9 * i;
            const double N[3] = {(double)t[4] * t[8] - (double)t[5] * t[7], (double)t[5] * t[6] - (double)t[3] * t[8], (double)t[3] * t[7] - (double)t[4] * t[6]};
            const double len = __builtin_sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
            cosA = __builtin_fmin(cosA, __builtin_fabs(N[0] * a[0] + N[1] * a[1] + N[2] * a[2]) / len);
        }
        cosA = __builtin_fmax(0.0, cosA - 1e-9);
    }
    const double sinA = __builtin_fmin(1.0, __builtin_sqrt(1 - cosA * cosA) + 1e-9);
    const float L = up(lmax);
    const float vals[12] = {Cf[0], Cf[1], Cf[2], up(R), (float)a[0], (float)a[1], (float)a[2], down(cosA),
                            up(sinA) > 1.0f ? 1.0f : up(sinA), down(nmin > 0 ? nmin : 0.0), L, up(kBPerL2 * (double)L * (double)L)};
    for (int k = 0; k < 12; ++k) out[k] = vals[k];
}

// ---- REFIT: the same twelve floats recomputed from the stored rows of a live image (ptss_update_triangles) -------
// Written once for the device (ptss_update.hip meshRefitKernel) and the host (refitBound below, ptss_probe_mesh_refit), both built
// with -ffp-contract=off: every value is a fixed expression of correctly rounded double operations (+, -, *, /, sqrt; products
// and sums of two floats are exact in double), so the two sides agree bit for bit. What is reduced over the triangles of a bound:
//   the box (minima and maxima: order-free)                                        -> C, rounded to float
//   max |p - C|^2, max |side|^2, min |e1 x e2| (order-free) and the AXIS SUM        -> R, Lmax, Nmin, the axis a
//   min |N . a| / |N| (order-free)                                                  -> cos alpha
// The axis sum is the one order-dependent quantity. Its shape is fixed by STORED POSITION: slot k of a group of kRefitSlots
// holds the unit normal of position 256 g + k (zero for an empty slot or a triangle without area); the slots are merged as a
// complete binary tree, level by level (k with k + 1, then blocks of two, of four, ...), each merge being
//   lower + upper    if lower . upper >= 0 (ties and zero vectors included),      lower - upper    otherwise
// — the block of lower positions decides the side, so no reference normal has to be known in advance (buildBound turns every
// normal to the side of the largest triangle's: a different, equally legal axis; any axis is sound, cos alpha being measured
// against the axis chosen). A leaf is the aligned block of 16 slots, so its sum is a node of its group's tree.
// Rounding is buildBound's: C to nearest and R measured from the rounded C; R, Lmax, sin alpha and B up; Nmin and cos alpha down;
// cos alpha - 1e-9 and sin alpha + 1e-9 pay for the double arithmetic. sqrt(max x) = max sqrt(x) for a correctly rounded sqrt.
constexpr int kRefitSlots = 256;   // positions per group = 16 leaves of 16

PTM_HD double dsqrt(double x) { return __builtin_sqrt(x); }
PTM_HD double dmin(double a, double b) { return b < a ? b : a; }
PTM_HD double dmax(double a, double b) { return b > a ? b : a; }
PTM_HD float floatAbove(float f) {   // the next float towards +inf (finite f)
    const uint32_t u = __builtin_bit_cast(uint32_t, f);
    return (u << 1) == 0u ? __builtin_bit_cast(float, 1u) : __builtin_bit_cast(float, (u >> 31) ? u - 1u : u + 1u);
}
PTM_HD float floatBelow(float f) { return -floatAbove(-f); }
PTM_HD float roundUp(double x) { const double y = x * (1 + 1e-12); const float f = (float)y; return (double)f < y ? floatAbove(f) : f; }
PTM_HD float roundDown(double x) { const double y = x * (1 - 1e-12); const float f = (float)y; return (double)f > y ? floatBelow(f) : f; }

struct RefitBox { double lo[3], hi[3]; };
struct RefitStat { double r2, l2, nmin, sum[3]; };   // max |p - C|^2, max |side|^2, min |e1 x e2|, the axis sum

PTM_HD RefitBox refitEmptyBox() { return {{__builtin_inf(), __builtin_inf(), __builtin_inf()}, {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()}}; }
PTM_HD RefitStat refitEmptyStat() { return {0.0, 0.0, __builtin_inf(), {0.0, 0.0, 0.0}}; }
PTM_HD void refitVertex(const float* t, int k, double p[3]) {   // v0, v0 + e1, v0 + e2 (exact in double)
    for (int c = 0; c < 3; ++c) p[c] = (double)t[c] + (k == 0 ? 0.0 : (double)t[3 * k + c]);
}
PTM_HD void refitNormal(const float* t, double N[3]) {
    N[0] = (double)t[4] * t[8] - (double)t[5] * t[7];
    N[1] = (double)t[5] * t[6] - (double)t[3] * t[8];
    N[2] = (double)t[3] * t[7] - (double)t[4] * t[6];
}
PTM_HD double refitLen(const double v[3]) { return dsqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

PTM_HD RefitBox refitBoxOf(const float* t) {
    RefitBox b = refitEmptyBox();
    for (int k = 0; k < 3; ++k) {
        double p[3];
        refitVertex(t, k, p);
        for (int c = 0; c < 3; ++c) { b.lo[c] = dmin(b.lo[c], p[c]); b.hi[c] = dmax(b.hi[c], p[c]); }
    }
    return b;
}
PTM_HD RefitBox refitMerge(const RefitBox& a, const RefitBox& b) {
    RefitBox o;
    for (int c = 0; c < 3; ++c) { o.lo[c] = dmin(a.lo[c], b.lo[c]); o.hi[c] = dmax(a.hi[c], b.hi[c]); }
    return o;
}
PTM_HD void refitCentre(const RefitBox& b, float Cf[3]) {
    for (int c = 0; c < 3; ++c) Cf[c] = (float)(0.5 * (b.lo[c] + b.hi[c])) + 0.0f;   // (+ 0: a box of -0 and +0 gives +0 in any order)
}
// max |p - C|^2 over the triangle's three vertices, C the rounded centre of the bound it is measured for
PTM_HD double refitReach2(const float* t, const float Cf[3]) {
    double r2 = 0.0;
    for (int k = 0; k < 3; ++k) {
        double p[3];
        refitVertex(t, k, p);
        const double dx = p[0] - Cf[0], dy = p[1] - Cf[1], dz = p[2] - Cf[2];
        r2 = dmax(r2, dx * dx + dy * dy + dz * dz);
    }
    return r2;
}
// the centre-free part of a slot: r2 is left 0 (refitReach2 fills it per bound)
PTM_HD RefitStat refitStatOf(const float* t) {
    RefitStat s = refitEmptyStat();
    const double e1[3] = {t[3], t[4], t[5]}, e2[3] = {t[6], t[7], t[8]}, e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
    s.l2 = dmax(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], dmax(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2], e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]));
    double N[3];
    refitNormal(t, N);
    const double len = refitLen(N);
    s.nmin = len;
    if (len > 0)
        for (int c = 0; c < 3; ++c) s.sum[c] = N[c] / len;
    return s;
}
// `lo`: the block of lower stored positions (it decides the side the upper block's sum is added on)
PTM_HD RefitStat refitMerge(const RefitStat& lo, const RefitStat& hi) {
    RefitStat o;
    o.r2 = dmax(lo.r2, hi.r2);
    o.l2 = dmax(lo.l2, hi.l2);
    o.nmin = dmin(lo.nmin, hi.nmin);
    const double along = lo.sum[0] * hi.sum[0] + lo.sum[1] * hi.sum[1] + lo.sum[2] * hi.sum[2];
    for (int c = 0; c < 3; ++c) o.sum[c] = along < 0 ? lo.sum[c] - hi.sum[c] : lo.sum[c] + hi.sum[c];
    return o;
}
// the unit axis of a finished sum; false: no cone (a triangle without area inside, or normals that cancel) — cos alpha = 0
PTM_HD bool refitAxis(const RefitStat& s, double a[3]) {
    const double sl = refitLen(s.sum);
    a[0] = 1; a[1] = 0; a[2] = 0;
    if (!(sl > 0 && s.nmin > 0)) return false;
    for (int c = 0; c < 3; ++c) a[c] = s.sum[c] / sl;
    return true;
}
PTM_HD double refitCos(const float* t, const double a[3]) {   // only where refitAxis returned true (every |N| > 0)
    double N[3];
    refitNormal(t, N);
    return __builtin_fabs(N[0] * a[0] + N[1] * a[1] + N[2] * a[2]) / refitLen(N);
}
// cosMin: min refitCos over the bound's triangles (1 when there is none to lower it), ignored without an axis
PTM_HD void refitFinish(const float Cf[3], const RefitStat& s, const double a[3], bool haveAxis, double cosMin, float out[12]) {
    const double cosA = haveAxis ? dmax(0.0, dmin(1.0, cosMin) - 1e-9) : 0.0;
    const double sinA = dmin(1.0, dsqrt(1 - cosA * cosA) + 1e-9);
    const float L = roundUp(dsqrt(s.l2));
    const float sinF = roundUp(sinA);
    out[0] = Cf[0]; out[1] = Cf[1]; out[2] = Cf[2]; out[3] = roundUp(dsqrt(s.r2));
    out[4] = (float)a[0]; out[5] = (float)a[1]; out[6] = (float)a[2]; out[7] = roundDown(cosA);
    out[8] = sinF > 1.0f ? 1.0f : sinF;
    out[9] = roundDown(s.nmin > 0 ? s.nmin : 0.0);
    out[10] = L;
    out[11] = roundUp(kBPerL2 * (double)L * (double)L);
}

// The refit of ONE bound on the host, in the kernel's reduction shape: the n triangles at consecutive stored positions starting
// at a multiple of `slots` — 16: a leaf (n <= 16), kRefitSlots: a group. (The tree is walked over all `slots` slots, empty ones
// included, as the kernel does: adding an empty slot's +0 turns a -0 component of the sum into +0.)
inline void refitBound(const float* tri9, int n, int slots, float out[12]) {
    RefitBox box = refitEmptyBox();
    for (int i = 0; i < n; ++i) box = refitMerge(box, refitBoxOf(tri9 + 9 * i));
    float Cf[3];
    refitCentre(box, Cf);
    RefitStat slot[kRefitSlots];
    for (int i = 0; i < kRefitSlots; ++i) {
        slot[i] = refitEmptyStat();
        if (i < n) { slot[i] = refitStatOf(tri9 + 9 * i); slot[i].r2 = refitReach2(tri9 + 9 * i, Cf); }
    }
    for (int step = 1; step < slots; step *= 2)
        for (int i = 0; i < slots; i += 2 * step) slot[i] = refitMerge(slot[i], slot[i + step]);
    double a[3], cosMin = 1.0;
    const bool haveAxis = refitAxis(slot[0], a);
    for (int i = 0; i < n && haveAxis; ++i) cosMin = dmin(cosMin, refitCos(tri9 + 9 * i, a));
    refitFinish(Cf, slot[0], a, haveAxis, cosMin, out);
}

}  // namespace ptmesh
