// ptstrip.h — which primitives the eye rays of one 64-pixel strip can reach: one 64-bit word per strip of a context's local
// pixel plane, bits 0-31 the stored sphere positions, bits 32-63 the stored triangle positions. Bounce 0 of a plain, bounded image
// of at most 32 spheres and 32 triangles visits only the primitives whose bit is set (pthit.h closestHit, kPrimary). The words
// depend on the camera and the scene alone: stripMaskKernel (ptss_kernels.hip) fills them beside primaryPrepKernel, once per
// camera. Written once for that kernel and for the host (host_capi.cpp ptss_probe_strip_masks, tests/test_strip_masks_cpu.py).
// Restates no reference line: it decides only which of the reference's tests cannot accept. DESIGN.md §3.25 has the proof;
// the rule, with the constants below:
//
//   THE PYRAMID. The eye ray of pixel (x, gy) with jitter (jx, jy) in [0, 1]^2 has the direction of M (u, v, 1) zNear (zNear of either sign), M the linear
//   map of ptv::rotate(q, .), u = ((x + jx) invW - 0.5) s, v = ((gy + jy) invH - 0.5) s aspect. A strip's pixels fill a rectangle
//   of one row (two rectangles when it wraps over a row end); the rectangle grows by kPixelMargin pixels on every side, and its
//   four corner directions span a cone in world space whose side planes pass through the camera. The float evaluation of a
//   direction (five roundings up to `start`, rotate, normalize) leaves it within 3e-6 rad of the real one in the camera domain
//   below; every test treats a ray as lying within kTheta = 1e-4 rad of the cone.
//   A SPHERE loses its bit when its centre lies outside one side plane, or behind the camera, by more than r_eff + kTheta (|v| +
//   r_eff), r_eff^2 = r^2 + kSphereRel |v|^2 — the reference's float discriminant can be >= 0 only for a line within r_eff of
//   the centre — and the camera is outside it by |v|^2 > r^2 (1 + kInsideRel).
//   A TRIANGLE loses its bit when the camera is off its plane (|s . N| >= kPlaneRel smax |e1| |e2|: the float distance then has
//   the real one's sign), no corner ray grazes it (every corner direction has c^ . N of one sign and at least kGraze |e1| |e2| +
//   kTheta |N| in size: |det| then exceeds its own rounding error a thousandfold), and the triangle ENLARGED about its centroid
//   by 1 + 3 beta, beta = kWeightEps smax (|e1| + |e2|) / min |c^ . N| + 1e-6 the bound of the float weights' error, has its three
//   corners outside the same plane by kTheta times their distance.
//   EVERYTHING ELSE KEEPS ITS BIT: a camera outside the domain (position beyond kCoordLimit, a quaternion not unit to 1e-3, |zNear|
//   outside [2^-30, 2^30], |s| max(1, aspect) > 16), a primitive with a coordinate beyond kCoordLimit, a strip over more than two
//   rows — and any comparison that a NaN makes false: every cull is written as `value < -slack` after `if (!(x >= bound)) keep`.
// The arithmetic is double: its own rounding (1e-16) is nothing beside the slacks, so the host and device builds may differ in a
// last bit without either leaving the rule.
#pragma once
#include "ptlocate.h"
#include "ptscene.h"

namespace ptstrip {

constexpr unsigned long long kAll = ~0ull;
constexpr int kMaxPerKind = 32;          // spheres, and triangles, a word has bits for
constexpr double kPixelMargin = 1.0;     // whole pixels added to a strip's rectangle on every side
constexpr double kTheta = 1e-4;          // a float eye ray lies within this angle (rad) of the real pyramid: 30 times the bound
constexpr double kSphereRel = 1e-5;      // r_eff^2 = r^2 + kSphereRel |v|^2: 5 times the float discriminant's error bound
constexpr double kInsideRel = 2e-3;      // the camera counts as inside a sphere up to |v|^2 = r^2 (1 + kInsideRel)
constexpr double kGraze = 1e-3;          // a corner ray grazes a triangle when |c^ . N| < kGraze |e1| |e2| (+ kTheta |N|)
constexpr double kPlaneRel = 1e-4;       // the camera lies in a triangle's plane when |s . N| < kPlaneRel smax |e1| |e2|
constexpr double kWeightEps = 16.0 / 16777216.0;   // 16 x 2^-24: the float weights' error is below 7 x 2^-24 |s| |e| / |det| each
constexpr double kCoordLimit = 1048576.0;          // 2^20: no float intermediate of either test overflows below it

struct D3 {
    double x, y, z;
};
PTM_HD D3 d3(double x, double y, double z) { return D3{x, y, z}; }
PTM_HD D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PTM_HD D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PTM_HD D3 operator*(D3 a, double s) { return D3{a.x * s, a.y * s, a.z * s}; }
PTM_HD double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PTM_HD D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
PTM_HD double length(D3 a) { return __builtin_sqrt(dot(a, a)); }
PTM_HD double absd(double x) { return __builtin_fabs(x); }
PTM_HD bool within(double x, double limit) { return absd(x) <= limit; }   // false for NaN and infinities
PTM_HD bool within(D3 a, double limit) { return within(a.x, limit) && within(a.y, limit) && within(a.z, limit); }

// what the eye-ray code reads of a frame (ptss_device.h EyeParams: the same float values)
struct View {
    ptss_camera camera;
    float s, aspect, invW, invH;
};
// where a context's local pixels sit in the frame (ptss_device.h TileMap)
struct Tile {
    int width, rank, world, bandRows;
};

PTM_HD bool viewInDomain(const View& v) {
    const ptss_quat q = v.camera.rotation;
    const double qq = (double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z + (double)q.w * q.w;
    const double s = v.s, a = v.aspect;
    return within(d3(v.camera.position.x, v.camera.position.y, v.camera.position.z), kCoordLimit) && qq >= 1.0 - 1e-3 && qq <= 1.0 + 1e-3 &&
           absd((double)v.camera.zNear) >= 0x1p-30 && absd((double)v.camera.zNear) <= 0x1p30 && absd(s) >= 0x1p-20 && a > 0.0 && absd(s) * (a > 1.0 ? a : 1.0) <= 16.0 &&
           v.invW > 0.0f && v.invW <= 1.0f && v.invH > 0.0f && v.invH <= 1.0f;
}

// ptv::rotate's linear map in double: v + 2 w (u x v) + 2 (u x (u x v))
PTM_HD D3 rotated(ptss_quat q, D3 v) {
    const D3 u = d3(q.x, q.y, q.z);
    const D3 uv = cross(u, v);
    const D3 uuv = cross(u, uv);
    return (v + uv * (2.0 * (double)q.w)) + uuv * 2.0;
}

// The cone of the eye rays through the pixels [x0, x1] x [y0, y1] (frame coordinates, inclusive), grown by the margin: inward unit
// normals of its four side planes and of the plane behind which no ray points, and its four unit corner directions.
struct Pyramid {
    D3 n[5];
    D3 corner[4];
    bool ok;
};
PTM_HD Pyramid pyramidOf(const View& v, int x0, int x1, int y0, int y1) {
    Pyramid p;
    p.ok = false;
    const double s = v.s, sy = (double)v.s * (double)v.aspect;
    const double ua = (((double)x0 - kPixelMargin) * (double)v.invW - 0.5) * s, ub = (((double)x1 + 1.0 + kPixelMargin) * (double)v.invW - 0.5) * s;
    const double va = (((double)y0 - kPixelMargin) * (double)v.invH - 0.5) * sy, vb = (((double)y1 + 1.0 + kPixelMargin) * (double)v.invH - 0.5) * sy;
    const ptss_quat q = v.camera.rotation;
    const double z = v.camera.zNear < 0.0f ? -1.0 : 1.0;   // `start` is (u, v, 1) zNear: the reference's cameras have zNear < 0 and look along -z
    const D3 w[4] = {rotated(q, d3(ua, va, 1.0) * z), rotated(q, d3(ub, va, 1.0) * z), rotated(q, d3(ub, vb, 1.0) * z), rotated(q, d3(ua, vb, 1.0) * z)};
    const D3 centre = rotated(q, d3(0.5 * (ua + ub), 0.5 * (va + vb), 1.0) * z);
    const double centreLen = length(centre);
    if (!(centreLen > 0.0)) return p;
    bool ok = true;
    for (int k = 0; k < 5; ++k) {
        D3 n = k < 4 ? cross(w[k], w[(k + 1) & 3]) : cross(rotated(q, d3(1.0, 0.0, 0.0)), rotated(q, d3(0.0, 1.0, 0.0)));
        const double len = length(n);
        if (!(len > 0.0) || !within(len, 1e300)) return p;
        n = n * (1.0 / len);
        const double side = dot(n, centre) / centreLen;   // the sine of the angle between the centre ray and the plane
        if (side < 0.0) n = n * -1.0;
        ok = ok && absd(side) > 1e-9;                   // (false for NaN) a degenerate rectangle keeps everything
        p.n[k] = n;
    }
    for (int k = 0; k < 4; ++k) {
        const double len = length(w[k]);
        if (!(len > 0.0) || !within(len, 1e300)) return p;
        p.corner[k] = w[k] * (1.0 / len);
    }
    p.ok = ok;
    return p;
}

// sphere row {centre, r^2}: true only when no float eye ray of the pyramid can be accepted by Sphere::intersectRay
PTM_HD bool sphereCulled(const Pyramid& p, D3 o, const float* row) {
    const D3 c = d3(row[0], row[1], row[2]);
    const double r2 = row[3];
    if (!within(c, kCoordLimit) || !(r2 > 0.0) || !(r2 <= kCoordLimit * kCoordLimit)) return false;
    const D3 v = c - o;
    const double vv = dot(v, v);
    if (!(vv > r2 * (1.0 + kInsideRel))) return false;   // the camera inside the sphere or within slack of it (or a NaN)
    const double reff = __builtin_sqrt(r2 + kSphereRel * vv);
    const double slack = reff + kTheta * (__builtin_sqrt(vv) + reff);
    for (int k = 0; k < 5; ++k)
        if (dot(p.n[k], v) < -slack) return true;
    return false;
}

// triangle rows {v0, .}, {e1, .}, {e2, .}: true only when no float eye ray of the pyramid can be accepted by Triangle::intersectRay
PTM_HD bool triangleCulled(const Pyramid& p, D3 o, const float* rows) {
    const D3 v0 = d3(rows[0], rows[1], rows[2]), e1 = d3(rows[4], rows[5], rows[6]), e2 = d3(rows[8], rows[9], rows[10]);
    if (!within(v0, kCoordLimit) || !within(e1, 2.0 * kCoordLimit) || !within(e2, 2.0 * kCoordLimit)) return false;
    const D3 N = cross(e1, e2);
    const double l1 = length(e1), l2 = length(e2), L2 = l1 * l2, lenN = length(N);
    if (!(L2 > 0.0)) return false;
    const D3 vert[3] = {v0, v0 + e1, v0 + e2};   // the triangle the test sees: its stored edges, not the caller's other two vertices
    const D3 s0 = vert[0] - o, s1 = vert[1] - o, s2 = vert[2] - o;
    double smax = length(s0);
    const double len1 = length(s1), len2 = length(s2);
    smax = len1 > smax ? len1 : smax;
    smax = len2 > smax ? len2 : smax;
    if (!(absd(dot(s0, N)) >= kPlaneRel * smax * L2)) return false;   // the camera in, or within slack of, the triangle's plane
    double lo = 0.0;
    int positive = 0, negative = 0;
    for (int k = 0; k < 4; ++k) {
        const double a = dot(p.corner[k], N);
        positive += a > 0.0 ? 1 : 0;
        negative += a < 0.0 ? 1 : 0;
        const double m = absd(a);
        lo = (k == 0 || m < lo) ? m : lo;
    }
    if (positive != 4 && negative != 4) return false;   // the plane's direction set crosses the pyramid: grazing for some ray of it
    const double detMin = lo - kTheta * lenN;
    if (!(detMin >= kGraze * L2)) return false;         // a corner ray grazes the triangle
    const double beta = kWeightEps * smax * (l1 + l2) / detMin + 1e-6;
    if (!within(beta, 1e6)) return false;
    const D3 g = (vert[0] + vert[1] + vert[2]) * (1.0 / 3.0);
    D3 big[3];
    double far[3];
    for (int i = 0; i < 3; ++i) {
        big[i] = (g + (vert[i] - g) * (1.0 + 3.0 * beta)) - o;
        far[i] = kTheta * length(big[i]);
    }
    for (int k = 0; k < 5; ++k)
        if (dot(p.n[k], big[0]) < -far[0] && dot(p.n[k], big[1]) < -far[1] && dot(p.n[k], big[2]) < -far[2]) return true;
    return false;
}

// the word of the pixels [x0, x1] of frame row y: bit j / 32 + t set unless stored sphere j / triangle t is culled; the bits past
// the counts stay clear (no test reads them)
PTM_HD unsigned long long rectMask(const View& v, const float* blob, const ptss::SceneLayout& L, int x0, int x1, int y) {
    const Pyramid p = pyramidOf(v, x0, x1, y, y);
    if (!p.ok) return kAll;
    const D3 o = d3(v.camera.position.x, v.camera.position.y, v.camera.position.z);
    unsigned long long m = 0ull;
    for (int j = 0; j < L.numSpheres; ++j)
        if (!sphereCulled(p, o, blob + 4 * (size_t)(L.offSphere + j))) m |= 1ull << j;
    for (int t = 0; t < L.numTriangles; ++t)
        if (!triangleCulled(p, o, blob + 4 * (size_t)(L.offTri + 3 * t))) m |= 1ull << (32 + t);
    return m;
}

// the images bounce 0 culls on: plain (no sphere chunks, no mesh), bounded with the camera in range (`bounded`: the kernels'
// kBounded), stored grouped by edge class, and small enough for one word
inline bool eligible(const ptss::SceneLayout& L, bool bounded) {
    return bounded && !L.accelSpheres && L.triClassed && L.numSpheres <= kMaxPerKind && L.numTriangles <= kMaxPerKind;
}

// the word of the strip whose first local pixel is `first` (a multiple of 64) in a context of numPixels local pixels
PTM_HD unsigned long long stripMask(const View& v, const Tile& t, uint32_t numPixels, uint32_t first, const float* blob, const ptss::SceneLayout& L) {
    if (first >= numPixels || L.numSpheres > kMaxPerKind || L.numTriangles > kMaxPerKind || !viewInDomain(v)) return kAll;
    const uint32_t last = (first + (ptloc::kStrip - 1) < numPixels) ? first + (ptloc::kStrip - 1) : numPixels - 1;
    const uint32_t rowFirst = first / (uint32_t)t.width, rowLast = last / (uint32_t)t.width;
    if (rowLast - rowFirst > 1u) return kAll;   // more than two rows (width < 64)
    const ptloc::Coord a = ptloc::locate(t.width, t.rank, t.world, t.bandRows, first);
    const ptloc::Coord b = ptloc::locate(t.width, t.rank, t.world, t.bandRows, last);
    if (rowLast == rowFirst) return rectMask(v, blob, L, a.x, b.x, a.gy);
    return rectMask(v, blob, L, a.x, t.width - 1, a.gy) | rectMask(v, blob, L, 0, b.x, b.gy);   // a wrap over a row end: both pieces
}

}  // namespace ptstrip
