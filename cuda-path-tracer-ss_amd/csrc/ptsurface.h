// ptsurface.h — rays that leave from points on the scene's own surfaces, and the gutter fill of a light map (ptss_generate_rays_surface,
// ptss_dilate_linear), written once for the gfx950 kernels (ptss_surface.hip) and for the host probes (host_capi.cpp
// ptss_probe_surface_rays, ptss_probe_dilate_linear; tests/test_surface_cpu.py). Everything is float32 built from ptmath.h operations in
// the order written here, compiled without contraction on both sides, so the two builds agree bit for bit: the host build of this header
// is the specification of the device's rays.
//
// A SURFACE POINT (ptss_surface_point) names a primitive by the caller's index (sphere k: k, triangle t: 0x40000000 | t) and a place
// (a, b) on it; bit 0 of its flags (PTSS_SURFACE_BACK) negates the normal, every other bit must be 0.
//
//   TRIANGLE   a, b are the weights w1, w2 of a ptss_ray_hit (w1 with vertex1, w2 with vertex2), accepted when a >= 0, b >= 0 and the
//              rounded float sum a + b <= 1 (NaN fails). With the image's rows v0, e1, e2 (packTriangles: e = v - v0, one subtraction)
//              and its vertex normals n0, n1, n2:
//                point = madd(e2, b, madd(e1, a, v0))                                   ptmotion.h's expression
//                w0 = 1 - (a + b);  n = normalize((n0 w0 + n1 a) + n2 b)                closestQuery's interpolation, then a normalize
//   SPHERE     a, b are unit fractions of longitude and latitude as on an equirect film, accepted when 0 <= a <= 1 and 0 <= b <= 1.
//              With the image's row {centre, r2} (r2 = radius * radius as the packer rounds it):
//                lon = (a - 0.5) (2 pi);  lat = (b - 0.5) pi;  sincos(lon) -> (sl, cl);  sincos(lat) -> (se, ce)
//                n = (sl ce, se, -(cl ce));  r = ptm::sqrt(r2);  point = madd(n, r, centre)
//   Then n = -n with PTSS_SURFACE_BACK. The point is the same on both sides.
//
// THE RAY of a point (ptss_surface_params.mode):
//   PTSS_SURFACE_NORMAL   v = n; no stream word is read or written (the jitter = 0 rule of ptss_generate_rays)
//   PTSS_SURFACE_COSINE   two uniforms u1, u2 of (0, 1] from the ray's stream, in that order, and the reference's Lambert sampler in
//                         scatter()'s order (CudaTracer.cu:536-541): azimuth = u1 * 2 * kPi (two products, left to right);
//                         y = ptm::sqrt(u2);  A = ptm::sqrt(1 - y * y);  sincos(azimuth) -> (sn, cs);  local = (A cs, y, A sn).
//                         The local vector is taken about n by an orthonormal basis made from n alone (Duff, Burgess, Christensen,
//                         Hery, Kensler, Liani, Villemin: "Building an Orthonormal Basis, Revisited", JCGT 6(1), 2017), not by the
//                         reference's rotateVectorToVector((0, 1, 0), n), whose quaternion is 0 / 0 at n = (0, -1, 0):
//                           s = copysign(1, n.z)   (the sign BIT of n.z: -0.0 gives -1);  q = -ptm::rcp(s + n.z)   (|s + n.z| in [1, 2])
//                           c = (n.x n.y) q
//                           t = (fma(s n.x, n.x q, 1),  s c,  -(s n.x))
//                           b = (c,  fma(n.y, n.y q, s),  -n.y)
//                           v = madd(b, A sn, madd(n, y, t * (A cs)))
//                         Every operand is finite for every unit n; local y = sqrt(u2) >= 2^-16.5 keeps dot(v, n) > 0.
//   Every ray: direction = normalize(v);  origin = point + kRayBump * n (scatter()'s Lambert bump, one product and one sum per
//   component);  tmax = maxDistance;  pad = 0.
// draws(mode) says how many uniforms a ray takes: 0 or 2.
//
// THE GUTTER FILL (dilateTexel): one pass over a width x height film of ptss_linear_entry into a SECOND film. A texel with samples > 0
// is copied. An empty one receives the field-by-field sum of those of its eight neighbours inside the film that hold samples, in the
// order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1): r, g, b added as 64-bit and samples, clamped as 32-bit unsigned integers,
// wrapping (ptlinear.h: sums wrap), so the order does not matter. The sum is the sample-weighted mean of the neighbours and an ordinary
// film row; a texel with no counted neighbour stays all zero.
#pragma once
#include "ptmath.h"

namespace ptsurf {
using namespace ptv;

constexpr float kTwoPi = 2 * ptm::kPi;
constexpr uint32_t kTriangleBit = 0x40000000u;   // ptss_surface_point::surface of triangle t: this | t (PTSS_SURFACE_TRIANGLE)

// the argument check ptss_generate_rays_surface and ptss_probe_surface_rays share; nullptr when the parameters are acceptable
inline const char* paramsError(const ptss_surface_params* p) {
    if (!p) return "surface params is null";
    if (p->structSize != (unsigned int)sizeof(ptss_surface_params)) return "structSize is not this library's sizeof(ptss_surface_params)";
    if (p->mode != PTSS_SURFACE_NORMAL && p->mode != PTSS_SURFACE_COSINE) return "unknown surface mode";
    if (!(p->maxDistance > 0.0f)) return "maxDistance must be positive (+inf allowed)";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

PTM_HD int draws(int mode) { return mode == PTSS_SURFACE_COSINE ? 2 : 0; }

PTM_HD bool flagsAccepted(uint32_t flags) { return (flags & ~(uint32_t)PTSS_SURFACE_BACK) == 0u; }
PTM_HD bool triangleAccepted(float a, float b) { return a >= 0.0f && b >= 0.0f && a + b <= 1.0f; }
PTM_HD bool sphereAccepted(float a, float b) { return a >= 0.0f && a <= 1.0f && b >= 0.0f && b <= 1.0f; }

struct Surfel {   // where a ray leaves from: the point and the unit normal on the side the flags name
    vec3 point, normal;
};

PTM_HD Surfel triangleSurfel(vec3 v0, vec3 e1, vec3 e2, vec3 n0, vec3 n1, vec3 n2, float a, float b, uint32_t flags) {
    Surfel s;
    s.point = madd(e2, b, madd(e1, a, v0));
    const float w0 = 1.0f - (a + b);
    const vec3 n = normalize((n0 * w0 + n1 * a) + n2 * b);
    s.normal = (flags & PTSS_SURFACE_BACK) ? -n : n;
    return s;
}

PTM_HD Surfel sphereSurfel(vec3 centre, float radius2, float a, float b, uint32_t flags) {
    const float lon = (a - 0.5f) * kTwoPi;
    const float lat = (b - 0.5f) * ptm::kPi;
    float sl, cl, se, ce;
    ptm::sincos(lon, sl, cl);
    ptm::sincos(lat, se, ce);
    const vec3 n = v3(sl * ce, se, -(cl * ce));
    Surfel s;
    s.point = madd(n, ptm::sqrt(radius2), centre);
    s.normal = (flags & PTSS_SURFACE_BACK) ? -n : n;
    return s;
}

// the local vector (lx, ly, lz), ly along n, about the unit vector n
PTM_HD vec3 aboutNormal(vec3 n, float lx, float ly, float lz) {
    const float s = ptm::u2f((ptm::f2u(n.z) & 0x80000000u) | 0x3f800000u);
    const float q = -ptm::rcp(s + n.z);
    const float c = (n.x * n.y) * q;
    const vec3 t = v3(ptm::fma(s * n.x, n.x * q, 1.0f), s * c, -(s * n.x));
    const vec3 b = v3(c, ptm::fma(n.y, n.y * q, s), -n.y);
    return madd(b, lz, madd(n, ly, t * lx));
}

// the ray of a surfel; u1, u2: the stream's draws in that order (not read in PTSS_SURFACE_NORMAL)
PTM_HD ptss_ray_query surfaceRay(const Surfel& s, int mode, float maxDistance, float u1, float u2) {
    vec3 v = s.normal;
    if (mode == PTSS_SURFACE_COSINE) {
        const float azimuth = u1 * 2 * ptm::kPi;
        const float y = ptm::sqrt(u2);
        const float A = ptm::sqrt(1 - y * y);
        float sn, cs;
        ptm::sincos(azimuth, sn, cs);
        v = aboutNormal(s.normal, A * cs, y, A * sn);
    }
    ptss_ray_query q;
    q.origin = s.point + ptm::kRayBump * s.normal;
    q.tmax = maxDistance;
    q.direction = normalize(v);
    q.pad = 0.0f;
    return q;
}

// the ptss_ray_hit a ray arriving at the surfel would report
PTM_HD ptss_ray_hit surfelHit(const Surfel& s, int materialIdx, int kind, int primitive, float a, float b) {
    ptss_ray_hit h;
    h.point = s.point;
    h.distance = 0.0f;
    h.normal = s.normal;
    h.materialIdx = materialIdx;
    h.kind = kind;
    h.primitive = primitive;
    h.w1 = kind == PTSS_HIT_TRIANGLE ? a : 0.0f;
    h.w2 = kind == PTSS_HIT_TRIANGLE ? b : 0.0f;
    return h;
}

// ---- the gutter fill ----
struct Texel {   // a ptss_linear_entry
    unsigned long long r, g, b;
    uint32_t samples, clamped;
};

PTM_HD const char* dilateSidesError(int width, int height) {
    if (width <= 0 || height <= 0) return "width and height must be positive";
    if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
    return nullptr;
}

// texel (x, y) of the output; at(x, y) -> the input's Texel, called for coordinates inside the film only
template <class At>
PTM_HD Texel dilateTexel(int x, int y, int width, int height, At at) {
    const Texel own = at(x, y);
    if (own.samples > 0u) return own;
    Texel o{0ull, 0ull, 0ull, 0u, 0u};
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = x + dx, ny = y + dy;
            if ((dx == 0 && dy == 0) || nx < 0 || ny < 0 || nx >= width || ny >= height) continue;
            const Texel e = at(nx, ny);
            if (e.samples > 0u) {
                o.r += e.r;
                o.g += e.g;
                o.b += e.b;
                o.samples += e.samples;
                o.clamped += e.clamped;
            }
        }
    return o;
}

// ---- the atlas (host only: ptss_surface_atlas, ptss_surface_atlas_blocks, ptss_main --bake) ----
// The texels of a light map over triangles[first .. first + count): triangle t gets a square block of side s = clamp(ceil(longestEdge
// * texelsPerUnit), minSide, maxSide) (a product that is not a number: minSide); blocks are shelf-packed left to right in the caller's
// order into atlasWidth columns, one empty texel between blocks and between shelves; the texels (i, j) of a block with i + j <= s - 1
// each get the point a = (3 i + 1) / (3 s), b = (3 j + 1) / (3 s): one float division each, a + b <= 1 - 1 / (3 s) before rounding and
// s <= 4096, so the rounded sum stays below 1. Returns 0, -1 for refused arguments, -3 for a range (PTSS_HOST_EINVAL, PTSS_HOST_ERANGE).
//
// atlasBlocks (ptss_surface_atlas_blocks) is the same walk continued over spheres[firstSphere .. firstSphere +
// numSpheres) on the same shelves: sphere k gets h = clamp(ceil(kPi * radius * texelsPerUnit), minSide, maxSide) rows (two products, left
// to right; not a number: minSide) and w = 2 h columns, and EVERY texel (i, j) of the block the point {k, a = (i + 0.5) / w,
// b = (j + 0.5) / h, 0} — sphereSurfel's longitude and latitude fractions, one float sum and one float division each — rows bottom up,
// after all triangle points. It also says where each block lies (ptss_surface_block; a primitive always gets one here, width >= 1).
// Refused beyond atlas' list: null spheres with numSpheres > 0 and 2 * maxSide > atlasWidth when numSpheres > 0 (-1); firstSphere +
// numSpheres at or above 2^30 (-3).
#if !defined(__HIP_DEVICE_COMPILE__)
inline int sideOf(float want, int minSide, int maxSide) {
    int s = minSide;
    if (want >= (float)maxSide) s = maxSide;
    else if (want > (float)minSide) s = (int)__builtin_ceilf(want);
    return s;
}

struct Shelves {   // the shelf walk: where the next block goes
    unsigned long long atlasWidth;
    unsigned long long x0 = 0, y0 = 0, shelf = 0;   // the next block's corner and the tallest block of the current shelf
    // the corner of a block of w x h texels, w <= atlasWidth; false: the atlas would reach 2^31 texels
    bool place(int w, int h, unsigned long long* bx, unsigned long long* by) {
        if (x0 + (unsigned long long)w > atlasWidth) {   // a new shelf, one empty row above the old one
            y0 += shelf + 1;
            x0 = 0;
            shelf = 0;
        }
        if ((y0 + (unsigned long long)h) * atlasWidth >= (1ull << 31)) return false;
        *bx = x0;
        *by = y0;
        if ((unsigned long long)h > shelf) shelf = (unsigned long long)h;
        x0 += (unsigned long long)w + 1;
        return true;
    }
};

inline int atlasBlocks(const ptss_triangle* triangles, size_t first, size_t count, const ptss_sphere* spheres, size_t firstSphere, size_t numSpheres,
                       float texelsPerUnit, int minSide, int maxSide, int atlasWidth, ptss_surface_block* blocksTri, ptss_surface_block* blocksSph,
                       ptss_surface_point* points, uint32_t* texels, size_t capacity, int* atlasHeight, size_t* numPoints) {
    if (!numPoints || (count > 0 && !triangles) || (numSpheres > 0 && !spheres)) return -1;
    if (!(texelsPerUnit > 0.0f && texelsPerUnit < ptm::inf())) return -1;
    if (minSide < 1 || maxSide < minSide || maxSide > 4096 || maxSide > atlasWidth) return -1;
    if (numSpheres > 0 && 2 * maxSide > atlasWidth) return -1;
    if (first >= ((size_t)1 << 30) || count > ((size_t)1 << 30) - first) return -3;
    if (firstSphere >= ((size_t)1 << 30) || numSpheres > ((size_t)1 << 30) - firstSphere) return -3;
    Shelves shelves{(unsigned long long)atlasWidth};
    unsigned long long x0, y0;
    size_t made = 0;
    for (size_t k = 0; k < count; ++k) {
        const ptss_triangle& t = triangles[first + k];
        const float e01 = length(t.vertex1 - t.vertex0), e02 = length(t.vertex2 - t.vertex0), e12 = length(t.vertex2 - t.vertex1);
        const int s = sideOf(ptm::max(ptm::max(e01, e02), e12) * texelsPerUnit, minSide, maxSide);
        if (!shelves.place(s, s, &x0, &y0)) return -3;
        if (blocksTri) blocksTri[k] = ptss_surface_block{(int)x0, (int)y0, s, s};
        for (int j = 0; j < s; ++j)
            for (int i = 0; i + j <= s - 1; ++i, ++made) {
                if (made >= capacity) continue;
                if (points)
                    points[made] = ptss_surface_point{(int)(kTriangleBit | (uint32_t)(first + k)), (float)(3 * i + 1) / (float)(3 * s),
                                                      (float)(3 * j + 1) / (float)(3 * s), 0u};
                if (texels) texels[made] = (uint32_t)((y0 + (unsigned long long)j) * (unsigned long long)atlasWidth + x0 + (unsigned long long)i);
            }
    }
    for (size_t k = 0; k < numSpheres; ++k) {
        const int h = sideOf(ptm::kPi * spheres[firstSphere + k].radius * texelsPerUnit, minSide, maxSide), w = 2 * h;
        if (!shelves.place(w, h, &x0, &y0)) return -3;
        if (blocksSph) blocksSph[k] = ptss_surface_block{(int)x0, (int)y0, w, h};
        for (int j = 0; j < h; ++j)
            for (int i = 0; i < w; ++i, ++made) {
                if (made >= capacity) continue;
                if (points) points[made] = ptss_surface_point{(int)(firstSphere + k), ((float)i + 0.5f) / (float)w, ((float)j + 0.5f) / (float)h, 0u};
                if (texels) texels[made] = (uint32_t)((y0 + (unsigned long long)j) * (unsigned long long)atlasWidth + x0 + (unsigned long long)i);
            }
    }
    if (atlasHeight) *atlasHeight = (int)(shelves.y0 + shelves.shelf);
    *numPoints = made;
    return 0;
}

inline int atlas(const ptss_triangle* triangles, size_t first, size_t count, float texelsPerUnit, int minSide, int maxSide, int atlasWidth,
                 ptss_surface_point* points, uint32_t* texels, size_t capacity, int* atlasHeight, size_t* numPoints) {
    return atlasBlocks(triangles, first, count, nullptr, 0, 0, texelsPerUnit, minSide, maxSide, atlasWidth, nullptr, nullptr, points, texels, capacity,
                       atlasHeight, numPoints);
}
#endif

}  // namespace ptsurf
