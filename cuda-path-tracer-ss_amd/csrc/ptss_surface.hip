// ptss_surface.hip — the kernels behind ptss_generate_rays_surface and ptss_dilate_linear (include/ptss.h): rays that
// leave from points on the scene's own surfaces, made from the scene image, and the gutter fill of a baked linear film. The arithmetic
// is csrc/ptsurface.h, shared with the host probes (ptss_probe_surface_rays, ptss_probe_dilate_linear: the specification); this file
// only moves the data.
//
// surfaceRayKernel is a streaming kernel like filmRayKernel: one lane per ray, filmRayKernel's block size, nothing staged in LDS — the
// gathers are per lane. Per ray one 16-byte point row, one word of a position table where the image stores its primitives in another
// order (classed and mesh images: offTriPos; the many-sphere image: offSpherePos), six 16-byte rows of a triangle (v0, e1, e2, n0, n1,
// n2) or one row and one word of a sphere, six stream words in and out (PTSS_SURFACE_COSINE only), and two or five 16-byte row stores.
// Every table is read through the global pointer: a mesh image keeps its triangle tables beyond ldsVec4 anyway (closestQuery's `td`).
// Every gather index — the caller's primitive number, then the stored position read from the image — is held against the image's
// counts BEFORE an address is formed from it: a bad point is counted (one atomic per wave, ptfilm.h countDropped), never dereferenced.
//
// dilateKernel: one thread per texel, workgroups of 32 x 8 texels laid out as one row of workgroups. Two forms with the same bytes:
//   <kStaged = false>   the texel's own row pair and, for an empty texel, the row pairs of its up to eight neighbours from global memory
//   <kStaged = true>    the 34 x 10 texels of the tile and a ring of one staged in LDS (two 16-byte rows a slot, 10.6 KiB a workgroup;
//                       a slot outside the film holds zeros and is never asked for), then the same nine reads from LDS
// Which one ships is kDilateStaged below. No workgroup waits for another; no bit of ptss_launched_kernels.
#include <hip/hip_runtime.h>

#include "ptss_device.h"
#include "ptsurface.h"
#include "ptfilm.h"

namespace ptss {

constexpr int kSurfaceBlock = 256;   // filmRayKernel's

struct SurfaceImage {   // what surfaceRayKernel reads of a SceneLayout; offsets in rows, -1: the caller's order is the stored one
    int numSpheres, sphereRows, numTriangles;
    int offSphere, offSphereMat, offSpherePos;
    int offTri, offTriNormal, offTriPos;
};

template <bool kSurfels>
__global__ __launch_bounds__(kSurfaceBlock) void surfaceRayKernel(const float4* __restrict__ blob, SurfaceImage I, int mode, float maxDistance,
                                                                  const uint4* __restrict__ points, uint32_t numPoints, uint32_t firstPoint,
                                                                  const uint32_t* __restrict__ index, uint32_t n, uint32_t* __restrict__ rng,
                                                                  float4* __restrict__ rays, float4* __restrict__ surfels,
                                                                  unsigned long long* __restrict__ rejected) {
    const uint32_t i = blockIdx.x * kSurfaceBlock + threadIdx.x;
    const bool inBatch = i < n;
    uint32_t p = 0;
    if (inBatch) p = index ? index[i] : firstPoint + i;
    bool ok = inBatch && p < numPoints;
    uint4 pt = uint4{0u, 0u, 0u, 0u};
    if (ok) pt = points[p];
    const float a = asF(pt.y), b = asF(pt.z);
    const bool triangle = (pt.x & ptsurf::kTriangleBit) != 0u;
    const uint32_t prim = pt.x & ~ptsurf::kTriangleBit;
    ok = ok && (int)pt.x >= 0 && ptsurf::flagsAccepted(pt.w);
    ok = ok && (triangle ? prim < (uint32_t)I.numTriangles && ptsurf::triangleAccepted(a, b)
                         : prim < (uint32_t)I.numSpheres && ptsurf::sphereAccepted(a, b));
    uint32_t pos = prim;   // where the image stores the primitive
    if (ok) {
        const int table = triangle ? I.offTriPos : I.offSpherePos;
        if (table >= 0) pos = reinterpret_cast<const uint32_t*>(blob + table)[prim];
        ok = pos < (uint32_t)(triangle ? I.numTriangles : I.sphereRows);
    }
    countDropped(inBatch && !ok, rejected);
    if (!ok) return;
    ptsurf::Surfel s;
    int materialIdx;
    if (triangle) {
        const float4* t = blob + I.offTri + 3 * (size_t)pos;
        const float4* nn = blob + I.offTriNormal + 3 * (size_t)pos;
        const float4 r0 = t[0], r1 = t[1], r2 = t[2], n0 = nn[0], n1 = nn[1], n2 = nn[2];
        s = ptsurf::triangleSurfel(xyz(r0), xyz(r1), xyz(r2), xyz(n0), xyz(n1), xyz(n2), a, b, pt.w);
        materialIdx = (int)asU(r0.w);
    } else {
        const float4 row = blob[I.offSphere + (size_t)pos];
        s = ptsurf::sphereSurfel(xyz(row), row.w, a, b, pt.w);
        materialIdx = reinterpret_cast<const int*>(blob + I.offSphereMat)[pos];
    }
    float u1 = 0.0f, u2 = 0.0f;
    if (mode == PTSS_SURFACE_COSINE) {   // (wave-uniform: a kernel argument)
        uint32_t* w = rng + 6 * (size_t)i;
        ptrng::State st;
#pragma unroll
        for (int k = 0; k < 5; ++k) st.v[k] = w[k];
        st.d = w[5];
        u1 = ptrng::uniform(st);
        u2 = ptrng::uniform(st);
#pragma unroll
        for (int k = 0; k < 5; ++k) w[k] = st.v[k];
        w[5] = st.d;
    }
    const ptss_ray_query q = ptsurf::surfaceRay(s, mode, maxDistance, u1, u2);
    rays[2 * (size_t)i] = float4{q.origin.x, q.origin.y, q.origin.z, q.tmax};
    rays[2 * (size_t)i + 1] = float4{q.direction.x, q.direction.y, q.direction.z, q.pad};
    if constexpr (kSurfels) {
        const ptss_ray_hit h = ptsurf::surfelHit(s, materialIdx, triangle ? PTSS_HIT_TRIANGLE : PTSS_HIT_SPHERE, (int)prim, a, b);
        float4* o = surfels + 3 * (size_t)i;
        o[0] = float4{h.point.x, h.point.y, h.point.z, h.distance};
        o[1] = float4{h.normal.x, h.normal.y, h.normal.z, asF((uint32_t)h.materialIdx)};
        o[2] = float4{asF((uint32_t)h.kind), asF((uint32_t)h.primitive), h.w1, h.w2};
    }
}

hipError_t launchSurfaceRays(hipStream_t st, const float4* sceneBlob, const SceneLayout& L, const ptss_surface_params& params, const void* points,
                             uint32_t numPoints, uint32_t firstPoint, const uint32_t* index, uint32_t n, void* rng, void* rays, void* surfels,
                             unsigned long long* rejected, unsigned long long* launches) {
    SurfaceImage I;
    I.numSpheres = L.numSpheres;
    I.sphereRows = L.accelSpheres ? L.numChunks * kChunkSpheres : L.numSpheres;
    I.numTriangles = L.numTriangles;
    I.offSphere = L.offSphere;
    I.offSphereMat = L.offSphereMat;
    I.offSpherePos = L.accelSpheres ? L.offSpherePos : -1;
    I.offTri = L.offTri;
    I.offTriNormal = L.offTriNormal;
    I.offTriPos = (meshImage(L) || L.triClassed) ? L.offTriPos : -1;
    const dim3 grid(filmBlocksFor(n, kSurfaceBlock)), block(kSurfaceBlock);
    const auto kernel = surfels ? surfaceRayKernel<true> : surfaceRayKernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, sceneBlob, I, params.mode, params.maxDistance, static_cast<const uint4*>(points), numPoints,
                       firstPoint, index, n, static_cast<uint32_t*>(rng), static_cast<float4*>(rays), static_cast<float4*>(surfels), rejected);
    return counted(launches);
}

// ---- the gutter fill ----
constexpr int kDilateTileX = 32, kDilateTileY = 8;
constexpr int kDilateBlock = kDilateTileX * kDilateTileY;
constexpr int kDilateSlotsX = kDilateTileX + 2, kDilateSlotsY = kDilateTileY + 2;

// The form the library ships: staged. Measured at 2048 x 2048 on a film with 60 % of its texels filled (tools/surface_bench.py;
// profiles/surface/), five interleaved pairs of windows: staged 0.048 ms against 0.083 ms from global memory, faster in
// every pair (a device copy of the film in and out: 0.031 ms). The form without LDS lost and stays compiled for the tests and the tool.
constexpr bool kDilateStaged = true;

__device__ __forceinline__ ptsurf::Texel texelOf(ulonglong2 rg, ulonglong2 bw) {
    return ptsurf::Texel{rg.x, rg.y, bw.x, (uint32_t)bw.y, (uint32_t)(bw.y >> 32)};
}

template <bool kStaged>
__global__ __launch_bounds__(kDilateBlock) void dilateKernel(const ulonglong2* __restrict__ film, ulonglong2* __restrict__ out, int width, int height,
                                                             int tilesX) {
    constexpr int kSlots = kStaged ? kDilateSlotsX * kDilateSlotsY : 1;
    __shared__ ulonglong2 sRG[kSlots];
    __shared__ ulonglong2 sBW[kSlots];
    const int tileX = (int)(blockIdx.x % (unsigned)tilesX), tileY = (int)(blockIdx.x / (unsigned)tilesX);
    const int X0 = tileX * kDilateTileX, Y0 = tileY * kDilateTileY;
    if constexpr (kStaged) {
        for (int slot = (int)threadIdx.x; slot < kSlots; slot += kDilateBlock) {
            const int sx = X0 - 1 + slot % kDilateSlotsX, sy = Y0 - 1 + slot / kDilateSlotsX;
            ulonglong2 rg = ulonglong2{0ull, 0ull}, bw = ulonglong2{0ull, 0ull};
            if (sx >= 0 && sy >= 0 && sx < width && sy < height) {   // the only global reads of this form: inside the film
                const size_t q = (size_t)sy * (size_t)width + (size_t)sx;
                rg = film[2 * q];
                bw = film[2 * q + 1];
            }
            sRG[slot] = rg;
            sBW[slot] = bw;
        }
        __syncthreads();
    }
    const int x = X0 + (int)(threadIdx.x % kDilateTileX), y = Y0 + (int)(threadIdx.x / kDilateTileX);
    if (x >= width || y >= height) return;
    // dilateTexel asks for coordinates inside the film only, at most one texel away from (x, y): inside the staged rectangle
    auto at = [&](int tx, int ty) -> ptsurf::Texel {
        if constexpr (kStaged) {
            const int slot = (ty - Y0 + 1) * kDilateSlotsX + (tx - X0 + 1);
            return texelOf(sRG[slot], sBW[slot]);
        } else {
            const size_t q = (size_t)ty * (size_t)width + (size_t)tx;
            return texelOf(film[2 * q], film[2 * q + 1]);
        }
    };
    const ptsurf::Texel t = ptsurf::dilateTexel(x, y, width, height, at);
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    out[2 * p] = ulonglong2{t.r, t.g};
    out[2 * p + 1] = ulonglong2{t.b, (unsigned long long)t.samples | ((unsigned long long)t.clamped << 32)};
}

hipError_t launchDilateLinear(hipStream_t st, const void* film, int width, int height, int form, void* out, unsigned long long* launches) {
    const bool staged = form == 2 || (form == 0 && kDilateStaged);   // form: 0 the shipped one, 1 global memory, 2 staged
    // the tiles as one row of workgroups: a film of W H < 2^31 texels has at most (W / 32 + 1) (H / 8 + 1) <= W H / 256 + W / 32 + H / 8 + 1
    // < 2^23 + 2^26 + 2^28 + 1 of them
    const unsigned tilesX = ((unsigned)width + kDilateTileX - 1) / kDilateTileX, tilesY = ((unsigned)height + kDilateTileY - 1) / kDilateTileY;
    const dim3 grid(tilesX * tilesY);
    hipLaunchKernelGGL(staged ? dilateKernel<true> : dilateKernel<false>, grid, dim3(kDilateBlock), 0, st, static_cast<const ulonglong2*>(film),
                       static_cast<ulonglong2*>(out), width, height, (int)tilesX);
    return counted(launches);
}

}  // namespace ptss
