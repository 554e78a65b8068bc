// ptss_film.hip — the kernels behind ptss_generate_rays, ptss_accumulate_paths and ptss_ray_features (include/ptss.h):
// the film of a path query. Eye rays made on the device from the caller's streams (csrc/ptcamera.h: pinhole, thin lens, equirectangular),
// finished samples accumulated per film pixel as writeToPixelsKernel accumulates them (CudaTracer.cu:63-104; ptshade.h finishPath), and
// the first-hit feature row of arbitrary rays. Like ptss_paths.hip this file has its own copy of closestQuery (pthit.h), so a feature
// row here is made by the operations of featureKernel.
//
// filmRayKernel and the accumulate kernels are streaming kernels: one lane per ray, no LDS, nothing staged. A ray's stream is six
// 4-byte words at a 4-byte aligned address (ptss_path_rng), read and written as pathQueryKernel reads and writes them.
#include "ptss_device.h"
#include "ptcamera.h"
#include "ptfilm.h"
#include "ptquant.h"
#include "pthit.h"

namespace ptss {

constexpr int kFilmBlock = 256;

// ptss_generate_rays: ray i = the eye ray of film pixel p = index ? index[i] : firstPixel + i, from stream rng[i], which is stored
// back advanced by the model's draws. p >= filmPixels: nothing is written (ray and stream stay as they are), the entry is counted.
// kPositions (ptss_generate_rays_positions): positions[i] = the sample's place on the film (ptcam::samplePosition), {NaN, NaN} for a
// dropped entry.
template <bool kPositions>
__device__ __forceinline__ void filmRayBody(const ptcam::Film& F, uint32_t filmPixels, uint32_t firstPixel, const uint32_t* __restrict__ index,
                                            uint32_t n, uint32_t* __restrict__ rng, float4* __restrict__ rays, float2* __restrict__ positions,
                                            unsigned long long* __restrict__ rejected) {
    const uint32_t i = blockIdx.x * kFilmBlock + threadIdx.x;
    const bool inBatch = i < n;
    uint32_t p = 0;
    if (inBatch) p = index ? index[i] : firstPixel + i;
    const bool ok = inBatch && p < filmPixels;
    if (index) countDropped(inBatch && !ok, rejected);   // (without an index the caller has checked the range)
    if constexpr (kPositions) {
        if (inBatch && !ok) positions[i] = float2{ptm::qnan(), ptm::qnan()};
    }
    if (!ok) return;
    float jx = 0.5f, jy = 0.5f, u1 = 0.0f, u2 = 0.0f;
    if (F.jitter) {
        uint32_t* s = rng + 6 * (size_t)i;
        ptrng::State st;
#pragma unroll
        for (int w = 0; w < 5; ++w) st.v[w] = s[w];
        st.d = s[5];
        jx = ptrng::uniform(st);
        jy = ptrng::uniform(st);
        if (F.kind == PTSS_FILM_THIN_LENS) {
            u1 = ptrng::uniform(st);
            u2 = ptrng::uniform(st);
        }
#pragma unroll
        for (int w = 0; w < 5; ++w) s[w] = st.v[w];
        s[5] = st.d;
    }
    const int x = (int)(p % (uint32_t)F.width), y = (int)(p / (uint32_t)F.width);
    const ptss_ray_query q = ptcam::filmRay(F, x, y, jx, jy, u1, u2);
    rays[2 * (size_t)i] = float4{q.origin.x, q.origin.y, q.origin.z, q.tmax};
    rays[2 * (size_t)i + 1] = float4{q.direction.x, q.direction.y, q.direction.z, q.pad};
    if constexpr (kPositions) {
        float X, Y;
        ptcam::samplePosition(x, y, jx, jy, X, Y);
        positions[i] = float2{X, Y};
    }
}

__global__ __launch_bounds__(kFilmBlock) void filmRayKernel(ptcam::Film F, uint32_t filmPixels, uint32_t firstPixel,
                                                            const uint32_t* __restrict__ index, uint32_t n, uint32_t* __restrict__ rng,
                                                            float4* __restrict__ rays, unsigned long long* __restrict__ rejected) {
    filmRayBody<false>(F, filmPixels, firstPixel, index, n, rng, rays, nullptr, rejected);
}

__global__ __launch_bounds__(kFilmBlock) void filmRayPositionsKernel(ptcam::Film F, uint32_t filmPixels, uint32_t firstPixel,
                                                                     const uint32_t* __restrict__ index, uint32_t n, uint32_t* __restrict__ rng,
                                                                     float4* __restrict__ rays, float2* __restrict__ positions,
                                                                     unsigned long long* __restrict__ rejected) {
    filmRayBody<true>(F, filmPixels, firstPixel, index, n, rng, rays, positions, rejected);
}

// ptss_accumulate_paths without an index: ray i belongs to pixel firstPixel + i alone — finishPath's read-modify-write (S = 1)
__global__ __launch_bounds__(kFilmBlock) void filmAccumulateKernel(const float4* __restrict__ results, uint32_t firstPixel, uint32_t n,
                                                                   uint4* __restrict__ film, ptss_uchar4* __restrict__ pixels,
                                                                   float4* __restrict__ history, const float* __restrict__ quantT) {
    const uint32_t i = blockIdx.x * kFilmBlock + threadIdx.x;
    if (i >= n) return;
    const float4 r = results[i];
    const uint32_t p = firstPixel + i;
    uint4 e = film[p];
    e.x += ptq::quantize_fast(r.x, quantT);
    e.y += ptq::quantize_fast(r.y, quantT);
    e.z += ptq::quantize_fast(r.z, quantT);
    e.w += 1u;
    film[p] = e;
    resolveEntry(e, p, pixels, history);
}

// ... with an index: several rays of a launch may belong to one pixel, so the sums are integer atomics (order-free, exact); the
// touched pixels are resolved by filmResolveKernel, launched behind this kernel
__global__ __launch_bounds__(kFilmBlock) void filmScatterKernel(const float4* __restrict__ results, const uint32_t* __restrict__ index, uint32_t n,
                                                                uint32_t* __restrict__ film, uint32_t filmPixels,
                                                                const float* __restrict__ quantT, unsigned long long* __restrict__ rejected) {
    const uint32_t i = blockIdx.x * kFilmBlock + threadIdx.x;
    const bool inBatch = i < n;
    const uint32_t p = inBatch ? index[i] : 0u;
    const bool ok = inBatch && p < filmPixels;
    countDropped(inBatch && !ok, rejected);
    if (!ok) return;
    const float4 r = results[i];
    uint32_t* e = film + 4 * (size_t)p;
    atomicAdd(e + 0, ptq::quantize_fast(r.x, quantT));
    atomicAdd(e + 1, ptq::quantize_fast(r.y, quantT));
    atomicAdd(e + 2, ptq::quantize_fast(r.z, quantT));
    atomicAdd(e + 3, 1u);
}

// every entry of the index resolves its pixel; entries that share a pixel store the same bytes
__global__ __launch_bounds__(kFilmBlock) void filmResolveKernel(const uint32_t* __restrict__ index, uint32_t n, const uint4* __restrict__ film,
                                                                uint32_t filmPixels, ptss_uchar4* __restrict__ pixels,
                                                                float4* __restrict__ history) {
    const uint32_t i = blockIdx.x * kFilmBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = index[i];
    if (p >= filmPixels) return;
    resolveEntry(film[p], p, pixels, history);
}

// ptss_ray_features: featureKernel's body (ptss_kernels.hip) over the caller's rays — closestQuery with tmax = +inf, the hit's normal,
// distance and material index, that material's diffuse colour; a miss: closestQuery's miss row and the scene's default colour
template <bool kSceneInLds>
__global__ __launch_bounds__(kBlock) void rayFeatureKernel(const float4* __restrict__ sceneBlob, SceneLayout L, const float4* __restrict__ rays,
                                                            vec3 defaultColor, float4* __restrict__ out, uint32_t n) {
    extern __shared__ __attribute__((aligned(256))) float4 lds[];
    const float4* sc;
    if constexpr (kSceneInLds) {
        for (int k = threadIdx.x; k < L.ldsVec4; k += kBlock) lds[k] = sceneBlob[k];
        __syncthreads();
        sc = lds;
    } else {
        sc = sceneBlob;
    }
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        const bool live = i < n;
        vec3 o = v3(0, 0, 0), d = v3(0, 0, 0);
        if (live) {
            o = xyz(rays[2 * (size_t)i]);
            d = xyz(rays[2 * (size_t)i + 1]);
        }
        const QueryHit q = closestQuery(sc, sceneBlob, L, o, d, ptm::inf(), live);
        if (live) {
            vec3 albedo = defaultColor;
            if (q.kind != 0) albedo = xyz(loadRow16(sc + L.offMaterial + 5 * q.materialIdx));
            float4* f = out + 2 * (size_t)i;
            f[0] = float4{q.normal.x, q.normal.y, q.normal.z, q.dist};
            f[1] = float4{albedo.x, albedo.y, albedo.z, asF((uint32_t)q.materialIdx)};
        }
    }
}

hipError_t launchFilmRays(hipStream_t st, const ptcam::Film& film, uint32_t firstPixel, const uint32_t* index, uint32_t n, void* rng, void* rays,
                          void* positions, unsigned long long* rejected, unsigned long long* launches) {
    const dim3 grid(filmBlocksFor(n, kFilmBlock)), block(kFilmBlock);
    const uint32_t filmPixels = (uint32_t)film.width * (uint32_t)film.height;
    if (!positions)
        hipLaunchKernelGGL(filmRayKernel, grid, block, 0, st, film, filmPixels, firstPixel, index, n, static_cast<uint32_t*>(rng),
                           static_cast<float4*>(rays), rejected);
    else
        hipLaunchKernelGGL(filmRayPositionsKernel, grid, block, 0, st, film, filmPixels, firstPixel, index, n, static_cast<uint32_t*>(rng),
                           static_cast<float4*>(rays), static_cast<float2*>(positions), rejected);
    return counted(launches);
}

hipError_t launchFilmAccumulate(hipStream_t st, const void* results, const uint32_t* index, uint32_t firstPixel, uint32_t n, void* film,
                                uint32_t filmPixels, ptss_uchar4* pixels, void* history, const float* quantTable, unsigned long long* rejected,
                                unsigned long long* launches) {
    const dim3 grid(filmBlocksFor(n, kFilmBlock)), block(kFilmBlock);
    if (!index) {
        hipLaunchKernelGGL(filmAccumulateKernel, grid, block, 0, st, static_cast<const float4*>(results), firstPixel, n, static_cast<uint4*>(film),
                           pixels, static_cast<float4*>(history), quantTable);
    } else {
        hipLaunchKernelGGL(filmScatterKernel, grid, block, 0, st, static_cast<const float4*>(results), index, n, static_cast<uint32_t*>(film),
                           filmPixels, quantTable, rejected);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (pixels || history)
            hipLaunchKernelGGL(filmResolveKernel, grid, block, 0, st, index, n, static_cast<const uint4*>(film), filmPixels, pixels,
                               static_cast<float4*>(history));
    }
    return counted(launches);
}

hipError_t launchRayFeatures(hipStream_t st, const float4* sceneBlob, SceneLayout layout, bool sceneInLds, const void* rays,
                             ptss_vec3 defaultColor, void* out, uint32_t n, int maxBlocks, unsigned long long* launches) {
    unsigned blocks = filmBlocksFor(n, kBlock);
    if (maxBlocks > 0 && blocks > (unsigned)maxBlocks) blocks = (unsigned)maxBlocks;
    const size_t lds = sceneInLds ? (size_t)layout.ldsVec4 * sizeof(float4) : 0;
    const auto kernel = sceneInLds ? rayFeatureKernel<true> : rayFeatureKernel<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, st, sceneBlob, layout, static_cast<const float4*>(rays), defaultColor,
                       static_cast<float4*>(out), n);
    return counted(launches);
}

}  // namespace ptss
