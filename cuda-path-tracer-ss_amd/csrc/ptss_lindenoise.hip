// ptss_lindenoise.hip — the kernels behind ptss_denoise_linear (include/ptss.h): the A-trous filter of the two linear
// films in linear light, guided by the film's measured variance. The arithmetic is csrc/ptlindn.h, shared with the host probe
// (ptss_probe_denoise_linear, the specification); this file only moves the data.
//
//   linDenoisePrepareKernel      film + moments + features -> plane 0 {c, v}, the packed feature rows {normal, depth} and the materials: a tap
//                                of a pass is then two 16-byte loads and one of 4 bytes, against a 16-byte and a 32-byte row of ptss_denoise.
//                                <Final>: levels = 0, the film's integer means written straight into the output film
//   linDenoiseStagedKernel<S>    one pass at spacing S = 1, 2 or 4. A workgroup of 32 x 8 pixels stages its tile and a halo of 2 S pixels
//                                (rows, feature rows, materials: 36 B a pixel; 15.2, 22.5 and 40.5 KiB) in LDS once and filters from there.
//                                The 3 x 3 of the variance and the depth slopes lie inside that halo (2 S >= 1): no further ring is staged.
//                                A wave's lanes read neighbouring 16-byte rows of one tile row (two tile rows per wave), which ds_read_b128
//                                serves without bank conflicts whatever the pitch, so the tile is not padded
//   linDenoisePassKernel         the same pass with every tap read from global memory, built like denoiseKernel: every spacing
// <Last>: the pass writes the output film (ptldn::finishRow) instead of a plane. Both forms call ptldn::filterPixel and give the same
// bytes; which spacing uses which is kStagedAt below, decided by measurement. No workgroup waits for another; no bit
// of ptss_launched_kernels.
#include <hip/hip_runtime.h>

#include "ptlindn.h"
#include "ptss_device.h"

namespace ptss {

using ptlin::u64;

constexpr int kLinDenoiseTileX = 32, kLinDenoiseTileY = 8;
constexpr int kLinDenoiseBlock = kLinDenoiseTileX * kLinDenoiseTileY;
constexpr int kLinDenoiseMaxStaged = 4;   // the largest spacing with a staged kernel

// The form per pass i (spacing 2^i) the library ships: true = staged. Spacings above kLinDenoiseMaxStaged have no staged form.
// Measured at 1080p (tools/denoise_linear_bench.py), a pass staged against the same pass from global memory, five
// interleaved pairs each: spacing 1 0.125 against 0.175 ms and spacing 2 0.111 against 0.163 ms, staged faster in every pair; spacing 4
// 0.174 against 0.167 ms, slower in every pair — 4.5 staged pixels per output pixel, and 40.5 KiB of LDS leave three workgroups a
// compute unit: the staging does not pay there. (That kernel stays compiled for the tests and the measurement.)
constexpr bool kStagedAt[ptldn::kMaxLevels] = {true, true, false, false, false, false};

__device__ __forceinline__ ptldn::Row rowOf(float4 r) { return ptldn::Row{ptv::v3(r.x, r.y, r.z), r.w}; }
__device__ __forceinline__ float4 packed(const ptldn::Row& r) { return float4{r.c.x, r.c.y, r.c.z, r.v}; }

__device__ __forceinline__ void storeFilmRow(ulonglong2* __restrict__ out, size_t p, const u64* o) {
    out[2 * p] = ulonglong2{o[0], o[1]};
    out[2 * p + 1] = ulonglong2{o[2], o[3]};
}

template <bool Splat, bool Final>
__global__ __launch_bounds__(kLinDenoiseBlock) void linDenoisePrepareKernel(const ulonglong2* __restrict__ film, const ulonglong2* __restrict__ moments,
                                                                            const float4* __restrict__ features, uint32_t n, ptldn::Rule R,
                                                                            float4* __restrict__ plane, float4* __restrict__ featureRows,
                                                                            int* __restrict__ materials, ulonglong2* __restrict__ out) {
    const uint32_t i = blockIdx.x * (uint32_t)kLinDenoiseBlock + threadIdx.x;
    if (i >= n) return;
    const size_t p = (size_t)i;
    const ulonglong2 rg = film[2 * p], bw = film[2 * p + 1];
    if constexpr (Final) {
        u64 o[4];
        ptldn::finishMeans(rg.x, rg.y, bw.x, bw.y, Splat, o);
        storeFilmRow(out, p, o);
    } else {
        const ulonglong2 m0 = moments[2 * p], m1 = moments[2 * p + 1];
        plane[p] = packed(ptldn::prepare(rg.x, rg.y, bw.x, bw.y, Splat, m0.x, m0.y, m1.x, m1.y, R));
        featureRows[p] = features[2 * p];
        materials[p] = reinterpret_cast<const int*>(features)[8 * p + 7];
    }
}

// what a pass does with its pixel's row
template <bool Last, bool Splat>
__device__ __forceinline__ void storePass(const ptldn::Row& row, size_t p, const ulonglong2* __restrict__ film, void* __restrict__ dst,
                                          const ptldn::Rule& R) {
    if constexpr (Last) {
        u64 o[4];
        ptldn::finishRow(row, film[2 * p + 1].y, Splat, R, o);
        storeFilmRow(static_cast<ulonglong2*>(dst), p, o);
    } else {
        static_cast<float4*>(dst)[p] = packed(row);
    }
}

template <bool Last, bool Splat>
__global__ __launch_bounds__(kLinDenoiseBlock) void linDenoisePassKernel(const float4* __restrict__ src, void* __restrict__ dst,
                                                                         const float4* __restrict__ featureRows, const int* __restrict__ materials,
                                                                         const ulonglong2* __restrict__ film, int width, int height, int tilesX,
                                                                         int step, ptldn::Rule R) {
    const int tileX = (int)(blockIdx.x % (unsigned)tilesX), tileY = (int)(blockIdx.x / (unsigned)tilesX);
    const int x = tileX * kLinDenoiseTileX + (int)(threadIdx.x % kLinDenoiseTileX);
    const int y = tileY * kLinDenoiseTileY + (int)(threadIdx.x / kLinDenoiseTileX);
    if (x >= width || y >= height) return;   // every access below is to pixel (x, y) or to a tap filterPixel has bounds-checked
    auto rowAt = [&](int qx, int qy) -> ptldn::Row { return rowOf(src[(size_t)qy * (size_t)width + (size_t)qx]); };
    auto featureAt = [&](int qx, int qy) -> ptdn::Feature {
        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
        const float4 f = featureRows[q];
        return ptdn::Feature{ptv::v3(f.x, f.y, f.z), f.w, materials[q]};
    };
    const ptldn::Row row = ptldn::filterPixel(x, y, width, height, step, R, rowAt, featureAt);
    storePass<Last, Splat>(row, (size_t)y * (size_t)width + (size_t)x, film, dst, R);
}

template <int S, bool Last, bool Splat>
__global__ __launch_bounds__(kLinDenoiseBlock) void linDenoiseStagedKernel(const float4* __restrict__ src, void* __restrict__ dst,
                                                                           const float4* __restrict__ featureRows, const int* __restrict__ materials,
                                                                           const ulonglong2* __restrict__ film, int width, int height, int tilesX,
                                                                           ptldn::Rule R) {
    constexpr int kHalo = 2 * S;
    constexpr int kW = kLinDenoiseTileX + 2 * kHalo, kH = kLinDenoiseTileY + 2 * kHalo;
    __shared__ float4 sRow[kW * kH];
    __shared__ float4 sFeature[kW * kH];
    __shared__ int sMaterial[kW * kH];
    const int tileX = (int)(blockIdx.x % (unsigned)tilesX), tileY = (int)(blockIdx.x / (unsigned)tilesX);
    const int x0 = tileX * kLinDenoiseTileX - kHalo, y0 = tileY * kLinDenoiseTileY - kHalo;   // the pixel of slot (0, 0)
    for (int slot = (int)threadIdx.x; slot < kW * kH; slot += kLinDenoiseBlock) {
        const int qx = x0 + slot % kW, qy = y0 + slot / kW;
        if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;   // a slot outside the frame is never read: filterPixel checks every tap
        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
        sRow[slot] = src[q];
        sFeature[slot] = featureRows[q];
        sMaterial[slot] = materials[q];
    }
    __syncthreads();
    const int x = tileX * kLinDenoiseTileX + (int)(threadIdx.x % kLinDenoiseTileX);
    const int y = tileY * kLinDenoiseTileY + (int)(threadIdx.x / kLinDenoiseTileX);
    if (x >= width || y >= height) return;
    // a tap lies within 2 S of (x, y) along each axis and (x, y) in the tile: its slot is inside the staged rectangle
    auto rowAt = [&](int qx, int qy) -> ptldn::Row { return rowOf(sRow[(qy - y0) * kW + (qx - x0)]); };
    auto featureAt = [&](int qx, int qy) -> ptdn::Feature {
        const int slot = (qy - y0) * kW + (qx - x0);
        const float4 f = sFeature[slot];
        return ptdn::Feature{ptv::v3(f.x, f.y, f.z), f.w, sMaterial[slot]};
    };
    const ptldn::Row row = ptldn::filterPixel(x, y, width, height, S, R, rowAt, featureAt);
    storePass<Last, Splat>(row, (size_t)y * (size_t)width + (size_t)x, film, dst, R);
}

using LinDenoisePassFn = void (*)(const float4*, void*, const float4*, const int*, const ulonglong2*, int, int, int, int, ptldn::Rule);
using LinDenoiseStagedFn = void (*)(const float4*, void*, const float4*, const int*, const ulonglong2*, int, int, int, ptldn::Rule);

template <int S>
static LinDenoiseStagedFn stagedKernelOf(bool last, bool splat) {
    return last ? (splat ? linDenoiseStagedKernel<S, true, true> : linDenoiseStagedKernel<S, true, false>) : linDenoiseStagedKernel<S, false, false>;
}

hipError_t launchLinearDenoise(hipStream_t st, const void* film, bool splat, int width, int height, const void* moments, const void* features,
                               const ptss_linear_params& params, const ptss_denoise_linear_params& denoise, int form, void* workspace, void* out,
                               unsigned long long* launches) {
    const ptldn::Rule R = ptldn::ruleOf(denoise, params);
    const size_t P = (size_t)width * (size_t)height;
    size_t off[4];
    ptldn::workspaceLayout(P, off);
    char* ws = static_cast<char*>(workspace);
    float4* plane[2] = {reinterpret_cast<float4*>(ws + off[0]), reinterpret_cast<float4*>(ws + off[1])};
    float4* featureRows = reinterpret_cast<float4*>(ws + off[2]);
    int* materials = reinterpret_cast<int*>(ws + off[3]);
    const ulonglong2* f = static_cast<const ulonglong2*>(film);
    unsigned long long launched = 0;
    hipError_t e = hipSuccess;
    auto after = [&]() {
        e = hipGetLastError();
        if (e == hipSuccess) ++launched;
        return e == hipSuccess;
    };
    const int L = denoise.levels;
    {
        const dim3 grid((unsigned)((P + kLinDenoiseBlock - 1) / kLinDenoiseBlock));
        using Fn = void (*)(const ulonglong2*, const ulonglong2*, const float4*, uint32_t, ptldn::Rule, float4*, float4*, int*, ulonglong2*);
        static constexpr Fn table[4] = {linDenoisePrepareKernel<false, false>, linDenoisePrepareKernel<false, true>,
                                        linDenoisePrepareKernel<true, false>, linDenoisePrepareKernel<true, true>};
        hipLaunchKernelGGL(table[(splat ? 2 : 0) + (L == 0 ? 1 : 0)], grid, dim3(kLinDenoiseBlock), 0, st, f, static_cast<const ulonglong2*>(moments),
                           static_cast<const float4*>(features), (uint32_t)P, R, plane[0], featureRows, materials, static_cast<ulonglong2*>(out));
    }
    bool ok = after();
    // the tiles of the frame as one row of workgroups (a frame 2^22 pixels high has more tile rows than a grid has in y); below 2^31 / 8
    const int tilesX = (width + kLinDenoiseTileX - 1) / kLinDenoiseTileX, tilesY = (height + kLinDenoiseTileY - 1) / kLinDenoiseTileY;
    const dim3 grid((unsigned)tilesX * (unsigned)tilesY);
    for (int i = 0; ok && i < L; ++i) {
        const bool last = i + 1 == L;
        const int step = 1 << i;
        const float4* src = plane[ptldn::sourcePlane(i)];
        void* dst = last ? out : static_cast<void*>(plane[1 - ptldn::sourcePlane(i)]);
        // form: 0 the measured table, 1 unstaged everywhere, 2 staged wherever a staged kernel exists, 4 + mask staged at pass k where
        // bit k of the mask is set (tests and measurements)
        const bool staged = step <= kLinDenoiseMaxStaged && (form == 2 || (form == 0 && kStagedAt[i]) || (form >= 4 && (((form - 4) >> i) & 1)));
        if (staged) {
            const LinDenoiseStagedFn fn = step == 1 ? stagedKernelOf<1>(last, splat) : (step == 2 ? stagedKernelOf<2>(last, splat) : stagedKernelOf<4>(last, splat));
            hipLaunchKernelGGL(fn, grid, dim3(kLinDenoiseBlock), 0, st, src, dst, featureRows, materials, f, width, height, tilesX, R);
        } else {
            const LinDenoisePassFn fn = last ? (splat ? linDenoisePassKernel<true, true> : linDenoisePassKernel<true, false>) : linDenoisePassKernel<false, false>;
            hipLaunchKernelGGL(fn, grid, dim3(kLinDenoiseBlock), 0, st, src, dst, featureRows, materials, f, width, height, tilesX, step, R);
        }
        ok = after();
    }
    launches[1] += launched;
    if (ok) ++launches[0];
    return e;
}

}  // namespace ptss
