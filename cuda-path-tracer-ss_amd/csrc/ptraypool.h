// ptraypool.h — layer 1 of the device code of ptss_kernels.hip: where a pixel and a ray live. Pixel order of a tile (locate),
// a ray in registers (RayRegs: the reference's Ray, RenderStructs.h, plus its XORWOW state), and the addressing, loads and
// stores of the ray pools (ptss_device.h "ray pools"), plain or past the L1 (kCoherent). Restates no reference arithmetic.
#pragma once
#include "ptlocate.h"
#include "ptss_device.h"
#include "ptwave.h"

namespace ptss {
namespace {

struct PixelCoord {
    int x, gy;
    uint32_t globalIndex;
};

__device__ __forceinline__ PixelCoord locate(const TileMap& t, uint32_t local) {
    const ptloc::Coord c = ptloc::locate(t.width, t.rank, t.world, t.bandRows, local);
    return PixelCoord{c.x, c.gy, c.globalIndex};
}
// The same for a wave whose lanes hold the consecutive local pixels first, first + 1, ... (bounce 0): the divisions once, on
// wave-uniform values (`first` must be wave-uniform: scalar registers), then an add, a compare and three selects per lane
// (ptlocate.h). A strip that crosses more than one row end (width < 64) takes locate() per lane; the choice is wave-uniform.
__device__ __forceinline__ ptloc::WaveOrigin locateWave(const TileMap& t, uint32_t first) {
    return ptloc::waveOrigin(t.width, t.rank, t.world, t.bandRows, first);
}
__device__ __forceinline__ PixelCoord locateLane(const TileMap& t, const ptloc::WaveOrigin& w, uint32_t first, uint32_t lane) {
    if (!w.oneWrap) return locate(t, first + lane);
    const ptloc::Coord c = ptloc::laneCoord(w, t.width, lane);
    return PixelCoord{c.x, c.gy, c.globalIndex};
}

// Ray::pixelOffset as carried by a ray: local pixel in the low 26 bits, sample lane (0..S-1, S <= 64) above.
// S = cfg.samplesPerPass independent random streams per pixel are traced per pass (1 = the reference).
constexpr uint32_t kLaneShift = 26;
constexpr uint32_t kPixMask = (1u << kLaneShift) - 1u;
__device__ __forceinline__ uint32_t pixOf(uint32_t packed) { return packed & kPixMask; }
__device__ __forceinline__ uint32_t laneOf(uint32_t packed) { return packed >> kLaneShift; }

struct RayRegs {
    vec3 o, d, L0, T;
    uint32_t pix;
    ptrng::State rng;
    bool active;
};

// ---- Ray pool addressing (ptss_device.h "ray pools"): a shard's region is a row of TILE BLOCKS, one per kBlock rays, each
// holding the kRayPlanes planes of its rays back to back: word (tile t, plane p, lane w) sits at (t * kRayPlanes + p) *
// kBlock + w. A tile of a workgroup is one block: its base is wave-uniform (scalar registers), the lane offset is
// threadIdx.x and the plane offset a compile-time constant, so a plane access needs no vector address arithmetic at all
// (the plane-major layout of round 1 spent a v_add_u32 + v_lshl_add_u64 per plane — 38 per tile, and both are half-rate
// instructions on gfx950: tools/microbench/vgpr_banks.hip). Survivors are stored at region slot `slot`: block
// slot / kBlock, lane slot % kBlock — one multiply-add per ray. Every access is still a 256-B contiguous wave transaction.
__device__ __forceinline__ const float* tileBlock(const float* __restrict__ region, uint32_t firstSlot /* multiple of kBlock */) {
    return region + (size_t)(firstSlot / kBlock) * (kRayPlanes * kBlock);
}
__device__ __forceinline__ uint32_t slotWord(uint32_t slot) {  // word offset of (slot, plane 0) inside the region
    return (slot / kBlock) * (uint32_t)(kRayPlanes * kBlock) + (slot % kBlock);
}

// One word of a block: scalar base + (32-bit lane byte offset, zero-extended) + compile-time plane offset — the form
// global_load/store take as `saddr + voffset + imm` (no 64-bit vector address pair per group of planes).
// kCoherent (the one-launch-per-frame kernel, frameKernel): the word was written, or will be read, by ANOTHER workgroup of the
// same launch — relaxed agent-scope accesses (global_load / global_store ... sc1: past the CU's L1, written through), the
// payload half of the sc1 hand-off of MI355X_MICROARCH.md "Workgroup dispatch, XCD placement & inter-workgroup visibility".
template <bool kCoherent = false>
__device__ __forceinline__ float ldPlane(const float* __restrict__ block, uint32_t laneBytes, int plane) {
    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(block) + (size_t)laneBytes + (size_t)plane * (kBlock * sizeof(float)));
    if constexpr (kCoherent) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}
template <bool kCoherent = false>
__device__ __forceinline__ void stPlane(float* __restrict__ region, uint32_t wordBytes, int plane, float v) {
    float* p = reinterpret_cast<float*>(reinterpret_cast<char*>(region) + (size_t)wordBytes + (size_t)plane * (kBlock * sizeof(float)));
    if constexpr (kCoherent) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// A tile fetches a ray's planes in the order it needs them, so that no plane occupies registers before
// its consumer runs: origin + direction for the closest-hit loops, the XORWOW state for the light samples, radiance /
// throughput / pixel for the update at the end. `block` = the tile's block (wave-uniform), w = the ray's lane in it.
template <bool kCoherent = false>
__device__ __forceinline__ void loadRayGeometry(const float* __restrict__ block, uint32_t w, RayRegs& r) {
    const uint32_t b = w * 4u;
    r.o = vec3{ldPlane<kCoherent>(block, b, kOx), ldPlane<kCoherent>(block, b, kOy), ldPlane<kCoherent>(block, b, kOz)};
    r.d = vec3{ldPlane<kCoherent>(block, b, kDx), ldPlane<kCoherent>(block, b, kDy), ldPlane<kCoherent>(block, b, kDz)};
    r.active = true;
}
template <bool kCoherent = false>
__device__ __forceinline__ void loadRayRng(const float* __restrict__ block, uint32_t w, RayRegs& r) {
    const uint32_t b = w * 4u;
    r.rng.v[0] = asU(ldPlane<kCoherent>(block, b, kR0));
    r.rng.v[1] = asU(ldPlane<kCoherent>(block, b, kR1));
    r.rng.v[2] = asU(ldPlane<kCoherent>(block, b, kR2));
    r.rng.v[3] = asU(ldPlane<kCoherent>(block, b, kR3));
    r.rng.v[4] = asU(ldPlane<kCoherent>(block, b, kR4));
    r.rng.d = asU(ldPlane<kCoherent>(block, b, kRd));
}
template <bool kCoherent = false>
__device__ __forceinline__ void loadRayRadiance(const float* __restrict__ block, uint32_t w, RayRegs& r) {
    const uint32_t b = w * 4u;
    r.L0 = vec3{ldPlane<kCoherent>(block, b, kL0x), ldPlane<kCoherent>(block, b, kL0y), ldPlane<kCoherent>(block, b, kL0z)};
    r.T = vec3{ldPlane<kCoherent>(block, b, kTx), ldPlane<kCoherent>(block, b, kTy), ldPlane<kCoherent>(block, b, kTz)};
    r.pix = asU(ldPlane<kCoherent>(block, b, kPix));
}
template <bool kCoherent = false>
__device__ __forceinline__ void loadRay(const float* __restrict__ block, uint32_t w, RayRegs& r) {
    loadRayGeometry<kCoherent>(block, w, r);
    loadRayRng<kCoherent>(block, w, r);
    loadRayRadiance<kCoherent>(block, w, r);
}

// the ray goes to region slot `slot` (its word in plane 0 of its block: slotWord)
template <bool kCoherent = false>
__device__ __forceinline__ void storeRay(float* __restrict__ region, uint32_t slot, const RayRegs& r) {
    const uint32_t b = slotWord(slot) * 4u;   // < 2^32: ptss_create bounds a region's bytes
    stPlane<kCoherent>(region, b, kOx, r.o.x);   stPlane<kCoherent>(region, b, kOy, r.o.y);   stPlane<kCoherent>(region, b, kOz, r.o.z);
    stPlane<kCoherent>(region, b, kDx, r.d.x);   stPlane<kCoherent>(region, b, kDy, r.d.y);   stPlane<kCoherent>(region, b, kDz, r.d.z);
    stPlane<kCoherent>(region, b, kL0x, r.L0.x); stPlane<kCoherent>(region, b, kL0y, r.L0.y); stPlane<kCoherent>(region, b, kL0z, r.L0.z);
    stPlane<kCoherent>(region, b, kTx, r.T.x);   stPlane<kCoherent>(region, b, kTy, r.T.y);   stPlane<kCoherent>(region, b, kTz, r.T.z);
    stPlane<kCoherent>(region, b, kPix, asF(r.pix));
    stPlane<kCoherent>(region, b, kR0, asF(r.rng.v[0]));
    stPlane<kCoherent>(region, b, kR1, asF(r.rng.v[1]));
    stPlane<kCoherent>(region, b, kR2, asF(r.rng.v[2]));
    stPlane<kCoherent>(region, b, kR3, asF(r.rng.v[3]));
    stPlane<kCoherent>(region, b, kR4, asF(r.rng.v[4]));
    stPlane<kCoherent>(region, b, kRd, asF(r.rng.d));
}

}  // namespace
}  // namespace ptss
