// ptwave.h — layer 0 of the device code of ptss_kernels.hip: bit casts, the wave-level votes and the lane-mask helpers every
// later layer uses (ptraypool.h, ptprim.h, ptaccel.h, pthit.h, ptshade.h). Restates no reference line: the reference has no
// wave-level code. Like every layer header it is private to the one translation unit that includes it (anonymous namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptmath.h"

namespace ptss {
using namespace ptv;   // vec3, quat and their operators (ptmath.h), for every layer and for the kernels
namespace {

__device__ __forceinline__ float asF(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ uint32_t asU(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ vec3 xyz(float4 v) { return vec3{v.x, v.y, v.z}; }
// "does any lane of the wave say yes": a ballot compared with zero stays in scalar registers (s_and / s_cmp / s_cbranch);
// hipcc's __any() round-trips the mask through a VGPR (v_cndmask + v_cmp) — two VALU instructions per triangle test
__device__ __forceinline__ bool waveAny(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// "every active lane says yes" (p must be one direct compare, see maskOf)
__device__ __forceinline__ bool waveAll(bool p) { return __builtin_amdgcn_ballot_w64(p) == __builtin_amdgcn_ballot_w64(true); }
// the set bits of a 64-bit wave mask below this lane (v_mbcnt_lo / v_mbcnt_hi), and the lane's own number in its wave
__device__ __forceinline__ uint32_t rankBelow(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
__device__ __forceinline__ uint32_t laneId() { return rankBelow(~0ull); }
// orders this wave's LDS traffic for the compiler; within one wave the LDS executes in order
__device__ __forceinline__ void waveLdsFence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// Lane predicates travel as 64-bit wave masks (one v_cmp each, combined with scalar ANDs, carried over the wave-uniform
// branch in SGPRs, turned back into a lane predicate for free by inverse_ballot). As bools they made hipcc round-trip
// through a VGPR — v_cndmask + v_cmp — every time a compound condition met a ballot: twice per triangle.
__device__ __forceinline__ unsigned long long maskOf(bool directCompare) { return __builtin_amdgcn_ballot_w64(directCompare); }

// A wave-uniform row of the scene image, addressed through a VECTOR register. The loops over primitives read rows that every lane
// shares; left to itself the compiler keeps such an address in a scalar register, bumps it with s_add and copies it into a VGPR in
// front of every group of LDS reads (ds_read takes vector addresses only) — one v_mov v, s per triangle head, one per weights block,
// one per sphere trip, each at the SGPR-operand issue cost (4.2 against 2.3 SIMD-cycles, tools/microbench/vgpr_banks.hip).
// vectorRow makes the address of row `row` of the image opaque to the uniformity analysis ONCE per query: the LDS byte address
// where the image is staged in LDS (decided at compile time wherever the image's address space is known), the byte offset into the
// image otherwise (global_load takes scalar base + vector offset). The loop advances it with a plain v_add_u32 (32, 48 and 64 are
// inline constants) and every read of a trip goes through rowAt with immediate offsets. Only addressing changes.
typedef __attribute__((address_space(3))) const float4 LdsRow;
constexpr uint32_t kRowBytes = 16u;   // one float4 row of the scene image
__device__ __forceinline__ uint32_t vectorRow(const float4* image, int row) {
    uint32_t at = (uint32_t)row * kRowBytes;
#if __HIP_DEVICE_COMPILE__   // (the host pass only parses device functions; it has no LDS address space)
    if (__builtin_amdgcn_is_shared(image)) at += (uint32_t)(uintptr_t)(LdsRow*)image;
#endif
    asm volatile("" : "+v"(at));
    return at;
}
__device__ __forceinline__ const float4* rowAt(const float4* image, uint32_t at) {
#if __HIP_DEVICE_COMPILE__
    if (__builtin_amdgcn_is_shared(image)) return (const float4*)(LdsRow*)(uintptr_t)at;
#endif
    return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(image) + at);
}

__device__ __forceinline__ uint32_t lowBits(int cnt) { return (cnt >= 32) ? 0xffffffffu : ((1u << cnt) - 1u); }
__device__ __forceinline__ uint32_t lowBitsClamped(int cnt) { return (cnt <= 0) ? 0u : lowBits(cnt); }

}  // namespace
}  // namespace ptss
