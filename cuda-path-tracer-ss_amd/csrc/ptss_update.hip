// ptss_update.hip — the kernels behind ptss_update_triangles (include/ptss.h): new vertex data that is already
// on the device is written into a live scene image, and the mesh image's leaf and group bounds are refitted around it, with no
// host round trip. The refit's arithmetic is csrc/ptmesh.h, shared with the host probe; this file moves the data and lays the
// reduction over the lanes of a wave.
#include <hip/hip_runtime.h>

#include "ptmesh.h"
#include "ptmotion.h"
#include "ptss_device.h"

namespace ptss {

constexpr int kUpdateBlock = 256;
constexpr int kTriWords = 19;   // sizeof(ptss_triangle) / 4
static_assert(sizeof(ptss_triangle) == kTriWords * 4, "ptss_triangle is 19 words");

// One record per thread. A workgroup's 256 records are 19,456 contiguous bytes: they are fetched with coalesced dword loads into
// LDS, and each thread then reads its own 19 words (an odd stride: no bank conflicts). A record with a vertex that is not finite
// or lies beyond |coordinate| <= 2^40 — the mesh image's precondition, which implies sphereBounded's and triDetBounded's — is
// counted and NOT written: the image never leaves the range its kernels were proven for. The material word and the key word
// (0xFFFFFFFE - original index) of the stored rows stay as they are; the rest is what packTriangles (ptpack.h) writes.
__global__ __launch_bounds__(kUpdateBlock) void sceneUpdateKernel(float4* __restrict__ blob, int offTri, int offTriNormal, int offTriVert,
                                                                  int offTriPos, const uint32_t* __restrict__ records, uint32_t first,
                                                                  uint32_t count, unsigned long long* __restrict__ rejected) {
    __shared__ uint32_t rec[kUpdateBlock * kTriWords];
    const uint32_t base = blockIdx.x * (uint32_t)kUpdateBlock;
    const uint32_t inBlock = count - base < (uint32_t)kUpdateBlock ? count - base : (uint32_t)kUpdateBlock;   // (base < count: the grid)
    const uint32_t* src = records + (size_t)base * kTriWords;
    for (uint32_t w = threadIdx.x; w < inBlock * kTriWords; w += kUpdateBlock) rec[w] = src[w];
    __syncthreads();
    if (threadIdx.x >= inBlock) return;
    const float* r = reinterpret_cast<const float*>(rec + threadIdx.x * kTriWords);   // v0, v1, v2, n0, n1, n2, materialIdx (ignored)
    if (!ptmo::recordAccepted(r)) {   // (false for NaN and infinities; ptss_render_features_motion asks the same question)
        if (rejected) atomicAdd(rejected, 1ull);
        return;
    }
    const int pos = reinterpret_cast<const int*>(blob + offTriPos)[first + base + threadIdx.x];
    float4* tri = blob + offTri + 3 * (size_t)pos;
    float4* nrm = blob + offTriNormal + 3 * (size_t)pos;
    float4* vert = blob + offTriVert + 2 * (size_t)pos;
    // e1 = v1 - v0, e2 = v2 - v0: packTriangles' single float subtraction (ptpack.h) (the build contracts nothing)
    tri[0] = float4{r[0], r[1], r[2], tri[0].w};
    tri[1] = float4{r[3] - r[0], r[4] - r[1], r[5] - r[2], tri[1].w};
    tri[2] = float4{r[6] - r[0], r[7] - r[1], r[8] - r[2], 0.0f};
    nrm[0] = float4{r[9], r[10], r[11], 0.0f};
    nrm[1] = float4{r[12], r[13], r[14], 0.0f};
    nrm[2] = float4{r[15], r[16], r[17], 0.0f};
    vert[0] = float4{r[3], r[4], r[5], 0.0f};
    vert[1] = float4{r[6], r[7], r[8], 0.0f};
}

// ---- the refit ---------------------------------------------------------------------------------------------------------------
// One wave per group of 256 stored positions, lane l holding positions 4 l .. 4 l + 3 in registers (36 floats): a leaf is four
// neighbouring lanes, the group the wave. Three dependent reductions, all by lane exchange (ptmesh.h has the shape and why it is
// fixed): the box -> the centres; reach, side, normal length and the axis sum -> R, Lmax, Nmin and the axes; the cone cosines.
// Exchanges with lane ^ 1 and ^ 2 finish the leaf, ^ 4 .. ^ 32 the group; every lane of a block ends with the block's value. An
// ordered merge takes the block of lower positions first, whichever lane evaluates it.
namespace {
using ptmesh::RefitBox;
using ptmesh::RefitStat;

__device__ __forceinline__ double xchg(double v, int mask) { return __shfl_xor(v, mask, 64); }
__device__ __forceinline__ RefitBox xchg(const RefitBox& b, int mask) {
    RefitBox o;
    for (int c = 0; c < 3; ++c) { o.lo[c] = xchg(b.lo[c], mask); o.hi[c] = xchg(b.hi[c], mask); }
    return o;
}
__device__ __forceinline__ RefitStat xchg(const RefitStat& s, int mask) {
    return RefitStat{xchg(s.r2, mask), xchg(s.l2, mask), xchg(s.nmin, mask), {xchg(s.sum[0], mask), xchg(s.sum[1], mask), xchg(s.sum[2], mask)}};
}
__device__ __forceinline__ RefitStat mergeAcross(const RefitStat& mine, int lane, int mask) {
    const RefitStat other = xchg(mine, mask);
    return (lane & mask) ? ptmesh::refitMerge(other, mine) : ptmesh::refitMerge(mine, other);
}
__device__ __forceinline__ void storeBound(float4* rows, const float b[12]) {
    for (int r = 0; r < 3; ++r) rows[r] = float4{b[4 * r], b[4 * r + 1], b[4 * r + 2], b[4 * r + 3]};
}
}  // namespace

__global__ __launch_bounds__(256) void meshRefitKernel(float4* __restrict__ blob, int numTriangles, int offTri, int numLeaves, int numGroups,
                                                       int offLeaf, int offGroup) {
    using namespace ptmesh;
    const int lane = threadIdx.x & 63;
    const int group = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (group >= numGroups) return;   // the whole wave
    float t[4][9];
    bool have[4];
    for (int j = 0; j < 4; ++j) {
        const int pos = group * kRefitSlots + lane * 4 + j;
        have[j] = pos < numTriangles;
        for (int k = 0; k < 9; ++k) t[j][k] = 0.0f;
        if (have[j]) {
            const float4* row = blob + offTri + 3 * (size_t)pos;
            const float4 a = row[0], b = row[1], c = row[2];
            t[j][0] = a.x; t[j][1] = a.y; t[j][2] = a.z;
            t[j][3] = b.x; t[j][4] = b.y; t[j][5] = b.z;
            t[j][6] = c.x; t[j][7] = c.y; t[j][8] = c.z;
        }
    }
    // 1: the boxes and their centres
    RefitBox box = refitEmptyBox();
    for (int j = 0; j < 4; ++j)
        if (have[j]) box = refitMerge(box, refitBoxOf(t[j]));
    for (int mask = 1; mask <= 2; mask *= 2) box = refitMerge(box, xchg(box, mask));
    float Cl[3], Cg[3];
    refitCentre(box, Cl);
    for (int mask = 4; mask <= 32; mask *= 2) box = refitMerge(box, xchg(box, mask));
    refitCentre(box, Cg);
    // 2: reach from each centre, longest side, smallest normal, the axis sum
    RefitStat s[4];
    double reachG = 0.0;
    for (int j = 0; j < 4; ++j) {
        s[j] = refitEmptyStat();
        if (have[j]) {
            s[j] = refitStatOf(t[j]);
            s[j].r2 = refitReach2(t[j], Cl);
            reachG = dmax(reachG, refitReach2(t[j], Cg));
        }
    }
    RefitStat m = refitMerge(refitMerge(s[0], s[1]), refitMerge(s[2], s[3]));
    for (int mask = 1; mask <= 2; mask *= 2) {
        m = mergeAcross(m, lane, mask);
        reachG = dmax(reachG, xchg(reachG, mask));
    }
    const RefitStat leafStat = m;
    m.r2 = reachG;
    for (int mask = 4; mask <= 32; mask *= 2) m = mergeAcross(m, lane, mask);
    const RefitStat groupStat = m;
    // 3: the cone cosines about each axis
    double al[3], ag[3];
    const bool haveL = refitAxis(leafStat, al), haveG = refitAxis(groupStat, ag);
    double cosL = 1.0, cosG = 1.0;
    for (int j = 0; j < 4; ++j)
        if (have[j]) {
            if (haveL) cosL = dmin(cosL, refitCos(t[j], al));
            if (haveG) cosG = dmin(cosG, refitCos(t[j], ag));
        }
    for (int mask = 1; mask <= 2; mask *= 2) { cosL = dmin(cosL, xchg(cosL, mask)); cosG = dmin(cosG, xchg(cosG, mask)); }
    for (int mask = 4; mask <= 32; mask *= 2) cosG = dmin(cosG, xchg(cosG, mask));
    float b[12];
    const int leaf = group * 16 + (lane >> 2);
    if ((lane & 3) == 0 && leaf < numLeaves) {
        refitFinish(Cl, leafStat, al, haveL, cosL, b);
        storeBound(blob + offLeaf + 3 * (size_t)leaf, b);
    }
    if (lane == 0) {
        refitFinish(Cg, groupStat, ag, haveG, cosG, b);
        storeBound(blob + offGroup + 3 * (size_t)group, b);
    }
}

hipError_t launchSceneUpdate(hipStream_t st, float4* sceneBlob, const SceneLayout& L, const void* records, uint32_t first, uint32_t count,
                             unsigned long long* rejected, unsigned long long* launched) {
    hipLaunchKernelGGL(sceneUpdateKernel, dim3((count + kUpdateBlock - 1) / kUpdateBlock), dim3(kUpdateBlock), 0, st, sceneBlob, L.offTri,
                       L.offTriNormal, L.offTriVert, L.offTriPos, static_cast<const uint32_t*>(records), first, count, rejected);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, PTSS_KERNEL_UPDATE);
    return e;
}

hipError_t launchMeshRefit(hipStream_t st, float4* sceneBlob, const SceneLayout& L, unsigned long long* launched) {
    hipLaunchKernelGGL(meshRefitKernel, dim3((unsigned)((L.mesh.numGroups + 3) / 4)), dim3(256), 0, st, sceneBlob, L.numTriangles, L.offTri,
                       L.mesh.numLeaves, L.mesh.numGroups, L.mesh.offLeaf, L.mesh.offGroup);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) markLaunched(launched, PTSS_KERNEL_REFIT);
    return e;
}

}  // namespace ptss
