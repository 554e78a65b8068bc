// ptscene.h — the description of a scene image: its layout record, the sizes that shape it and the LDS a workgroup needs
// beside it. Host-clean (no HIP header): shared by the kernels (through ptss_device.h), by the packer that builds an image
// (ptpack.h) and by the host mirror's probe of it (host/host_capi.cpp). See DESIGN.md "Where a scene image is built".
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PTSCENE_HD __host__ __device__
#else
#define PTSCENE_HD
#endif

namespace ptss {

// Two of the build-time switches (ptss_device.h has the others): the ones that shape the image and its work area.
#ifndef PTSS_BLOCK
#define PTSS_BLOCK 256    // rays per tile = threads per workgroup (128-ray tiles: -20 % at one sample per tick, profiles/README.md)
#endif
#ifndef PTSS_CHUNK
#define PTSS_CHUNK 16     // spheres per chunk of the many-sphere traversal (at most 16: chunkCandidates); with the kd-split order (ptpack.h
                          // spatialOrder), configs[4]'s scene at S = 4, same box: 4: 2,224, 8: 3,762, 16: 4,158-4,167 Mrays/s — every
                          // lane tests every chunk bound, so halving their number is worth more than the tighter fit of smaller chunks
#endif
constexpr int kBlock = PTSS_BLOCK;          // rays per tile = threads per workgroup
constexpr int kChunkSpheres = PTSS_CHUNK;
static_assert((kChunkSpheres & (kChunkSpheres - 1)) == 0, "chunk size must be a power of two");   // spheres per chunk of the many-sphere traversal
constexpr int kWaves = kBlock / 64;

// ---- range guards proven once per scene (FrameBuffers::guardFlags; ptpack.h sceneGuardFlags decides at ptss_create / ptss_set_scene) ----
// A set bit lets the kernels run the unguarded fast division / reciprocal on that scene constant; a clear bit leaves the guarded code.
enum GuardFlag : uint32_t {
    kGuardLightPowers = 1u,    // every component of every light power is +0.0 or has |p| in [2^-60, 2^60): numerators of L_i (addLambertTerm)
    kGuardRefraction = 2u,     // every material's index of refraction has |n| in [2^-60, 2^60): n1 / n2 in scatter (the other operand is 1)
    kGuardPhongExponent = 4u,  // every material's specularExponent is +inf (its Phong sampler never runs) or has |exponent + 1| in
                               // [2^-125, 2^126): rcp(exponent + 1) in scatter
};

// ---- scene blob: one contiguous array of float4 staged into LDS by every workgroup --------------
// (scene records are read by all lanes at the same index -> LDS broadcast reads)
struct SceneLayout {
    int numSpheres, numTriangles, numMaterials, numPointLights, numAreaLights;
    // offsets in float4 units
    int offSphere;      // S x {cx, cy, cz, radius^2}; with accelSpheres: the spheres in spatially sorted order, padded to whole
                        // chunks of kChunkSpheres with copies of the last one
    int offSphereMat;   // ceil(S/4) x 4 ints
    int offTri;         // T x 3: {v0.xyz, bits(materialIdx)}, {e1.xyz, bits(0xFFFFFFFE - original index)}, {e2.xyz, 0} — in storage order (triClassed)
    int offTriNormal;   // T x 3: {n0,0},{n1,0},{n2,0}
    int offTriVert;     // T x 2: {v1,0},{v2,0}   (area-light sampling)
    int offMaterial;    // M x 5: {diffuseColor, diffAvg},{specularColor, specAvg},{absorption, refrAvg},
                        //        {emmitance, roughness},{specularExponent, indexOfRefraction, bits(flags), 0}
    int offPointLight;  // P x 2: {position,0},{power,0}
    int offAreaLight;   // A x 2: {power, bits(position of triangle triangleIdx)}, {bits(position of triangleIdx + 1), 0, 0, 0}
    // Sphere acceleration (scenes with many spheres; ptpack.h planImages decides): chunks of kChunkSpheres consecutive sorted spheres
    // with a conservative bounding sphere each; a lane visits only the chunks its ray can touch (ptaccel.h).
    int accelSpheres;   // 0: every sphere is tested by every ray (the reference's loop); 1: chunked
    int numChunks;
    int offChunk;       // numChunks x {Cx, Cy, Cz, inflated R^2}
    int offSphereOrig;  // ints: original (caller's) index of each sorted sphere — decides ties the way the reference's order does
    int offSpherePos;   // ints: the inverse, sorted position of each original index (regrouped traversal: winner by original index)
    int offQuant;       // 65 rows: the 8-bit tone-map thresholds T[0..256] (ptquant.h), read by finishPath
    int offPrimSphere;  // S x {o - centre, dot(v,v) - r^2}        written on the device per camera (primaryPrepKernel)
    int offPrimTri;     // T x 2: {o - v0, dot(e2, r)}, {r = cross(s, e1), 0}
    int offPrimChunk;   // many-sphere image: numChunks x {o - C, dot(v,v) - bound, rounded down}, per camera as well (bounce 0's chunk test)
    int totalVec4;
    int ldsVec4;        // rows [0, ldsVec4) are staged into LDS; the rest (the many-sphere integer tables: material, original
                        // index, position — read only when a hit is accepted) stay in global memory
    int neeSkipSafe;    // 1: light powers and diffuse colours are finite, so zero Lambert terms are exactly +-0
    int sphereBounded;  // 1: every |coordinate| <= 1e15 and every sphere radius in [1e-12, 1e15]: the sphere candidate tests may take
                        //    the two-instructions-shorter discriminant form (ptprim.h shiftInSphere<true>) while the camera is in range
    int neePairs;       // 1: at least two lights and at least four of five primitives reflect diffusely (diffAvg > 0): a lit point then
                        //    nearly always needs both of its shadow segments, and the kernels that test the pair together (shared origin
                        //    terms, pairAnyHit) pay: +4.8 % on configs[1]'s scene; with specular-only materials about the scene many entries
                        //    hold one segment and they do not: -1.4 % on configs[2]'s
    int triDetBounded;  // 1: every triangle has |e1| |e2| <= 2^100 (finite), so |det| = |e1 . (d x e2)| < 2^126 whenever
                        //    |d|^2 < 2^30 — the closest-hit triangle loop may then use the reciprocal's fast path unguarded
    int triClassed;     // 1: every vertex is finite (bounded geometry) and the triangles are STORED GROUPED BY EDGE CLASS (pttri.h; the
                        //    caller's order inside a group; T <= 255): the uniform triangle loops run one loop per class, each with the body that
                        //    leaves out the products with that class's exact-zero edge components; the closest hit decides by the key
                        //    (distance, ~original index), which is what the reference's sequential `dist <= distance` rule ends on.
                        //    0: the caller's order, the general body, the sequential rule
    // Classed scenes (T <= 255) and mesh images (T >= 512) never coincide, so the two share these five words: the layout keeps
    // its size and every field its offset (the kernels of the other images read the same kernel-argument words as before).
    union {
        uint32_t triClassPack[5];  // positions [begin(c), begin(c + 1)) hold the triangles of class code c = class(e1) * 4 + class(e2): the 17 begins
                                   // (begin(16) = T) as BYTES, four per word — five scalar registers instead of seventeen (classed scenes have
                                   // T <= 255); a loop header extracts its two bounds with two s_bfe (ptprim.h classBegin)
        struct {
            // Mesh image (ptpack.h meshEligible): the triangles stored in a kd order of their centroids, every
            // kMeshLeaf consecutive positions a LEAF and every kMeshLeaf^2 a GROUP, each with a conservative bound of three rows
            // (ptmesh.h). numLeaves = 0: not a mesh image. The triangle tables (offTri, offTriNormal, offTriVert, offTriPos,
            // offPrimTri) lie beyond ldsVec4: global memory, read through the kernels' `cold` pointer.
            int numLeaves, numGroups;
            int offGroup;   // numGroups x 3 rows, staged in LDS
            int offLeaf;    // numLeaves x 3 rows: in LDS when offLeaf < ldsVec4, else in global memory
            int reserved;
        } mesh;
    };
    int offTriPos;      // ints: stored position of each original triangle index
};

constexpr int kMeshLeaf = 16;   // triangles per leaf = leaves per group of the mesh image
// the mesh image is in use (a classed image's byte table would alias mesh.numLeaves; classed scenes have T <= 255)
PTSCENE_HD inline bool meshImage(const SceneLayout& L) { return !L.triClassed && L.mesh.numLeaves > 0; }

// ---- LDS work area behind the scene image -----------------------------------------------------
// block: [0..kWaves) wave survivor totals, [8] block base in the output region
// per wave: the shadow-ray queue of one NEE round (kNeeLights lights x 64 lanes):
//           7 float planes (lo.xyz, w_i.xyz, max distance) + 1 word (owner lane | slot-in-round << 8),
//           then kNeeLights x 64 answer BYTES.
constexpr int kNeeLights = 2;                       // lights regrouped per round
constexpr int kQueueCap = kNeeLights * 64;
constexpr int kWaveLdsWords = 8 * kQueueCap + kNeeLights * 64 / 4;  // answers are bytes: 24,048 -> 22,512 B per workgroup
                                                                    // with the 38-primitive scenes, i.e. 7 workgroups per CU instead of 6
constexpr int kBlockScratchVec4 = 4;
constexpr int kBlockLdsVec4 = kBlockScratchVec4 + (kWaves * kWaveLdsWords + 3) / 4;

constexpr size_t kVec4Bytes = 16;   // one row of the image (a float4)
// dynamic LDS of a bounce / frame workgroup: the staged part of the image (sceneInLds) and the work area behind it
inline size_t bounceLdsBytes(const SceneLayout& layout, bool sceneInLds) {
    return ((sceneInLds ? (size_t)layout.ldsVec4 : 0) + kBlockLdsVec4) * kVec4Bytes;
}

}  // namespace ptss
