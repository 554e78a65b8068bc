// ptpack.h — building a scene image on the host: which images a scene gets (planImages), their rows (packScene) and the
// checks of a scene description (validateScene). Pure host arithmetic, no HIP type: included by the context code
// (ptss_api.hip, which uploads the rows as float4) and by the host mirror (host/host_capi.cpp, ptss_probe_pack_scene), so
// that every byte of an image can be pinned on a machine without a GPU (tests/test_pack_scene.py).
// The image's description — SceneLayout and the sizes that shape it — is ptscene.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <utility>
#include <vector>

#include "ptmath.h"
#include "ptmesh.h"
#include "ptquant.h"
#include "ptscene.h"
#include "ptss_types.h"
#include "pttri.h"

namespace ptpack {
using namespace ptv;
using ptss::SceneLayout;

// One row of an image: what the device reads as a float4.
struct alignas(16) Row {
    float x, y, z, w;
};
static_assert(sizeof(Row) == ptss::kVec4Bytes, "a row is a float4");
inline float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
inline int* intsAt(std::vector<Row>& blob, int off) { return reinterpret_cast<int*>(&blob[(size_t)off]); }   // an integer table of the image

// ---- sphere acceleration (scenes with many spheres) ------------------------------------------------------------------
// The kernel may skip a sphere only if the reference's test certainly rejects it (Primitives.h:107-127, float32): its
// discriminant is certainly negative, or both its roots are. Spheres are sorted spatially (spatialOrder) and cut into chunks of kChunkSpheres; each chunk gets
// a bounding sphere (C, R) with |c_i - C| + r_i <= R for its members. For a ray (o, d) with | |d|^2 - 1 | <= eps = 1e-5
// let vC = o - C, vv = vC.vC, dv = d.vC, dm = min(dv, 0). The kernel culls the chunk iff
//       vv - (1 + 2 eps) / (1 - mu) dm^2  >  R^2 (1 + m)^3 (1 + 4e-6) / (1 - mu)        with m = 5e-3, mu = m + m^2
// (shiftInChunk: the right side is the stored bound, the factor of dm^2 is 4 kAccelQ, both rounded up).
// Why that is safe. Let E be the distance of C from the RAY {o + t d^, t >= 0}: E^2 = vv - dm^2 / |d|^2 (the line's distance
// while the closest approach lies ahead, |vC| once it lies behind the origin), and 1 / |d|^2 <= 1 + 2 eps. Multiplied by
// (1 - mu) the test says E^2 - mu vv > R^2 (1+m)^3 (1 + 4e-6) in real arithmetic; the float evaluation of the left side
// (v rounded per component, two three-term dot products, t = dv - |dv| exact, one product, one fma) errs by less than
// 1e-6 vv, which the factor (1 + 4e-6) pays for even where the next step has no slack (|vC| = R (1 + m)):
// R^2 (1+m)^3 + mu vv >= (R + m (|vC| + R))^2 (AM-GM), so E > R + m (|vC| + R). The distance of a member's centre from the
// ray is then E_i >= E - |c_i - C| > r_i + m |v_i| (|v_i| <= |vC| + R), i.e. E_i^2 > r_i^2 + 2.5e-5 |v_i|^2. Two cases.
// The member's closest approach lies ahead (d.v_i <= 0): E_i is the line's distance dist_i, and the exact discriminant / 4,
// r_i^2 - dist_i^2 + (|d|^2 - 1)(d^.v_i)^2 <= r_i^2 - dist_i^2 + 1e-5 |v_i|^2, is below -1.5e-5 |v_i|^2; float32 evaluation
// moves it by less than 1e-6 |v_i|^2 (|v_i| > r_i here): negative, Sphere::intersectRay returns false (Primitives.h:118).
// It lies behind (d.v_i > 0): E_i = |v_i|, so c = |v_i|^2 - r_i^2 > 2.5e-5 |v_i|^2, in float32 still > 2.4e-5 |v_i|^2. If
// the float discriminant b^2 - 4c is negative the test returns false; if not, b^2 >= 4c > 9.6e-5 |v_i|^2 puts |b| far above
// its rounding error (5e-7 |v_i|), so b has its true sign, positive, and 4c >= 2.4e-5 b^2 keeps sqrt(b^2 - 4c) below
// b (1 - 1e-5): both roots (-b +- sqrt) / 2 are negative beyond any rounding and the test returns false (Primitives.h:123-127).
// Rays whose direction is not unit to 1e-5 (the reference does not renormalise blended vertex normals) visit every chunk;
// a NaN anywhere fails the `>`. Until round 3 the kernel tested the LINE's distance and, separately, "the bound lies wholly
// behind the plane through the origin": the ray's distance is one test instead of two and skips more — a ray that leaves
// a chunk it starts beside no longer enters it (tools/chunk_bounds_stat.py: 5.09 -> 4.67 chunks per mid-bounce ray).
// Requires finite, moderate geometry (|coordinate|, radius <= 1e15, radius >= 1e-12) so that no discriminant overflows; packScene and
// the per-frame camera check fall back to the plain image otherwise.
constexpr double kAccelM = 5e-3;
constexpr float kAccelLimit = 1e15f;
constexpr int kAccelMinSpheres = 64;

// Finite, moderate geometry: every |coordinate| <= 1e15, every sphere radius in [1e-12, 1e15] (false for NaN and infinities).
// What the chunked traversal requires, and what lets the sphere candidate tests take their shorter form
// (SceneLayout::sphereBounded, ptprim.h shiftInSphere<true>: r^2 well inside the normal range, no discriminant near overflow).
inline bool geometryBounded(const ptss_scene_desc& s) {
    auto ok = [](float v) { return std::fabs(v) <= kAccelLimit; };
    for (size_t i = 0; i < s.numSpheres; ++i) {
        const ptss_sphere& sp = s.spheres[i];
        if (!ok(sp.position.x) || !ok(sp.position.y) || !ok(sp.position.z) || !ok(sp.radius)) return false;
        if (!(std::fabs(sp.radius) >= 1e-12f)) return false;
    }
    for (size_t i = 0; i < s.numTriangles; ++i) {
        const ptss_triangle& t = s.triangles[i];
        for (const ptss_vec3* v : {&t.vertex0, &t.vertex1, &t.vertex2})
            if (!ok(v->x) || !ok(v->y) || !ok(v->z)) return false;
    }
    for (size_t i = 0; i < s.numPointLights; ++i)
        if (!ok(s.pointLights[i].position.x) || !ok(s.pointLights[i].position.y) || !ok(s.pointLights[i].position.z)) return false;
    return true;
}
inline bool cameraInRange(const ptss_camera& cam) {
    auto ok = [](float v) { return std::fabs(v) <= kAccelLimit; };
    return ok(cam.position.x) && ok(cam.position.y) && ok(cam.position.z);
}

inline bool accelEligible(const ptss_scene_desc& s) { return s.numSpheres >= (size_t)kAccelMinSpheres && geometryBounded(s); }

// ---- the mesh image (SceneLayout::mesh) ---------------------------------------------------------------------
// Scenes of many triangles and few spheres: 512 triangles or more — every edge-classed scene (T <= 255) keeps its image, and so
// does every scene of the older test suites, the largest of which (tests/test_gpu_kernel_coverage.py, the in-place cases) holds
// 484 triangles —, fewer than kAccelMinSpheres spheres (those keep the sphere chunks), at most 2^20 triangles,
// and every vertex finite with |coordinate| <= 2^40 — which, with the kernels' per-query test |o|^2 < 2^80, |d|^2 = 1 +- 1e-5,
// keeps every intermediate of the reference's test finite: |det| <= |e1| |e2| |d| < 2^84, |e2 . r| <= |e2| |o - v0| |e1| < 2^126
// (so no NaN distance either), and the reciprocal inside its fast range.
constexpr int kMeshMinTriangles = 512;
constexpr size_t kMeshMaxTriangles = size_t(1) << 20;
inline bool meshEligible(const ptss_scene_desc& s) {
    if (s.numTriangles < (size_t)kMeshMinTriangles || s.numTriangles > kMeshMaxTriangles || s.numSpheres >= (size_t)kAccelMinSpheres) return false;
    auto ok = [](float v) { return std::fabs(v) <= 0x1p40f; };   // false for NaN and infinities
    for (size_t i = 0; i < s.numTriangles; ++i) {
        const ptss_triangle& t = s.triangles[i];
        for (const ptss_vec3* v : {&t.vertex0, &t.vertex1, &t.vertex2})
            if (!ok(v->x) || !ok(v->y) || !ok(v->z)) return false;
    }
    return true;
}

// ---- the kd order of spheres and of triangles --------------------------------------------------------------------------------
// Orders idx[lo, hi) — indices into the points p — in place. The points are split recursively at the median along the axis of
// largest extent (a kd-tree built by std::nth_element; ties by original index, so the order is deterministic), the cut
// placed at a multiple of `coarse` points while a part holds more than `coarse` and at a multiple of `leaf` below that: every
// `leaf` consecutive positions are a leaf and every `coarse` consecutive positions a subtree.
// The spheres' centres, (kChunkSpheres, 64): a chunk is a leaf. Against round 1's Morton curve (whose jumps put far-apart spheres
// into one chunk) a ray of the configs[5] scene meets about half as many chunk bounds. Any permutation is legal there: the
// traversal decides ties by ORIGINAL index (offSphereOrig).
// The triangles' centroids, (kMeshLeaf, kMeshLeaf^2): every kMeshLeaf consecutive positions are a leaf and every kMeshLeaf^2 a
// group. Any permutation is legal, the closest hit being keyed by original index.
using Point = std::array<float, 3>;
inline void kdOrder(const std::vector<Point>& p, std::vector<int>& idx, int lo, int hi, int leaf, int coarse) {
    const int n = hi - lo;
    if (n <= leaf) return;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lo; i < hi; ++i)
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], p[(size_t)idx[i]][a]);
            mx[a] = std::max(mx[a], p[(size_t)idx[i]][a]);
        }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
    const int unit = n > coarse ? coarse : leaf;
    int left = ((n / 2 + unit - 1) / unit) * unit;  // points in the lower part: about half, a whole number of units
    if (left >= n) left -= unit;
    if (left <= 0) return;
    std::nth_element(idx.begin() + lo, idx.begin() + lo + left, idx.begin() + hi, [&](int a, int b) {
        const float ka = p[(size_t)a][axis], kb = p[(size_t)b][axis];
        return ka < kb || (ka == kb && a < b);
    });
    kdOrder(p, idx, lo, lo + left, leaf, coarse);
    kdOrder(p, idx, lo + left, hi, leaf, coarse);
}

// A ball around n member spheres: from the mean of their centres, `steps` steps of "move towards the farthest point of the
// farthest member by 1 / (step + 1) of the way" (Badoiu-Clarkson), keeping the best centre seen — close to the smallest
// enclosing ball. Any centre is legal for a chunk bound: packScene measures R from the float centre it stores.
struct Ball {
    double c[3], r;
};
inline Ball enclosingBall(const ptss_scene_desc& s, const int* idx, int n, int steps) {
    auto reach = [&](const double c[3], int j, double* toward) {   // distance from c to the far side of member j
        const ptss_sphere& sp = s.spheres[idx[j]];
        const double dx = (double)sp.position.x - c[0], dy = (double)sp.position.y - c[1], dz = (double)sp.position.z - c[2];
        const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (toward) { toward[0] = len > 0 ? dx / len : 0; toward[1] = len > 0 ? dy / len : 0; toward[2] = len > 0 ? dz / len : 0; }
        return len + std::fabs((double)sp.radius);
    };
    double C[3] = {0, 0, 0};
    for (int j = 0; j < n; ++j) {
        C[0] += s.spheres[idx[j]].position.x / n; C[1] += s.spheres[idx[j]].position.y / n; C[2] += s.spheres[idx[j]].position.z / n;
    }
    Ball best{{C[0], C[1], C[2]}, INFINITY};
    for (int step = 1; step <= steps; ++step) {
        int far = 0;
        double farR = -1, dir[3];
        for (int j = 0; j < n; ++j) {
            const double r = reach(C, j, nullptr);
            if (r > farR) { farR = r; far = j; }
        }
        if (!(farR < INFINITY)) break;
        if (farR < best.r) best = Ball{{C[0], C[1], C[2]}, farR};
        reach(C, far, dir);
        for (int a = 0; a < 3; ++a) C[a] += dir[a] * farR / (step + 1);
    }
    return best;
}
// The kd leaves, improved pair by pair: the members of a chunk and of one of its six nearest chunks are split again, half
// and half, along the line joining the two centres, the axes and three diagonals, and the split with the smallest
// R_a^2 + R_b^2 (the two balls' cross-sections, what a passing line sees) replaces the pair if it beats the present one.
// Up to three sweeps over scenes of up to 256 chunks, one up to 1,024, none beyond (the cost grows with the chunk count and
// is paid at scene set-up). configs[4]'s scene: a mid-bounce ray touches 3.73 bounds instead of 3.95.
inline void refineChunks(const ptss_scene_desc& s, std::vector<int>& order) {
    constexpr int kM = ptss::kChunkSpheres;
    const int K = (int)(order.size() / kM);   // whole chunks only
    const int sweeps = K < 2 ? 0 : (K <= 256 ? 3 : (K <= 1024 ? 1 : 0));
    if (sweeps == 0) return;
    std::vector<Ball> ball((size_t)K);
    for (int k = 0; k < K; ++k) ball[(size_t)k] = enclosingBall(s, &order[(size_t)k * kM], kM, 64);
    auto centre = [&](int i, int a) { return a == 0 ? (double)s.spheres[i].position.x : (a == 1 ? (double)s.spheres[i].position.y : (double)s.spheres[i].position.z); };
    for (int sweep = 0; sweep < sweeps; ++sweep) {
        int improved = 0;
        for (int a = 0; a < K; ++a) {
            std::vector<std::pair<double, int>> near;
            for (int b = 0; b < K; ++b) {
                if (b == a) continue;
                double d2 = 0;
                for (int x = 0; x < 3; ++x) d2 += (ball[(size_t)b].c[x] - ball[(size_t)a].c[x]) * (ball[(size_t)b].c[x] - ball[(size_t)a].c[x]);
                near.emplace_back(d2, b);
            }
            const size_t take = std::min<size_t>(6, near.size());
            std::partial_sort(near.begin(), near.begin() + take, near.end());
            for (size_t q = 0; q < take; ++q) {
                const int b = near[q].second;
                int both[2 * kM], trial[2 * kM], keep[2 * kM];
                for (int j = 0; j < kM; ++j) { both[j] = order[(size_t)a * kM + j]; both[kM + j] = order[(size_t)b * kM + j]; }
                double bestCost = ball[(size_t)a].r * ball[(size_t)a].r + ball[(size_t)b].r * ball[(size_t)b].r;
                const double floor = bestCost * (1 - 1e-9);
                Ball keepA{}, keepB{};
                bool found = false;
                const double join[3] = {ball[(size_t)b].c[0] - ball[(size_t)a].c[0], ball[(size_t)b].c[1] - ball[(size_t)a].c[1], ball[(size_t)b].c[2] - ball[(size_t)a].c[2]};
                const double dirs[7][3] = {{join[0], join[1], join[2]}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {0, 1, 1}, {1, 0, 1}};
                for (const auto& dir : dirs) {
                    std::copy(both, both + 2 * kM, trial);
                    auto key = [&](int i) { return centre(i, 0) * dir[0] + centre(i, 1) * dir[1] + centre(i, 2) * dir[2]; };
                    std::sort(trial, trial + 2 * kM, [&](int x, int y) { return key(x) < key(y) || (key(x) == key(y) && x < y); });
                    const Ball ta = enclosingBall(s, trial, kM, 48), tb = enclosingBall(s, trial + kM, kM, 48);
                    const double cost = ta.r * ta.r + tb.r * tb.r;
                    if (cost < bestCost && cost < floor) {
                        bestCost = cost; keepA = ta; keepB = tb; found = true;
                        std::copy(trial, trial + 2 * kM, keep);
                    }
                }
                if (found) {
                    for (int j = 0; j < kM; ++j) { order[(size_t)a * kM + j] = keep[j]; order[(size_t)b * kM + j] = keep[kM + j]; }
                    ball[(size_t)a] = keepA; ball[(size_t)b] = keepB;
                    ++improved;
                }
            }
        }
        if (improved == 0) break;
    }
}
// sorted position -> original index of the spheres: the kd order of their centres, its leaves refined
inline std::vector<int> spatialOrder(const ptss_scene_desc& s) {
    std::vector<int> order((size_t)s.numSpheres);
    std::vector<Point> centre((size_t)s.numSpheres);
    for (size_t i = 0; i < s.numSpheres; ++i) {
        order[i] = (int)i;
        centre[i] = Point{s.spheres[i].position.x, s.spheres[i].position.y, s.spheres[i].position.z};
    }
    kdOrder(centre, order, 0, (int)s.numSpheres, ptss::kChunkSpheres, 64);
    refineChunks(s, order);
    return order;
}

// ---- packScene's steps, in the order packScene calls them ---------------------------------------------------------------------

// rows of the sphere table: whole chunks in the many-sphere image, the caller's spheres otherwise
inline int sphereRowsOf(const SceneLayout& L) { return L.accelSpheres ? L.numChunks * ptss::kChunkSpheres : L.numSpheres; }
// plain image: sphere rows (and their camera-origin twins) padded to a multiple of four, zero-filled — the
// candidate pass fetches four rows per trip and drops the padding's bits (sphereCandidates)
inline int sphereAllocOf(const SceneLayout& L) { return L.accelSpheres ? sphereRowsOf(L) : (sphereRowsOf(L) + 3) / 4 * 4; }

inline void setCounts(const ptss_scene_desc& s, bool accel, SceneLayout& L) {
    L.accelSpheres = accel ? 1 : 0;
    L.numChunks = accel ? (int)((s.numSpheres + ptss::kChunkSpheres - 1) / ptss::kChunkSpheres) : 0;
    L.numSpheres = (int)s.numSpheres;
    L.numTriangles = (int)s.numTriangles;
    L.numMaterials = (int)s.numMaterials;
    L.numPointLights = (int)s.numPointLights;
    L.numAreaLights = (int)s.numAreaLights;
}

// The offset table of the plain and of the many-sphere image (accel): everything up to ldsVec4 is staged into LDS.
inline void layoutPlain(const ptss_scene_desc& s, bool accel, SceneLayout& L) {
    setCounts(s, accel, L);
    const int sphereRows = sphereRowsOf(L), sphereAlloc = sphereAllocOf(L);
    int off = 0;
    L.offSphere = off;      off += sphereAlloc;
    if (!accel) { L.offSphereMat = off; off += (sphereRows + 3) / 4; }
    L.offChunk = off;       off += (L.numChunks + 3) / 4 * 4;   // bound rows padded to a multiple of four (zero rows: chunkMask drops their bits)
    L.offTri = off;         off += 3 * L.numTriangles;
    L.offTriNormal = off;   off += 3 * L.numTriangles;
    L.offTriVert = off;     off += 2 * L.numTriangles;
    L.offMaterial = off;    off += 5 * L.numMaterials;
    L.offPointLight = off;  off += 2 * L.numPointLights;
    L.offAreaLight = off;   off += 2 * L.numAreaLights;
    L.offTriPos = off;      off += (L.numTriangles + 3) / 4;   // ints: stored position of each original triangle index
    L.offQuant = off;       off += ptq::kTableFloats / 4;
    L.offPrimSphere = off;  off += accel ? 0 : sphereAlloc;  // the chunked traversal keeps the camera-origin parts of its chunk bounds only (offPrimChunk)
    L.offPrimTri = off;     off += 2 * L.numTriangles;
    L.offPrimChunk = off;   off += accel ? (L.numChunks + 3) / 4 * 4 : 0;
    L.ldsVec4 = off;        // everything up to here is staged into LDS
    if (accel) {            // cold integer tables of the many-sphere image: global memory only
        L.offSphereMat = off;   off += (sphereRows + 3) / 4;
        L.offSphereOrig = off;  off += (sphereRows + 3) / 4;
        L.offSpherePos = off;   off += (L.numSpheres + 3) / 4;
    } else {
        L.offSphereOrig = L.offSpherePos = 0;
    }
    L.totalVec4 = off;
    for (int k = 0; k < 5; ++k) L.triClassPack[k] = 0u;   // (orderTriangles fills it in; as mesh dimensions: numLeaves = 0, no mesh image)
}

// The offset table of the mesh image: group bounds, leaf bounds where they fit, spheres, materials, lights and the tone-map table
// are staged in LDS; the triangle tables stay in global memory (read through `cold`) — T x 10 rows would not fit beyond ~400
// triangles. (T >= 512: never classed, so the union holds the mesh dimensions.)
inline void layoutMesh(const ptss_scene_desc& s, SceneLayout& L) {
    setCounts(s, false, L);
    const int sphereRows = sphereRowsOf(L), sphereAlloc = sphereAllocOf(L);
    const int numLeaves = (L.numTriangles + ptss::kMeshLeaf - 1) / ptss::kMeshLeaf;
    const int numGroups = (numLeaves + ptss::kMeshLeaf - 1) / ptss::kMeshLeaf;
    int off = 0;
    L.offSphere = off;      off += sphereAlloc;
    L.offSphereMat = off;   off += (sphereRows + 3) / 4;
    L.offChunk = off;
    const int offGroup = off;   off += 3 * ((numGroups + 3) / 4 * 4);   // padded to whole trips of four bounds (meshGroupMask drops their bits)
    const int leafRows = 3 * numLeaves;
    const int rest = 5 * L.numMaterials + 2 * L.numPointLights + 2 * L.numAreaLights + ptq::kTableFloats / 4 + sphereAlloc;
    SceneLayout probe{};
    probe.ldsVec4 = off + leafRows + rest;
    const bool leavesInLds = ptss::bounceLdsBytes(probe, true) <= 64 * 1024;
    int offLeaf = 0;
    if (leavesInLds) { offLeaf = off; off += leafRows; }
    L.offMaterial = off;    off += 5 * L.numMaterials;
    L.offPointLight = off;  off += 2 * L.numPointLights;
    L.offAreaLight = off;   off += 2 * L.numAreaLights;
    L.offQuant = off;       off += ptq::kTableFloats / 4;
    L.offPrimSphere = off;  off += sphereAlloc;
    L.offPrimChunk = off;
    L.ldsVec4 = off;
    if (!leavesInLds) { offLeaf = off; off += leafRows; }
    L.offTri = off;         off += 3 * L.numTriangles;
    L.offTriNormal = off;   off += 3 * L.numTriangles;
    L.offTriVert = off;     off += 2 * L.numTriangles;
    L.offTriPos = off;      off += (L.numTriangles + 3) / 4;
    L.offPrimTri = off;     off += 2 * L.numTriangles;
    L.offSphereOrig = L.offSpherePos = 0;
    L.totalVec4 = off;
    L.mesh.numLeaves = numLeaves;
    L.mesh.numGroups = numGroups;
    L.mesh.offGroup = offGroup;
    L.mesh.offLeaf = offLeaf;
    L.mesh.reserved = 0;
}

// The scene flags neeSkipSafe, sphereBounded, neePairs, triDetBounded and triClassed (each described at its SceneLayout field).
inline void setFlags(const ptss_scene_desc& s, SceneLayout& L) {
    auto finite3 = [](const ptss_vec3& v) { return v.x - v.x == 0.0f && v.y - v.y == 0.0f && v.z - v.z == 0.0f; };
    L.neeSkipSafe = 1;
    for (size_t i = 0; i < s.numMaterials; ++i)
        if (!finite3(s.materials[i].diffuseColor) || !(s.materials[i].diffAvg - s.materials[i].diffAvg == 0.0f)) L.neeSkipSafe = 0;
    for (size_t i = 0; i < s.numPointLights; ++i)
        if (!finite3(s.pointLights[i].power)) L.neeSkipSafe = 0;
    for (size_t i = 0; i < s.numAreaLights; ++i)
        if (!finite3(s.areaLights[i].power)) L.neeSkipSafe = 0;
    L.sphereBounded = geometryBounded(s) ? 1 : 0;  // see SceneLayout::sphereBounded
    {   // see SceneLayout::neePairs: at least two lights, and at least four of five primitives wear a diffusely reflecting material
        size_t diffuse = 0;
        for (size_t i = 0; i < s.numSpheres; ++i) diffuse += s.materials[s.spheres[i].materialIdx].diffAvg > 0.0f ? 1 : 0;
        for (size_t i = 0; i < s.numTriangles; ++i) diffuse += s.materials[s.triangles[i].materialIdx].diffAvg > 0.0f ? 1 : 0;
        L.neePairs = (L.sphereBounded && s.numPointLights + s.numAreaLights >= 2 && 5 * diffuse >= 4 * (s.numSpheres + s.numTriangles)) ? 1 : 0;
    }
    L.triDetBounded = 1;  // see SceneLayout::triDetBounded
    for (size_t i = 0; i < s.numTriangles; ++i) {
        const ptss_triangle& t = s.triangles[i];
        const vec3 e1 = t.vertex1 - t.vertex0, e2 = t.vertex2 - t.vertex0;  // as stored (packTriangles)
        const double n1 = std::sqrt((double)e1.x * e1.x + (double)e1.y * e1.y + (double)e1.z * e1.z);
        const double n2 = std::sqrt((double)e2.x * e2.x + (double)e2.y * e2.y + (double)e2.z * e2.z);
        if (!(n1 * n2 <= 0x1p100)) L.triDetBounded = 0;  // false for NaN / infinite edges as well
    }
    L.triClassed = (L.triDetBounded && L.sphereBounded && L.numTriangles <= 255) ? 1 : 0;   // (the class bounds travel as bytes)
}

// The range guards this scene's constants satisfy (ptscene.h GuardFlag; the membership functions are ptmath.h's). Not part of the
// image: the verdict travels in FrameBuffers::guardFlags.
inline uint32_t sceneGuardFlags(const ptss_scene_desc& s) {
    uint32_t flags = ptss::kGuardLightPowers | ptss::kGuardRefraction | ptss::kGuardPhongExponent;
    auto fast3 = [](const ptss_vec3& v) { return ptm::fast_numerator(v.x) && ptm::fast_numerator(v.y) && ptm::fast_numerator(v.z); };
    for (size_t i = 0; i < s.numPointLights; ++i)
        if (!fast3(s.pointLights[i].power)) flags &= ~(uint32_t)ptss::kGuardLightPowers;
    for (size_t i = 0; i < s.numAreaLights; ++i)
        if (!fast3(s.areaLights[i].power)) flags &= ~(uint32_t)ptss::kGuardLightPowers;
    for (size_t i = 0; i < s.numMaterials; ++i) {
        const float n = s.materials[i].indexOfRefraction, e = s.materials[i].specularExponent;
        if (!ptm::fast_divisor(n)) flags &= ~(uint32_t)ptss::kGuardRefraction;
        if (!(e == ptm::inf() || ptm::fast_rcp_operand(e + 1))) flags &= ~(uint32_t)ptss::kGuardPhongExponent;
    }
    return flags;
}

// Storage order of the triangles: the caller's, or — SceneLayout::triClassed — grouped by edge class (pttri.h), the caller's
// order kept inside a group, with the class begins as bytes in triClassPack; or — the mesh image — the kd order of the centroids.
// Returns triOrder[position] = original index.
inline std::vector<int> orderTriangles(const ptss_scene_desc& s, SceneLayout& L) {
    std::vector<int> triOrder((size_t)L.numTriangles), triCode((size_t)L.numTriangles, 0);
    for (int i = 0; i < L.numTriangles; ++i) {
        triOrder[(size_t)i] = i;
        const ptss_triangle& t = s.triangles[i];
        if (L.triClassed) triCode[(size_t)i] = pttri::triangleClass(t.vertex1 - t.vertex0, t.vertex2 - t.vertex0);   // the edges as stored (packTriangles)
    }
    std::stable_sort(triOrder.begin(), triOrder.end(), [&](int a, int b) { return triCode[(size_t)a] < triCode[(size_t)b]; });
    for (int code = 0, pos = 0; code <= 16 && L.triClassed; ++code) {
        while (pos < L.numTriangles && triCode[(size_t)triOrder[(size_t)pos]] < code) ++pos;
        L.triClassPack[code / 4] |= (uint32_t)pos << (8 * (code % 4));
    }
    if (ptss::meshImage(L)) {
        std::vector<Point> centroid((size_t)L.numTriangles);
        for (int i = 0; i < L.numTriangles; ++i) {
            const ptss_triangle& t = s.triangles[i];
            for (int a = 0; a < 3; ++a) {
                const float* v0 = &t.vertex0.x, *v1 = &t.vertex1.x, *v2 = &t.vertex2.x;
                centroid[(size_t)i][a] = (float)(((double)v0[a] + v1[a] + v2[a]) / 3);
            }
        }
        kdOrder(centroid, triOrder, 0, L.numTriangles, ptss::kMeshLeaf, ptss::kMeshLeaf * ptss::kMeshLeaf);
    }
    return triOrder;
}

// Sphere rows with their material, original-index and position tables. Returns order[row] = original index: the caller's order,
// or — many-sphere image — the spatial order, the last chunk padded with copies of the last sphere.
inline std::vector<int> packSpheres(const ptss_scene_desc& s, const SceneLayout& L, std::vector<Row>& blob) {
    const bool accel = L.accelSpheres != 0;
    const int sphereRows = sphereRowsOf(L);
    std::vector<int> order;
    if (accel) {
        order = spatialOrder(s);
        while ((int)order.size() < sphereRows) order.push_back(order.back());  // pad the last chunk with copies
    } else {
        order.resize(s.numSpheres);
        for (size_t i = 0; i < s.numSpheres; ++i) order[i] = (int)i;
    }
    for (int i = 0; i < sphereRows; ++i) {
        const ptss_sphere& sp = s.spheres[order[i]];
        // radius*radius is the same single rounding the reference performs per test (Primitives.h:113)
        blob[L.offSphere + i] = Row{sp.position.x, sp.position.y, sp.position.z, sp.radius * sp.radius};
        intsAt(blob, L.offSphereMat)[i] = sp.materialIdx;
        if (accel) intsAt(blob, L.offSphereOrig)[i] = order[i];
        if (accel && i < L.numSpheres) intsAt(blob, L.offSpherePos)[order[i]] = i;
    }
    return order;
}

// The chunks' bounding spheres, in double, rounded outwards (the derivation is at the top of this file).
inline void packChunkBounds(const ptss_scene_desc& s, const SceneLayout& L, const std::vector<int>& order, std::vector<Row>& blob) {
    for (int k = 0; k < L.numChunks; ++k) {
        // Centre: close to the smallest enclosing ball's (enclosingBall) — on the configs[4] scene the radii shrink by 8 % on
        // average (up to 18 %) against the mean of the members' centres, and a mid-bounce ray touches 3.95 instead of 4.67 bounds.
        const Ball ball = enclosingBall(s, &order[(size_t)k * ptss::kChunkSpheres], ptss::kChunkSpheres, 512);
        const float Cf[3] = {(float)ball.c[0], (float)ball.c[1], (float)ball.c[2]};
        double Rmax = 0;
        for (int j = 0; j < ptss::kChunkSpheres; ++j) {
            const ptss_sphere& sp = s.spheres[order[k * ptss::kChunkSpheres + j]];
            const double dx = (double)sp.position.x - Cf[0], dy = (double)sp.position.y - Cf[1], dz = (double)sp.position.z - Cf[2];
            Rmax = std::max(Rmax, std::sqrt(dx * dx + dy * dy + dz * dz) + std::fabs((double)sp.radius));
        }
        const double infl = Rmax * Rmax * (1 + kAccelM) * (1 + kAccelM) * (1 + kAccelM) * (1 + 4e-6) / (1 - (kAccelM + kAccelM * kAccelM)) * (1 + 1e-9);
        blob[L.offChunk + k] = Row{Cf[0], Cf[1], Cf[2], std::nextafter((float)infl, INFINITY)};
    }
}

// Triangle rows, normals and vertices in storage order, and the position of each original index.
inline void packTriangles(const ptss_scene_desc& s, const SceneLayout& L, const std::vector<int>& triOrder, std::vector<Row>& blob) {
    for (int pos = 0; pos < L.numTriangles; ++pos) {
        const int i = triOrder[(size_t)pos];
        const ptss_triangle& t = s.triangles[i];
        const vec3 e1 = t.vertex1 - t.vertex0;  // Primitives.h:34-35, hoisted (same subtraction, same bits)
        const vec3 e2 = t.vertex2 - t.vertex0;
        blob[L.offTri + 3 * pos + 0] = Row{t.vertex0.x, t.vertex0.y, t.vertex0.z, u2f((uint32_t)t.materialIdx)};
        blob[L.offTri + 3 * pos + 1] = Row{e1.x, e1.y, e1.z, u2f(0xfffffffeu - (uint32_t)i)};   // the low half of the closest hit's (distance, 0xFFFFFFFE - original index) key
        blob[L.offTri + 3 * pos + 2] = Row{e2.x, e2.y, e2.z, 0};
        blob[L.offTriNormal + 3 * pos + 0] = Row{t.normal0.x, t.normal0.y, t.normal0.z, 0};
        blob[L.offTriNormal + 3 * pos + 1] = Row{t.normal1.x, t.normal1.y, t.normal1.z, 0};
        blob[L.offTriNormal + 3 * pos + 2] = Row{t.normal2.x, t.normal2.y, t.normal2.z, 0};
        blob[L.offTriVert + 2 * pos + 0] = Row{t.vertex1.x, t.vertex1.y, t.vertex1.z, 0};
        blob[L.offTriVert + 2 * pos + 1] = Row{t.vertex2.x, t.vertex2.y, t.vertex2.z, 0};
        intsAt(blob, L.offTriPos)[i] = pos;
    }
}

// THE BOUNDS OF THE MESH IMAGE (ptmesh.h mayTouch). A bound may exclude a leaf only if the reference's float
// test (Primitives.h:25-83) cannot accept any of its triangles for the ray, at any distance > 0. Notation: u = 2^-24; the
// triangle as the test sees it is v0, v0 + e1, v0 + e2 with the STORED float edges; s = o - v0, q = d x e2, r = s x e1 and the
// exact det = e1 . q, n1 = s . q, n2 = d . r, nd = e2 . r, so that o + t d = v0 + b1 e1 + b2 e2 with t = nd / det, b1 = n1 / det,
// b2 = n2 / det exactly. Lmax: the longest side of any triangle of the bound; sigma >= |s| (|o - C| + R).
//  (1) Rounding of the test (ptmath.h dot = two fma over a product, cross = fma over a product, each correctly rounded; every
//      intermediate finite, meshEligible): |det_f - det| <= 9.1 u |e1||e2||d| <= eta = 12 u |d| Lmax^2, and the three
//      numerators are off by at most 10.2 u times the product of their factors' norms, bounded by 12 u |d| sigma Lmax
//      (n1, n2) and 12 u sigma Lmax^2 (nd). The camera-origin precomputes (primaryPrepKernel) are the same operations.
//  (2) Let D <= |det| be known. If D >= 4 eta then det_f = det (1 + theta), |theta| <= rho = eta / D <= 1/4: same sign.
//      inv = RN(1 / det_f) (rcp_in_range is the correctly rounded reciprocal on its range).
//      b1_f = RN(n1_f inv) "not < 0" means n1_f / det >= 0 (a negative product rounding to -0 is below 2^-148), so
//      b1 >= -d1 with d1 = 12 u |d| sigma Lmax / D; likewise b2 >= -d1. b0_f "not < 0" means RN(b1_f + b2_f) <= 1, so
//      b1_f + b2_f <= 1 + u, and b1 <= b1_f (1 + rho)(1 + 2.1 u) + d1: b0 = 1 - b1 - b2 >= -(1.01 rho + 3.2 u + 2 d1).
//      The negative parts of (b0, b1, b2) sum to at most 1.01 rho + 3.2 u + 4 d1, and a point whose weights sum to 1 with
//      negative parts summing to n lies within n Lmax of the triangle: X = o + t d is within
//      Lmax (1.01 rho + 3.2 u) + 48 u |d| sigma Lmax^2 / D of it.
//  (3) dist_f = RN(nd_f inv) > 0 means nd_f / det > 0, so t >= -12 u sigma Lmax^2 / D: the point o + max(t, 0) d of the
//      HALF line lies within 12 u |d| sigma Lmax^2 / D of X. (The limit `dist <= distance` is not used: any distance.)
//  So an accepted ray passes within infl = Lmax (4 u + 1.02 eta / D) + B sigma / D, B = 64 u |d| Lmax^2, of the ball.
//  (4) D: every unit normal lies in the double cone (a, alpha), so |det| = |d . (e1 x e2)| >= Nmin (|d . a| cos alpha -
//      |d| sin alpha); and an accepted triangle has |det_f| > 1e-7 (Primitives.h:41), so |det| >= 1e-7 - eta. D is the larger.
//      A direction for which D < 4 eta may graze a triangle so flatly that its computed weights say nothing about where it
//      passes: such a ray ENTERS the bound unconditionally — that is the |det|-dependent term the absolute epsilon needs.
//  (5) The kernel's float evaluation: |d| <= kDirNorm, 1 / |d|^2 <= kInvDir2 (the per-query unit-direction test), 2^-16
//      relative allowances on the squared distance, on sigma and on D, 2^-20 on the cone term (the axis rounded to float,
//      |d . a| rounded), 2^-10 on infl. Here, in double from the exact float inputs: C rounded to float and R measured from
//      it, rounded up; Nmin and cos alpha rounded down, Lmax, sin alpha and B up (ptmesh::buildBound).
// tests/test_mesh_bound.py pins the predicate on random, grazing (|det| swept down to 1e-7), shared-edge and far-origin rays,
// and shows that the same test fails for a bound with its inflation scaled down.
inline void packMeshBounds(const ptss_scene_desc& s, const SceneLayout& L, const std::vector<int>& triOrder, std::vector<Row>& blob) {
    auto boundOf = [&](int first, int count, Row* rows) {
        std::vector<float> tri((size_t)count * 9);
        for (int k = 0; k < count; ++k) {
            const ptss_triangle& t = s.triangles[triOrder[(size_t)(first + k)]];
            const vec3 e1 = t.vertex1 - t.vertex0, e2 = t.vertex2 - t.vertex0;   // as stored
            const float v[9] = {t.vertex0.x, t.vertex0.y, t.vertex0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z};
            std::copy(v, v + 9, tri.begin() + 9 * k);
        }
        float b[12];
        ptmesh::buildBound(tri.data(), count, b);
        for (int r = 0; r < 3; ++r) rows[r] = Row{b[4 * r], b[4 * r + 1], b[4 * r + 2], b[4 * r + 3]};
    };
    constexpr int kGroupTris = ptss::kMeshLeaf * ptss::kMeshLeaf;
    for (int k = 0; k < L.mesh.numLeaves; ++k)
        boundOf(k * ptss::kMeshLeaf, std::min(ptss::kMeshLeaf, L.numTriangles - k * ptss::kMeshLeaf), &blob[(size_t)(L.mesh.offLeaf + 3 * k)]);
    for (int g = 0; g < L.mesh.numGroups; ++g)
        boundOf(g * kGroupTris, std::min(kGroupTris, L.numTriangles - g * kGroupTris), &blob[(size_t)(L.mesh.offGroup + 3 * g)]);
}

// Material, point-light and area-light rows (after packTriangles: an area light names its two triangles by stored position).
inline void packMaterialsAndLights(const ptss_scene_desc& s, const SceneLayout& L, std::vector<Row>& blob) {
    for (int i = 0; i < L.numMaterials; ++i) {
        const ptss_material& m = s.materials[i];
        Row* o = &blob[L.offMaterial + 5 * i];
        o[0] = Row{m.diffuseColor.x, m.diffuseColor.y, m.diffuseColor.z, m.diffAvg};
        o[1] = Row{m.specularColor.x, m.specularColor.y, m.specularColor.z, m.specAvg};
        o[2] = Row{m.absorption.x, m.absorption.y, m.absorption.z, m.refrAvg};
        o[3] = Row{m.emmitance.x, m.emmitance.y, m.emmitance.z, m.roughness};
        o[4] = Row{m.specularExponent, m.indexOfRefraction, u2f((uint32_t)(unsigned char)m.flags), 0};
    }
    for (int i = 0; i < L.numPointLights; ++i) {
        const ptss_point_light& p = s.pointLights[i];
        blob[L.offPointLight + 2 * i + 0] = Row{p.position.x, p.position.y, p.position.z, 0};
        blob[L.offPointLight + 2 * i + 1] = Row{p.power.x, p.power.y, p.power.z, 0};
    }
    for (int i = 0; i < L.numAreaLights; ++i) {
        const ptss_area_light& a = s.areaLights[i];
        // getAreaLightPoint picks triangle triangleIdx or triangleIdx + 1 (CudaTracer.cu:408): both as stored positions
        const int* triPos = intsAt(blob, L.offTriPos);
        blob[L.offAreaLight + 2 * i] = Row{a.power.x, a.power.y, a.power.z, u2f((uint32_t)triPos[a.triangleIdx])};
        blob[L.offAreaLight + 2 * i + 1] = Row{u2f((uint32_t)triPos[a.triangleIdx + 1]), 0, 0, 0};
    }
}

// One image of a (validated) scene: accel — the many-sphere image, mesh — the mesh image, neither — the plain image.
inline void packScene(const ptss_scene_desc& s, SceneLayout& L, std::vector<Row>& blob, bool accel, bool mesh) {
    if (mesh) layoutMesh(s, L);
    else layoutPlain(s, accel, L);
    setFlags(s, L);
    const std::vector<int> triOrder = orderTriangles(s, L);
    blob.assign((size_t)L.totalVec4 + 1, Row{0, 0, 0, 0});
    ptq::build_thresholds(reinterpret_cast<float*>(&blob[L.offQuant]));
    const std::vector<int> sphereOrder = packSpheres(s, L, blob);
    packChunkBounds(s, L, sphereOrder, blob);
    packTriangles(s, L, triOrder, blob);
    if (mesh) packMeshBounds(s, L, triOrder, blob);
    packMaterialsAndLights(s, L, blob);
}

// ---- which images a scene gets ------------------------------------------------------------------------------------------------
// Scenes with many spheres get the chunked image (accelEligible), and the plain one as image 1 for cameras outside its range
// (cameraInRange); everySphereLoop keeps the plain one only. Scenes of many triangles and few spheres get the mesh image
// (meshEligible), which serves every camera (a query outside its derivation walks every triangle); everySphereLoop keeps the
// reference's loop over every triangle for them too.
struct ImagePlan {
    bool accel, mesh;
    int numImages;
};
inline ImagePlan planImages(const ptss_scene_desc& s, bool everySphereLoop) {
    const bool accel = accelEligible(s) && !everySphereLoop;
    const bool mesh = !accel && meshEligible(s) && !everySphereLoop;
    return ImagePlan{accel, mesh, accel ? 2 : 1};
}
struct PackedImage {
    SceneLayout layout{};
    std::vector<Row> blob;   // layout.totalVec4 + 1 rows
    // Scene access path: images that fit the default 64 KiB dynamic-LDS window are staged in LDS (north_star); larger ones
    // are read in place (wave-uniform scalar loads + per-lane gathers from global memory) — same kernel, same results, no
    // size limit. (On the 38-primitive "mixed" scene reading in place measured 16 % slower, profiles/README.md r01.)
    bool inLds = true;
};
// The one or two packed images of a (validated) scene. Throws std::bad_alloc when the host runs out of memory.
inline std::vector<PackedImage> packImages(const ptss_scene_desc& s, bool everySphereLoop) {
    const ImagePlan plan = planImages(s, everySphereLoop);
    std::vector<PackedImage> images((size_t)plan.numImages);
    for (int i = 0; i < plan.numImages; ++i) {
        packScene(s, images[(size_t)i].layout, images[(size_t)i].blob, plan.accel && i == 0, plan.mesh);
        images[(size_t)i].inLds = ptss::bounceLdsBytes(images[(size_t)i].layout, true) <= 64 * 1024;
    }
    return images;
}

// What is wrong with a scene description, or nullptr: the checks packScene relies on.
inline const char* validateScene(const ptss_scene_desc& s) {
    if ((s.numSpheres && !s.spheres) || (s.numTriangles && !s.triangles) || (s.numMaterials && !s.materials) ||
        (s.numPointLights && !s.pointLights) || (s.numAreaLights && !s.areaLights))
        return "scene: null array with non-zero count";
    for (size_t i = 0; i < s.numSpheres; ++i)
        if (s.spheres[i].materialIdx < 0 || (size_t)s.spheres[i].materialIdx >= s.numMaterials)
            return "scene: sphere materialIdx out of range";
    for (size_t i = 0; i < s.numTriangles; ++i)
        if (s.triangles[i].materialIdx < 0 || (size_t)s.triangles[i].materialIdx >= s.numMaterials)
            return "scene: triangle materialIdx out of range";
    for (size_t i = 0; i < s.numAreaLights; ++i)
        if (s.areaLights[i].triangleIdx < 0 || (size_t)s.areaLights[i].triangleIdx + 1 >= s.numTriangles)
            return "scene: area light needs triangles [triangleIdx, triangleIdx+1]";
    return nullptr;
}

}  // namespace ptpack
