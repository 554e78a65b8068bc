// ptss_api.hip — context management and the frame driver behind include/ptss.h.
//
// ptss_generate_frame is the reference's generateFrame (CudaTracer/CudaTracer.cu:587-647) with the
// host taken out of the inner loop: the per-bounce live-ray count stays on the device
// (FrameBuffers::counts), every bounce kernel is launched unconditionally and applies the
// reference's `numRays > 128` guard itself, so a frame is one uninterrupted stream of launches
// with at most one event wait at the end (cfg.syncEachFrame, the reference's :639-642).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "ptss.h"
#include "ptss_device.h"
#include <algorithm>
#include <array>
#include <cmath>
#include "ptquant.h"
#include "ptdenoise.h"
#include "ptreproject.h"
#include "ptmesh.h"
#include "pttri.h"

using namespace ptv;

#if PTSS_DIAG
namespace ptss { hipError_t readDiagCounters(unsigned long long* out8); }
#endif
namespace {

thread_local std::string g_detail;

int fail(int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess)
        snprintf(buf, sizeof(buf), "%s: %s (%s)", what, hipGetErrorString(e), hipGetErrorName(e));
    else
        snprintf(buf, sizeof(buf), "%s", what);
    g_detail = buf;
    return code;
}

#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return fail(PTSS_EHIP, #expr, _e); \
    } while (0)

#define RC_TRY(expr) do { if (int _rc = (expr)) return _rc; } while (0)   // a step that reports a PTSS_* code

struct EventPair {
    hipEvent_t a, b;
};

}  // namespace

// One ray population of the frame with its own pools, counters and stream (ptss_device.h, "frame lanes"). A context
// has 1..kMaxLanes of them; with one lane the caller's stream is used and nothing below differs from a single population.
struct Lane {
    hipStream_t stream = nullptr;            // own stream (contexts with several lanes only)
    float* dPool[2] = {nullptr, nullptr};
    uint32_t* dCounts[2] = {nullptr, nullptr};   // alternate per frame (flushKernel arms the other one)
    uint32_t* dShardCount0 = nullptr;
    uint32_t* dLastCounts = nullptr;         // counts of the frame before (flushKernel's copy)
    uint32_t* dDone = nullptr;               // done[countIndex(b, s)]: workgroups of shard s that ended a bounce-b kernel, all frames (never reset)
    uint32_t doneTarget[ptss::kMaxBounces + 1] = {};  // what done[b][*] add up to once everything launched so far has ended
                                             // (stored by this lane's bounce-b kernel as it starts: bounce b - 1 has then finished)
    hipEvent_t evDone[2] = {nullptr, nullptr};   // end of this lane's frame, by frame parity (several lanes only)
    uint32_t regionCap = 0;                  // slots per shard region of this lane's pools
    int maxBlocks = 0;                       // one 256-ray tile per workgroup over this lane's share of the frame
    // live-count hints: counts[] of a recent frame, read back asynchronously, size the next frames' grids
    uint32_t hint[ptss::kMaxBounces + 1] = {0};  // per bounce: the fullest shard's live count
    bool haveHint = false;
    uint32_t* hCounts = nullptr;  // pinned, 4 slots x kCountWords
    hipEvent_t hintEvent[4] = {nullptr, nullptr, nullptr, nullptr};
    bool hintPending[4] = {false, false, false, false};
};

// One packed scene (packScene) on the device, with how the frames use it.
struct SceneImage {
    float4* dBlob = nullptr;
    ptss::SceneLayout layout{};
    bool inLds = true;       // staged in LDS (true) or read through scalar loads (false)
    bool oneLaunch = false;  // the frame is traced by ONE launch (frameKernel)
};

struct ptss_context {
    ptss_render_config cfg{};
    hipStream_t stream = nullptr;
    ptss::TileMap tile{};
    // images[0]: the scene image the context was made for; images[1] (sphere acceleration on, else empty): the plain image,
    // for cameras outside the chunked image's range. The frames use images[active].
    SceneImage images[2];
    int active = 0;
    const SceneImage& image() const { return images[active]; }
    std::vector<Lane> lanes;
    hipEvent_t evFork = nullptr;            // several lanes: the caller's stream has reached this frame
    int countParity = 0;                    // which of a lane's two count buffers the next frame uses
    uint32_t* dRngHome = nullptr;
    unsigned long long* dTotal = nullptr;   // [0 .. kMaxLanes) ray-bounce totals per lane, [kMaxLanes]: records ptss_update_triangles
                                            // rejected (kRejectedWord), [kMaxLanes + 1 .. +8) unused, then one word: guard timeouts (must stay 0)
    uint32_t* dAccumOwned = nullptr;
    uint32_t* dAccum = nullptr;  // owned or bound
    float* dFsum = nullptr;
    uint32_t* dStaged = nullptr;  // S > 1: per-stream sample words of the current pass. Free-running lanes: TWO buffers, by frame parity —
                                  // the lanes of frame N + 1 already park samples while displayKernel of frame N (on the caller's stream,
                                  // behind the join) still adds up frame N's; a lane starts frame N + 2 only behind displayKernel of frame N
    bool stagedTwice = false;
    hipEvent_t evDisplay[2] = {nullptr, nullptr};   // displayKernel of the last frame of each parity has run (stagedTwice only)
    uint32_t capacity = 0, numPixels = 0;  // capacity: stride of the per-pixel planes (rngHome)
    uint32_t samples = 1;                    // cfg.samplesPerPass (sample lanes per pixel)
    bool cameraDirty = true;           // primary-ray precomputes must be refreshed
    float defaultColor[3] = {0, 0, 0};
    // ProgramData (CudaTracer.h:32-42)
    ptss_camera camera{};
    int lastResetTick = 0;
    int lastTicks = 0;
    unsigned maxIterations = 15;
    bool resetTicksThisFrame = true;
    bool usePathTracer = true;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    float lastMs = 0.0f;
    int gridCap = 0;             // workgroups per shard at most = 16 resident rounds of this scene's bounce kernel (0 = uncapped)
    unsigned frameIndex = 0;
    // bounce-kernel timing (cfg.timeKernels): every launch is bracketed by two events on ITS stream; a finished pair becomes
    // an interval [start, end) in ms since evEpoch. ptss_bounce_kernel_time reports the UNION of the intervals: with one lane
    // that is the sum of the launch durations, with several lanes (whose kernels overlap in time) the time during which at
    // least one bounce kernel was running — the figure a launch-time roofline needs.
    std::vector<EventPair> evFree, evBusy;
    std::vector<std::pair<double, double>> kernelSpans;
    hipEvent_t evEpoch = nullptr;
    unsigned int timeoutsSeen = 0;   // ptss_guard_timeouts value already reported as PTSS_ETIMEOUT
    unsigned long long launchedKernels = 0;   // bounce / frame kernel instantiations enqueued since ptss_create (ptss_launched_kernels)
    float4* dDenoise[2] = {nullptr, nullptr};   // ptss_denoise's ping-pong colour planes, allocated by its first call with levels >= 2
    int denoiseLastPlane = -1;                  // the plane the last non-final pass of the latest ptss_denoise wrote (-1: none), and its
    int denoiseLastLevel = -1;                  // level; on denoiseStream (ptss_read_denoise_plane)
    hipStream_t denoiseStream = nullptr;
    int numCUs = 0;                             // hipDeviceProp_t::multiProcessorCount of cfg.device (sceneState's launch caps)
    hipStream_t updateStream = nullptr;         // the stream of the latest ptss_update_triangles (its read-backs synchronise on it)
    bool updated = false;
};
constexpr int kTotalWords = ptss::kMaxLanes + 8 + 1;
constexpr int kRejectedWord = ptss::kMaxLanes;

namespace {

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
// (SceneLayout::sphereBounded, ptss_kernels.hip shiftInSphere<true>: r^2 well inside the normal range, no discriminant near overflow).
bool geometryBounded(const ptss_scene_desc& s) {
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
bool cameraInRange(const ptss_camera& cam) {
    auto ok = [](float v) { return std::fabs(v) <= kAccelLimit; };
    return ok(cam.position.x) && ok(cam.position.y) && ok(cam.position.z);
}

bool accelEligible(const ptss_scene_desc& s) { return s.numSpheres >= (size_t)kAccelMinSpheres && geometryBounded(s); }

// ---- the mesh image (SceneLayout::mesh) ---------------------------------------------------------------------
// Scenes of many triangles and few spheres: 512 triangles or more — every edge-classed scene (T <= 255) keeps its image, and so
// does every scene of the older test suites, the largest of which (tests/test_gpu_kernel_coverage.py, the in-place cases) holds
// 484 triangles —, fewer than kAccelMinSpheres spheres (those keep the sphere chunks), at most 2^20 triangles,
// and every vertex finite with |coordinate| <= 2^40 — which, with the kernels' per-query test |o|^2 < 2^80, |d|^2 = 1 +- 1e-5,
// keeps every intermediate of the reference's test finite: |det| <= |e1| |e2| |d| < 2^84, |e2 . r| <= |e2| |o - v0| |e1| < 2^126
// (so no NaN distance either), and the reciprocal inside its fast range.
constexpr int kMeshMinTriangles = 512;
constexpr size_t kMeshMaxTriangles = size_t(1) << 20;
bool meshEligible(const ptss_scene_desc& s) {
    if (s.numTriangles < (size_t)kMeshMinTriangles || s.numTriangles > kMeshMaxTriangles || s.numSpheres >= (size_t)kAccelMinSpheres) return false;
    auto ok = [](float v) { return std::fabs(v) <= 0x1p40f; };   // false for NaN and infinities
    for (size_t i = 0; i < s.numTriangles; ++i) {
        const ptss_triangle& t = s.triangles[i];
        for (const ptss_vec3* v : {&t.vertex0, &t.vertex1, &t.vertex2})
            if (!ok(v->x) || !ok(v->y) || !ok(v->z)) return false;
    }
    return true;
}
// stored position -> original index: kdSplit's scheme on the triangles' centroids, the cut placed at a multiple of kMeshLeaf^2
// while a part holds more than that and at a multiple of kMeshLeaf below, so that every kMeshLeaf consecutive positions are a
// leaf and every kMeshLeaf^2 a group. Ties by original index (a deterministic order); any permutation is legal, the closest hit
// being keyed by original index.
void meshSplit(const std::vector<std::array<float, 3>>& c, std::vector<int>& idx, int lo, int hi) {
    constexpr int kLeaf = ptss::kMeshLeaf, kGroup = ptss::kMeshLeaf * ptss::kMeshLeaf;
    const int n = hi - lo;
    if (n <= kLeaf) return;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lo; i < hi; ++i)
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], c[(size_t)idx[i]][a]);
            mx[a] = std::max(mx[a], c[(size_t)idx[i]][a]);
        }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
    const int unit = n > kGroup ? kGroup : kLeaf;
    int left = ((n / 2 + unit - 1) / unit) * unit;
    if (left >= n) left -= unit;
    if (left <= 0) return;
    std::nth_element(idx.begin() + lo, idx.begin() + lo + left, idx.begin() + hi, [&](int a, int b) {
        const float ka = c[(size_t)a][axis], kb = c[(size_t)b][axis];
        return ka < kb || (ka == kb && a < b);
    });
    meshSplit(c, idx, lo, lo + left);
    meshSplit(c, idx, lo + left, hi);
}

// sorted position -> original index. The spheres are split recursively at the median of their centres along the axis of
// largest extent (a kd-tree built by std::nth_element; ties by original index, so the order is deterministic), the cut
// placed at a multiple of 64 spheres while a part holds more than 64 and at a multiple of kChunkSpheres below that: every
// chunk of kChunkSpheres consecutive positions is a leaf and every 64 consecutive positions a subtree. Against round 1's
// Morton curve (whose jumps put far-apart spheres into one chunk) a ray of the configs[5] scene meets about half as many
// chunk bounds. Any permutation is legal here: the traversal decides ties by ORIGINAL index (offSphereOrig).
void kdSplit(const ptss_scene_desc& s, std::vector<int>& idx, int lo, int hi) {
    const int n = hi - lo;
    if (n <= ptss::kChunkSpheres) return;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = lo; i < hi; ++i) {
        const float c[3] = {s.spheres[idx[i]].position.x, s.spheres[idx[i]].position.y, s.spheres[idx[i]].position.z};
        for (int a = 0; a < 3; ++a) {
            mn[a] = std::min(mn[a], c[a]);
            mx[a] = std::max(mx[a], c[a]);
        }
    }
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
    const int unit = n > 64 ? 64 : ptss::kChunkSpheres;
    int left = ((n / 2 + unit - 1) / unit) * unit;  // spheres in the lower part: about half, a whole number of units
    if (left >= n) left -= unit;
    if (left <= 0) return;
    auto key = [&](int i) { return axis == 0 ? s.spheres[i].position.x : (axis == 1 ? s.spheres[i].position.y : s.spheres[i].position.z); };
    std::nth_element(idx.begin() + lo, idx.begin() + lo + left, idx.begin() + hi,
                     [&](int a, int b) { return key(a) < key(b) || (key(a) == key(b) && a < b); });
    kdSplit(s, idx, lo, lo + left);
    kdSplit(s, idx, lo + left, hi);
}
// A ball around n member spheres: from the mean of their centres, `steps` steps of "move towards the farthest point of the
// farthest member by 1 / (step + 1) of the way" (Badoiu-Clarkson), keeping the best centre seen — close to the smallest
// enclosing ball. Any centre is legal for a chunk bound: packScene measures R from the float centre it stores.
struct Ball {
    double c[3], r;
};
Ball enclosingBall(const ptss_scene_desc& s, const int* idx, int n, int steps) {
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
void refineChunks(const ptss_scene_desc& s, std::vector<int>& order) {
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
std::vector<int> spatialOrder(const ptss_scene_desc& s) {
    std::vector<int> order((size_t)s.numSpheres);
    for (size_t i = 0; i < s.numSpheres; ++i) order[i] = (int)i;
    kdSplit(s, order, 0, (int)s.numSpheres);
    refineChunks(s, order);
    return order;
}

void packScene(const ptss_scene_desc& s, ptss::SceneLayout& L, std::vector<float4>& blob, bool accel, bool mesh) {
    auto u2f = [](uint32_t u) { return __builtin_bit_cast(float, u); };
    L.accelSpheres = accel ? 1 : 0;
    L.numChunks = accel ? (int)((s.numSpheres + ptss::kChunkSpheres - 1) / ptss::kChunkSpheres) : 0;
    const int sphereRows = accel ? L.numChunks * ptss::kChunkSpheres : (int)s.numSpheres;
    L.numSpheres = (int)s.numSpheres;
    L.numTriangles = (int)s.numTriangles;
    L.numMaterials = (int)s.numMaterials;
    L.numPointLights = (int)s.numPointLights;
    L.numAreaLights = (int)s.numAreaLights;
    int off = 0;
    // plain image: sphere rows (and their camera-origin twins) padded to a multiple of four, zero-filled — the
    // candidate pass fetches four rows per trip and drops the padding's bits (sphereCandidates)
    const int sphereAlloc = accel ? sphereRows : (sphereRows + 3) / 4 * 4;
    L.offSphere = off;      off += sphereAlloc;
    if (!accel) { L.offSphereMat = off; off += (sphereRows + 3) / 4; }
    L.offChunk = off;       off += (L.numChunks + 3) / 4 * 4;   // bound rows padded to a multiple of four (zero rows: chunkMask drops their bits)
    const int numLeaves = mesh ? (L.numTriangles + ptss::kMeshLeaf - 1) / ptss::kMeshLeaf : 0;
    const int numGroups = (numLeaves + ptss::kMeshLeaf - 1) / ptss::kMeshLeaf;
    bool leavesInLds = false;
    int offGroup = 0, offLeaf = 0;   // (L.mesh shares its words with triClassPack, which is cleared below)
    if (mesh) {
        // Mesh image: group bounds, leaf bounds where they fit, spheres, materials, lights and the tone-map table are staged in
        // LDS; the triangle tables stay in global memory (read through `cold`) — T x 10 rows would not fit beyond ~400 triangles.
        offGroup = off;   off += 3 * ((numGroups + 3) / 4 * 4);   // padded to whole trips of four bounds (meshGroupMask drops their bits)
        const int leafRows = 3 * numLeaves;
        const int rest = 5 * L.numMaterials + 2 * L.numPointLights + 2 * L.numAreaLights + ptq::kTableFloats / 4 + sphereAlloc;
        ptss::SceneLayout probe{};
        probe.ldsVec4 = off + leafRows + rest;
        leavesInLds = ptss::bounceLdsBytes(probe, true) <= 64 * 1024;
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
    } else {
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
    }
    if (accel) {            // cold integer tables of the many-sphere image: global memory only
        L.offSphereMat = off;   off += (sphereRows + 3) / 4;
        L.offSphereOrig = off;  off += (sphereRows + 3) / 4;
        L.offSpherePos = off;   off += (L.numSpheres + 3) / 4;
    } else {
        L.offSphereOrig = L.offSpherePos = 0;
    }
    L.totalVec4 = off;
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
        const vec3 e1 = t.vertex1 - t.vertex0, e2 = t.vertex2 - t.vertex0;  // as stored below
        const double n1 = std::sqrt((double)e1.x * e1.x + (double)e1.y * e1.y + (double)e1.z * e1.z);
        const double n2 = std::sqrt((double)e2.x * e2.x + (double)e2.y * e2.y + (double)e2.z * e2.z);
        if (!(n1 * n2 <= 0x1p100)) L.triDetBounded = 0;  // false for NaN / infinite edges as well
    }
    // Storage order of the triangles: the caller's, or — SceneLayout::triClassed — grouped by edge class (pttri.h), the caller's
    // order kept inside a group. triOrder[position] = original index.
    L.triClassed = (L.triDetBounded && L.sphereBounded && L.numTriangles <= 255) ? 1 : 0;   // (the class bounds travel as bytes)
    std::vector<int> triOrder((size_t)L.numTriangles), triCode((size_t)L.numTriangles, 0);
    for (int i = 0; i < L.numTriangles; ++i) {
        triOrder[(size_t)i] = i;
        const ptss_triangle& t = s.triangles[i];
        if (L.triClassed) triCode[(size_t)i] = pttri::triangleClass(t.vertex1 - t.vertex0, t.vertex2 - t.vertex0);   // the edges as stored below
    }
    std::stable_sort(triOrder.begin(), triOrder.end(), [&](int a, int b) { return triCode[(size_t)a] < triCode[(size_t)b]; });
    for (int k = 0; k < 5; ++k) L.triClassPack[k] = 0u;
    for (int code = 0, pos = 0; code <= 16 && L.triClassed; ++code) {
        while (pos < L.numTriangles && triCode[(size_t)triOrder[(size_t)pos]] < code) ++pos;
        L.triClassPack[code / 4] |= (uint32_t)pos << (8 * (code % 4));
    }
    if (mesh) {   // (T >= 512: never classed, so the union holds the mesh dimensions)
        std::vector<std::array<float, 3>> centroid((size_t)L.numTriangles);
        for (int i = 0; i < L.numTriangles; ++i) {
            const ptss_triangle& t = s.triangles[i];
            for (int a = 0; a < 3; ++a) {
                const float* v0 = &t.vertex0.x, *v1 = &t.vertex1.x, *v2 = &t.vertex2.x;
                centroid[(size_t)i][a] = (float)(((double)v0[a] + v1[a] + v2[a]) / 3);
            }
        }
        meshSplit(centroid, triOrder, 0, L.numTriangles);
        L.mesh.numLeaves = numLeaves;
        L.mesh.numGroups = numGroups;
        L.mesh.offGroup = offGroup;
        L.mesh.offLeaf = offLeaf;
        L.mesh.reserved = 0;
    }
    blob.assign((size_t)off + 1, float4{0, 0, 0, 0});
    ptq::build_thresholds(reinterpret_cast<float*>(&blob[L.offQuant]));
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
        blob[L.offSphere + i] = float4{sp.position.x, sp.position.y, sp.position.z, sp.radius * sp.radius};
        reinterpret_cast<int*>(&blob[L.offSphereMat])[i] = sp.materialIdx;
        if (accel) reinterpret_cast<int*>(&blob[L.offSphereOrig])[i] = order[i];
        if (accel && i < L.numSpheres) reinterpret_cast<int*>(&blob[L.offSpherePos])[order[i]] = i;
    }
    for (int k = 0; k < L.numChunks; ++k) {  // bounding sphere of the chunk, in double, rounded outwards
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
        blob[L.offChunk + k] = float4{Cf[0], Cf[1], Cf[2], std::nextafter((float)infl, INFINITY)};
    }
    for (int pos = 0; pos < L.numTriangles; ++pos) {
        const int i = triOrder[(size_t)pos];
        const ptss_triangle& t = s.triangles[i];
        const vec3 e1 = t.vertex1 - t.vertex0;  // Primitives.h:34-35, hoisted (same subtraction, same bits)
        const vec3 e2 = t.vertex2 - t.vertex0;
        blob[L.offTri + 3 * pos + 0] = float4{t.vertex0.x, t.vertex0.y, t.vertex0.z, u2f((uint32_t)t.materialIdx)};
        blob[L.offTri + 3 * pos + 1] = float4{e1.x, e1.y, e1.z, u2f(0xfffffffeu - (uint32_t)i)};   // the low half of the closest hit's (distance, 0xFFFFFFFE - original index) key
        blob[L.offTri + 3 * pos + 2] = float4{e2.x, e2.y, e2.z, 0};
        blob[L.offTriNormal + 3 * pos + 0] = float4{t.normal0.x, t.normal0.y, t.normal0.z, 0};
        blob[L.offTriNormal + 3 * pos + 1] = float4{t.normal1.x, t.normal1.y, t.normal1.z, 0};
        blob[L.offTriNormal + 3 * pos + 2] = float4{t.normal2.x, t.normal2.y, t.normal2.z, 0};
        blob[L.offTriVert + 2 * pos + 0] = float4{t.vertex1.x, t.vertex1.y, t.vertex1.z, 0};
        blob[L.offTriVert + 2 * pos + 1] = float4{t.vertex2.x, t.vertex2.y, t.vertex2.z, 0};
        reinterpret_cast<int*>(&blob[L.offTriPos])[i] = pos;
    }
    if (mesh) {
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
        auto boundOf = [&](int first, int count, float4* rows) {
            std::vector<float> tri((size_t)count * 9);
            for (int k = 0; k < count; ++k) {
                const ptss_triangle& t = s.triangles[triOrder[(size_t)(first + k)]];
                const vec3 e1 = t.vertex1 - t.vertex0, e2 = t.vertex2 - t.vertex0;   // as stored
                const float v[9] = {t.vertex0.x, t.vertex0.y, t.vertex0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z};
                std::copy(v, v + 9, tri.begin() + 9 * k);
            }
            float b[12];
            ptmesh::buildBound(tri.data(), count, b);
            for (int r = 0; r < 3; ++r) rows[r] = float4{b[4 * r], b[4 * r + 1], b[4 * r + 2], b[4 * r + 3]};
        };
        constexpr int kGroupTris = ptss::kMeshLeaf * ptss::kMeshLeaf;
        for (int k = 0; k < numLeaves; ++k)
            boundOf(k * ptss::kMeshLeaf, std::min(ptss::kMeshLeaf, L.numTriangles - k * ptss::kMeshLeaf), &blob[(size_t)(L.mesh.offLeaf + 3 * k)]);
        for (int g = 0; g < numGroups; ++g)
            boundOf(g * kGroupTris, std::min(kGroupTris, L.numTriangles - g * kGroupTris), &blob[(size_t)(L.mesh.offGroup + 3 * g)]);
    }
    for (int i = 0; i < L.numMaterials; ++i) {
        const ptss_material& m = s.materials[i];
        float4* o = &blob[L.offMaterial + 5 * i];
        o[0] = float4{m.diffuseColor.x, m.diffuseColor.y, m.diffuseColor.z, m.diffAvg};
        o[1] = float4{m.specularColor.x, m.specularColor.y, m.specularColor.z, m.specAvg};
        o[2] = float4{m.absorption.x, m.absorption.y, m.absorption.z, m.refrAvg};
        o[3] = float4{m.emmitance.x, m.emmitance.y, m.emmitance.z, m.roughness};
        o[4] = float4{m.specularExponent, m.indexOfRefraction, u2f((uint32_t)(unsigned char)m.flags), 0};
    }
    for (int i = 0; i < L.numPointLights; ++i) {
        const ptss_point_light& p = s.pointLights[i];
        blob[L.offPointLight + 2 * i + 0] = float4{p.position.x, p.position.y, p.position.z, 0};
        blob[L.offPointLight + 2 * i + 1] = float4{p.power.x, p.power.y, p.power.z, 0};
    }
    for (int i = 0; i < L.numAreaLights; ++i) {
        const ptss_area_light& a = s.areaLights[i];
        // getAreaLightPoint picks triangle triangleIdx or triangleIdx + 1 (CudaTracer.cu:408): both as stored positions
        const int* triPos = reinterpret_cast<const int*>(&blob[L.offTriPos]);
        blob[L.offAreaLight + 2 * i] = float4{a.power.x, a.power.y, a.power.z, u2f((uint32_t)triPos[a.triangleIdx])};
        blob[L.offAreaLight + 2 * i + 1] = float4{u2f((uint32_t)triPos[a.triangleIdx + 1]), 0, 0, 0};
    }
}

int validateScene(const ptss_scene_desc& s) {
    if ((s.numSpheres && !s.spheres) || (s.numTriangles && !s.triangles) || (s.numMaterials && !s.materials) ||
        (s.numPointLights && !s.pointLights) || (s.numAreaLights && !s.areaLights))
        return fail(PTSS_EINVAL, "scene: null array with non-zero count");
    for (size_t i = 0; i < s.numSpheres; ++i)
        if (s.spheres[i].materialIdx < 0 || (size_t)s.spheres[i].materialIdx >= s.numMaterials)
            return fail(PTSS_EINVAL, "scene: sphere materialIdx out of range");
    for (size_t i = 0; i < s.numTriangles; ++i)
        if (s.triangles[i].materialIdx < 0 || (size_t)s.triangles[i].materialIdx >= s.numMaterials)
            return fail(PTSS_EINVAL, "scene: triangle materialIdx out of range");
    for (size_t i = 0; i < s.numAreaLights; ++i)
        if (s.areaLights[i].triangleIdx < 0 || (size_t)s.areaLights[i].triangleIdx + 1 >= s.numTriangles)
            return fail(PTSS_EINVAL, "scene: area light needs triangles [triangleIdx, triangleIdx+1]");
    return PTSS_OK;
}

// rows of the frame this context owns: bands of cfg.bandRows rows, dealt round-robin to the tileWorld ranks
int localRows(const ptss_render_config& cfg) {
    int rows = 0;
    for (int y = 0; y < cfg.height; ++y)
        if ((y / cfg.bandRows) % cfg.tileWorld == cfg.tileRank) ++rows;
    return rows;
}

// ptss_create's failures: PTSS_ENOMEM when the device ran out of memory, PTSS_EHIP for any other HIP error
int createCheck(hipError_t e, const char* what) { return e == hipSuccess ? PTSS_OK : fail(e == hipErrorOutOfMemory ? PTSS_ENOMEM : PTSS_EHIP, what, e); }
#define ALLOC_TRY(expr) RC_TRY(createCheck((expr), #expr))
template <class T>
hipError_t mallocZeroed(T** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? hipMemset(*p, 0, bytes) : e;
}

// ---- the scene-dependent part of a context (ptss_create and ptss_set_scene) ------------------------------------------------------
// Which images the scene gets, their blobs on the device, how the frames read each of them, and the launch caps that follow.
// Everything else a context owns — pools, random streams, accumulator, counters — does not depend on the scene.
struct SceneState {
    SceneImage images[2];
    int gridCap = 0;
    float defaultColor[3] = {0, 0, 0};
};
void releaseSceneState(SceneState& st) {
    for (SceneImage& im : st.images) {
        (void)hipFree(im.dBlob);
        im = SceneImage{};
    }
}
// Fills `st` (empty on entry) or leaves nothing allocated. numLanes, maxBlocks0: the context's lanes and lane 0's widest grid.
int buildSceneState(const ptss_scene_desc& scene, const ptss_render_config& cfg, int numLanes, int maxBlocks0, int numCUs, SceneState& st) {
    // Scenes with many spheres get the chunked image (see accelEligible / packScene), and the plain one as images[1] for cameras
    // outside its range; cfg.everySphereLoop keeps the plain one only. Scenes of many triangles and few spheres get the mesh image
    // (meshEligible), which serves every camera (a query outside its derivation walks every triangle); everySphereLoop keeps the
    // reference's loop over every triangle for them too.
    const bool wantAccel = accelEligible(scene) && !cfg.everySphereLoop;
    const bool wantMesh = !wantAccel && meshEligible(scene) && !cfg.everySphereLoop;
    const int numImages = wantAccel ? 2 : 1;
    std::vector<float4> blob[2];
    try {
        for (int i = 0; i < numImages; ++i) {
            SceneImage& im = st.images[i];
            packScene(scene, im.layout, blob[i], wantAccel && i == 0, wantMesh);
            // Scene access path: images that fit the default 64 KiB dynamic-LDS window are staged in LDS (north_star); larger ones
            // are read in place (wave-uniform scalar loads + per-lane gathers from global memory) — same kernel, same results, no
            // size limit. (On the 38-primitive "mixed" scene reading in place measured 16 % slower, profiles/README.md r01.)
            im.inLds = ptss::bounceLdsBytes(im.layout, true) <= 64 * 1024;
        }
    } catch (const std::bad_alloc&) {
        return fail(PTSS_ENOMEM, "scene image (host)");
    }
    for (int i = 0; i < numImages; ++i) {
        hipError_t e = hipMalloc(&st.images[i].dBlob, blob[i].size() * sizeof(float4));
        if (e == hipSuccess) e = hipMemcpy(st.images[i].dBlob, blob[i].data(), blob[i].size() * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            releaseSceneState(st);
            return createCheck(e, "scene image (device)");
        }
    }
    st.defaultColor[0] = scene.defaultColor.x;
    st.defaultColor[1] = scene.defaultColor.y;
    st.defaultColor[2] = scene.defaultColor.z;
    // Launches wider than 16 resident rounds stop growing: a workgroup then walks several tiles and stages the scene
    // into LDS once for all of them. One round = CUs x workgroups per CU of THIS scene's bounce kernel (LDS image and
    // register budget decide: 7 for the 38-primitive scenes, 3-4 for the many-sphere image), so 16 rounds =
    // CUs x perCU workgroups per shard (kShards = 16 shards). Measured on the mixed scene (256 x 7 = 1,792 per shard):
    // 448: -4.6 %, 896: -1.3 %, 1,280-3,584: equal, uncapped: -2 % (profiles/README.md).
    const SceneImage& primary = st.images[0];   // (not recomputed when the frames switch to images[1])
    const int perCU = ptss::bounceOccupancyBlocksPerCU(primary.layout, primary.inLds, primary.layout.sphereBounded != 0);
    st.gridCap = numCUs * (perCU > 0 ? perCU : 4) * 16 / ptss::kShards;
    // One launch per frame (ptss_kernels.hip frameKernel): only when every workgroup of the frame's grid is resident at once —
    // its workgroups wait for each other — i.e. bounce-0 tiles <= CUs x resident workgroups per CU of THAT kernel with this
    // scene's LDS image. The occupancy API over-reports by one workgroup per CU for kernels of more than 96 SGPRs
    // (MI355X_MICROARCH.md, "Residency and cooperative launch"): one is kept in reserve. One lane, scene staged in LDS.
    // A bounded image runs the bounded or the unbounded frame kernel, as the camera is in range or not: both must fit.
    auto qualifies = [&](const SceneImage& im) {
        if (cfg.oneLaunchFrames <= 0 || numLanes != 1 || !im.inLds) return false;   // opt-in (include/ptss.h)
        if (ptss::meshImage(im.layout)) return false;   // the mesh image has no frame kernel
        int perCU = ptss::frameOccupancyBlocksPerCU(im.layout, false);
        if (im.layout.sphereBounded) perCU = std::min(perCU, ptss::frameOccupancyBlocksPerCU(im.layout, true));
        const int resident = perCU - 1;
        return resident >= 1 && maxBlocks0 <= numCUs * resident;
    };
    for (int i = 0; i < numImages; ++i) st.images[i].oneLaunch = qualifies(st.images[i]);
#ifdef PTSS_TUNING_KNOBS   // measurement builds only (tools/build_variants.py "knobs"); the shipped library reads no environment
    if (const char* e = getenv("PTSS_SCENE_PATH")) {
        if (!strcmp(e, "scalar"))
            for (int i = 0; i < numImages; ++i) st.images[i].inLds = false;
    }
    if (const char* e = getenv("PTSS_GRID_CAP")) st.gridCap = atoi(e);
#endif
    return PTSS_OK;
}
void adoptSceneState(ptss_context* c, const SceneState& st) {
    for (int i = 0; i < 2; ++i) c->images[i] = st.images[i];
    c->gridCap = st.gridCap;
    for (int k = 0; k < 3; ++k) c->defaultColor[k] = st.defaultColor[k];
    c->active = 0;
}

// A lane's device resources (ptss_create). releaseLane frees whatever of them exists: ptss_destroy, also after a failed create.
int allocLane(Lane& ln, const uint32_t (&shardCount0)[ptss::kShards], bool ownStream) {
    const size_t poolBytes = (size_t)ptss::kRayPlanes * ln.regionCap * ptss::kShards * sizeof(float);
    for (float*& pool : ln.dPool) ALLOC_TRY(hipMalloc(&pool, poolBytes));
    for (uint32_t*& counts : ln.dCounts) ALLOC_TRY(mallocZeroed(&counts, ptss::kCountWords * sizeof(uint32_t)));
    ALLOC_TRY(mallocZeroed(&ln.dLastCounts, ptss::kCountWords * sizeof(uint32_t)));
    for (int s = 0; s < ptss::kShards; ++s)  // arm bounce 0 of the first frame (flushKernel arms every later one)
        ALLOC_TRY(hipMemcpy(ln.dCounts[0] + ptss::countIndex(0, s), &shardCount0[s], sizeof(uint32_t), hipMemcpyHostToDevice));
    ALLOC_TRY(hipMalloc(&ln.dShardCount0, sizeof(shardCount0)));
    ALLOC_TRY(hipMemcpy(ln.dShardCount0, shardCount0, sizeof(shardCount0), hipMemcpyHostToDevice));
    ALLOC_TRY(mallocZeroed(&ln.dDone, (ptss::kCountWords + ptss::kCountStride) * sizeof(uint32_t)));  // + the finished-frames counter
    if (ownStream) {
        ALLOC_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
        for (hipEvent_t& ev : ln.evDone) ALLOC_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    ALLOC_TRY(hipHostMalloc(&ln.hCounts, 4 * ptss::kCountWords * sizeof(uint32_t), hipHostMallocDefault));
    for (hipEvent_t& ev : ln.hintEvent) ALLOC_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    return PTSS_OK;
}
#undef ALLOC_TRY

// curandSetupKernel (CudaTracer.cu:722-724): per-pixel subsequence via the 2^67 jump table, on stream st; returns once it has run
// (ptss_create, ptss_reseed)
hipError_t seedStreams(ptss_context* c, unsigned long long seed, hipStream_t st) {
    std::vector<uint32_t> table(ptrng::kJumpTableWords);
    ptrng::build_subsequence_table(table.data());
    uint32_t* dTable = nullptr;
    hipError_t e = hipMalloc(&dTable, table.size() * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    e = hipMemcpy(dTable, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && c->numPixels > 0) e = ptss::launchRngInit(st, c->dRngHome, c->capacity, c->samples, c->tile, seed, dTable);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dTable);
    return e;
}

// everything this context has enqueued on its own streams has run (ptss_set_scene, ptss_reseed)
int quiesce(ptss_context* c) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Lane& ln : c->lanes)
        if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
    return PTSS_OK;
}

void releaseLane(Lane& ln) {
    for (hipEvent_t ev : ln.hintEvent)
        if (ev) (void)hipEventDestroy(ev);
    if (ln.hCounts) (void)hipHostFree(ln.hCounts);
    (void)hipFree(ln.dDone);
    for (hipEvent_t ev : ln.evDone)
        if (ev) (void)hipEventDestroy(ev);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
    for (float* pool : ln.dPool) (void)hipFree(pool);
    for (uint32_t* counts : ln.dCounts) (void)hipFree(counts);
    (void)hipFree(ln.dShardCount0);
    (void)hipFree(ln.dLastCounts);
}

ptss::FrameBuffers frameBuffers(const ptss_context* c, int laneIdx, ptss_uchar4* pixels, int sample) {
    const Lane& ln = c->lanes[(size_t)laneIdx];
    ptss::FrameBuffers fb{};
    fb.pool[0] = ln.dPool[0];
    fb.pool[1] = ln.dPool[1];
    fb.rngHome = c->dRngHome;
    fb.counts = ln.dCounts[c->countParity];
    fb.countsNext = ln.dCounts[1 - c->countParity];
    fb.shardCount0 = ln.dShardCount0;
    fb.lastCounts = ln.dLastCounts;
    fb.totalRayBounces = c->dTotal + laneIdx;
    fb.guardTimeouts = reinterpret_cast<uint32_t*>(c->dTotal + ptss::kMaxLanes + 8);
    fb.accum = c->dAccum;
    fb.fsum = c->dFsum;
    fb.staged = c->dStaged ? c->dStaged + (c->stagedTwice ? (size_t)(c->frameIndex & 1u) * c->capacity * c->samples : 0) : nullptr;
    fb.quantTable = reinterpret_cast<const float*>(c->image().dBlob + c->image().layout.offQuant);
    fb.pixels = pixels;
    fb.regionCap = ln.regionCap;
    fb.numPixels = c->numPixels;
    fb.plane = c->capacity;
    fb.samples = c->samples;
    fb.firstTiles = c->samples * (c->capacity / ptss::kBlock);
    // The reference stops bouncing once <= 128 rays are live IN THE WHOLE FRAME (CudaTracer.cu:622). A
    // shard of a multi-GPU frame cannot know the frame-wide count without a collective per bounce, so a context with
    // tileWorld > 1 never stops early; the two agree whenever the frame-wide count stays above 128. (The lanes of ONE
    // context do know each other's counts: the guard is exact for any number of lanes.)
    fb.minLive = c->tile.world > 1 ? 0u : ptss::kMinLiveRays;
    fb.inverseTicks = 1.f / (float)((int)c->samples * (sample + 1));  // CudaTracer.cu:94 (S = 1: 1.f / (ticks + 1))
    fb.defaultColor[0] = c->defaultColor[0];
    fb.defaultColor[1] = c->defaultColor[1];
    fb.defaultColor[2] = c->defaultColor[2];
    fb.laneIndex = (uint32_t)laneIdx;
    fb.laneCount = (uint32_t)c->lanes.size();
    fb.frameRays = c->numPixels * c->samples;
    fb.numPeers = fb.laneCount - 1;
    fb.myDone = ln.dDone;
    fb.myFrameDone = ln.dDone + ptss::kCountWords;
    fb.frameSeq = c->frameIndex;
    fb.joinsFrame = (laneIdx + 1 == (int)c->lanes.size()) ? 1u : 0u;
    uint32_t p = 0;
    for (size_t k = 0; k < c->lanes.size(); ++k) {
        if ((int)k == laneIdx) continue;
        fb.peerCounts[p] = c->lanes[k].dCounts[c->countParity];
        fb.peerDone[p] = c->lanes[k].dDone;
        fb.peerFrameDone[p] = c->lanes[k].dDone + ptss::kCountWords;
        ++p;
    }
    return fb;
}

void drainKernelEvents(ptss_context* c, bool wait) {
    size_t k = 0;
    for (size_t i = 0; i < c->evBusy.size(); ++i) {
        EventPair p = c->evBusy[i];
        hipError_t q = wait ? hipEventSynchronize(p.b) : hipEventQuery(p.b);
        if (q == hipSuccess) {
            float start = 0, ms = 0;   // start since the epoch (coarse at large values), duration from the pair itself (exact)
            if (hipEventElapsedTime(&start, c->evEpoch, p.a) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess)
            {
                if (c->kernelSpans.size() >= (1u << 20)) c->kernelSpans.clear();   // nobody is asking (ptss_bounce_kernel_time empties it)
                c->kernelSpans.emplace_back((double)start, (double)start + (double)ms);
            }
            c->evFree.push_back(p);
        } else {
            c->evBusy[k++] = p;
        }
    }
    c->evBusy.resize(k);
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is not an error
}

// Frame lanes: did a lane give up waiting for a peer since the last check (FrameBuffers::guardTimeouts)? Called by the
// entry points that have just synchronised; one 4-byte read-back, and only in contexts with more than one lane.
int checkLaneTimeouts(ptss_context* c) {
    if (c->lanes.size() < 2 && !c->images[0].oneLaunch && !c->images[1].oneLaunch) return PTSS_OK;   // only kernels that wait for others can time out
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, c->dTotal + ptss::kMaxLanes + 8, sizeof(v), hipMemcpyDeviceToHost));
    if (v != c->timeoutsSeen) {
        c->timeoutsSeen = v;
        return fail(PTSS_ETIMEOUT, "a bounded wait on the device expired (a frame lane for a peer lane, or a workgroup of the one-launch "
                                   "frame kernel for its shard): the frame was not traced as specified");
    }
    return PTSS_OK;
}

// ---- the steps of a frame (ptss_generate_frame) ------------------------------------------------------------------------
// The chunked image assumes a camera within the geometry's magnitude range (packScene): outside it the frames use the plain one.
void selectImage(ptss_context* c) {
    if (!c->images[1].dBlob) return;
    const int want = cameraInRange(c->camera) ? 0 : 1;
    if (want != c->active) {
        c->active = want;
        c->cameraDirty = true;
    }
}

ptss::EyeParams eyeParams(const ptss_context* c) {   // {camera, s (CudaTracer.cu:334), aspect, invW, invH}
    return {c->camera, -2 * ptm::tan(c->camera.fieldOfView * 0.5f), (float)c->tile.height / (float)c->tile.width, 1.0f / c->tile.width,
            1.0f / c->tile.height};
}

// harvest the newest finished live-count readbacks (never blocks)
void harvestHints(ptss_context* c) {
    for (Lane& ln : c->lanes)
        for (int q = 0; q < 4; ++q) {
            if (!ln.hintPending[q] || hipEventQuery(ln.hintEvent[q]) != hipSuccess) continue;
            const uint32_t* src = ln.hCounts + (size_t)q * ptss::kCountWords;
            for (int b = 0; b <= ptss::kMaxBounces; ++b) {
                uint32_t mx = 0;
                for (int s = 0; s < ptss::kShards; ++s) mx = std::max(mx, src[ptss::countIndex(b, s)]);
                ln.hint[b] = mx;
            }
            ln.haveHint = true;
            ln.hintPending[q] = false;
        }
    (void)hipGetLastError();
}

// Several lanes: each runs on its own stream, forked from the caller's here and joined into it by flushAndJoin; their
// launches are issued round-robin, bounce by bounce, so that the streams advance together.
// STRICT ordering (the default): every frame forks, so the lanes start behind whatever the caller put on its stream
// before this call — a reader of the previous frame's pixels or accumulator, a zero-fill, a newly bound buffer's writer.
// FREE-RUNNING (cfg.lanesFreeRun, opt-in): the fork happens only when the library's own work on the caller's stream
// requires it (the clear of a reset, the camera precomputes) — otherwise a lane's next frame depends on nothing but
// its own previous one, and the lanes run on, frame after frame, while the caller's stream merely waits for each
// frame's end (the join); the caller has promised not to touch the buffers in between (include/ptss.h).
int forkLanes(ptss_context* c, bool forkNeeded) {
    if (c->lanes.size() > 1 && (forkNeeded || c->frameIndex == 0 || !c->cfg.lanesFreeRun)) {
        HIP_TRY(hipEventRecord(c->evFork, c->stream));
        for (Lane& ln : c->lanes) HIP_TRY(hipStreamWaitEvent(ln.stream, c->evFork, 0));
    }
    // Free-running lanes with S > 1: this frame parks its samples in the buffer of its parity, which displayKernel of the frame
    // two back (same parity, on the caller's stream) must have emptied — the only thing a free-running lane ever waits for
    // on the caller's side, and an event that has nearly always fired by now.
    if (c->stagedTwice && c->frameIndex >= 2)
        for (Lane& ln : c->lanes) HIP_TRY(hipStreamWaitEvent(ln.stream, c->evDisplay[c->frameIndex & 1u], 0));
    return PTSS_OK;
}

// cfg.timeKernels: brackets the one kernel that launch() enqueues on stream s with an event pair (drainKernelEvents)
template <class Launch>
int timedLaunch(ptss_context* c, hipStream_t s, Launch launch) {
    if (!c->cfg.timeKernels) return launch();
    EventPair ev{nullptr, nullptr};
    if (c->evFree.empty() && c->evBusy.size() >= 4096) drainKernelEvents(c, true);
    if (c->evFree.empty()) {
        HIP_TRY(hipEventCreate(&ev.a));
        HIP_TRY(hipEventCreate(&ev.b));
    } else {
        ev = c->evFree.back();
        c->evFree.pop_back();
    }
    HIP_TRY(hipEventRecord(ev.a, s));
    RC_TRY(launch());
    HIP_TRY(hipEventRecord(ev.b, s));
    c->evBusy.push_back(ev);
    return PTSS_OK;
}

// every bounce in ONE launch (frameKernel): CudaTracer.cu:622-633 without leaving the device; its grid is the frame's tiles
int traceOneLaunch(ptss_context* c, const ptss::FrameBuffers& fb, int numIterations, bool bounded, const ptss::EyeParams& eye) {
    const SceneImage& im = c->image();
    return timedLaunch(c, c->stream, [&] {
        HIP_TRY(ptss::launchFrame(c->stream, fb, im.dBlob, im.layout, numIterations, bounded, c->lanes[0].maxBlocks, c->tile, eye,
                                          &c->launchedKernels));
        return PTSS_OK;
    });
}

// one launch per bounce and lane (CudaTracer.cu:622-633, guard evaluated on the device), the lanes round-robin inside a bounce
int traceBounces(ptss_context* c, ptss::FrameBuffers* fbs, int numIterations, bool bounded, const ptss::EyeParams& eye) {
    const SceneImage& im = c->image();
    const int K = (int)c->lanes.size();
    for (int i = 0; i < numIterations; ++i)
        for (int k = 0; k < K; ++k) {
            Lane& ln = c->lanes[(size_t)k];
            const hipStream_t ls = K > 1 ? ln.stream : c->stream;
            // grid: one tile per workgroup for the expected live count (+1.5 %), never more than the lane's share of the
            // frame; the kernel grid-strides, so a low hint costs time, not correctness
            int blocks = ln.maxBlocks;
            if (i > 0 && ln.haveHint) {
                // tiles for the fullest shard (+1.5 %), times kShards (workgroup b serves shard b % kShards)
                const unsigned long long tilesPerShard = ((unsigned long long)ln.hint[i] * 65 / 64 + ptss::kBlock) / ptss::kBlock + 1;
                const unsigned long long want = tilesPerShard * ptss::kShards;
                if (want < (unsigned long long)blocks) blocks = (int)want;
            }
            // launches wider than 16 resident rounds stop growing (gridCap, ptss_create)
            if (c->gridCap > 0 && c->gridCap * ptss::kShards < blocks) blocks = c->gridCap * ptss::kShards;
            // the peers' done totals once their bounce i - 1 of this frame has ended (all of those launches precede this
            // one in host order, so a kernel that waits for them never waits for something behind it in a shared queue)
            if (i > 0)
                for (int j = 0, p = 0; j < K; ++j)
                    if (j != k) fbs[k].peerTarget[p++] = c->lanes[(size_t)j].doneTarget[i - 1];
            RC_TRY(timedLaunch(c, ls, [&] {
                HIP_TRY(ptss::launchBounce(ls, fbs[k], im.dBlob, im.layout, i, i == numIterations - 1, im.inLds, bounded, blocks, c->tile, eye,
                                               &c->launchedKernels));
                return PTSS_OK;
            }));
            ln.doneTarget[i] += (uint32_t)blocks;  // every workgroup of the launch adds 1 to done[i][its shard] as it ends
        }
    return PTSS_OK;
}

// flushKernel of every lane (CudaTracer.cu:637), the live-count readbacks for later grids, and the join into the caller's stream
int flushAndJoin(ptss_context* c, const ptss::FrameBuffers* fbs, int numIterations) {
    const int K = (int)c->lanes.size();
    for (int k = 0; k < K; ++k) {
        Lane& ln = c->lanes[(size_t)k];
        const hipStream_t ls = K > 1 ? ln.stream : c->stream;
        // (flushKernel itself waits, on the device, until every peer lane has finished the previous frame: FrameBuffers::myFrameDone)
        ptss::FlushTargets targets{};
        for (int j = 0, p = 0; j < K; ++j)
            if (j != k) {
                for (int b = 0; b <= ptss::kMaxBounces; ++b) targets.target[p][b] = c->lanes[(size_t)j].doneTarget[b];
                ++p;
            }
        HIP_TRY(ptss::launchFlush(ls, fbs[k], numIterations, targets));
        // every 8th frame (and until a hint exists) copy counts[] to pinned memory for later grid sizing
        if (!ln.haveHint || (c->frameIndex & 7u) == 0) {
            const int q = (int)((c->frameIndex >> 3) & 3u);
            if (!ln.hintPending[q]) {
                HIP_TRY(hipMemcpyAsync(ln.hCounts + (size_t)q * ptss::kCountWords, ln.dLastCounts, ptss::kCountWords * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, ls));
                HIP_TRY(hipEventRecord(ln.hintEvent[q], ls));
                ln.hintPending[q] = true;
            }
        }
        // the join: the caller's stream is ordered behind every lane's frame (the lanes themselves run on) — ONE event, behind
        // the last lane's flushKernel, which ends only when every other lane's has (FrameBuffers::joinsFrame); an event per lane cost 1-2 %
        if (K > 1 && k == K - 1) {
            HIP_TRY(hipEventRecord(ln.evDone[c->frameIndex & 1u], ls));
            HIP_TRY(hipStreamWaitEvent(c->stream, ln.evDone[c->frameIndex & 1u], 0));
        }
    }
    return PTSS_OK;
}

}  // namespace

extern "C" {

int ptss_version(void) { return PTSS_VERSION; }

const char* ptss_error_string(int code) {
    switch (code) {
        case PTSS_OK: return "ok";
        case PTSS_EINVAL: return "invalid argument";
        case PTSS_EHIP: return "HIP runtime error";
        case PTSS_ENODEVICE: return "no usable HIP device";
        case PTSS_ENOMEM: return "out of memory";
        case PTSS_ERANGE: return "buffer too small or index out of range";
        case PTSS_ETIMEOUT: return "a frame lane timed out waiting for a peer lane";
        default: return "unknown error";
    }
}

const char* ptss_last_error_detail(void) { return g_detail.c_str(); }

int ptss_default_config(ptss_render_config* cfg) {
    if (!cfg) return fail(PTSS_EINVAL, "cfg is null");
    memset(cfg, 0, sizeof(*cfg));
    cfg->structSize = (unsigned int)sizeof(*cfg);
    cfg->width = 512;  // DIM, CudaUtils.h:7
    cfg->height = 512;
    cfg->seed = 0x5EEDull;
    cfg->maxIterations = 15;  // CudaTracer.h:39
    cfg->device = 0;
    cfg->tileRank = 0;
    cfg->tileWorld = 1;
    cfg->bandRows = 8;
    cfg->syncEachFrame = 1;
    cfg->floatAccumulator = 0;
    cfg->timeKernels = 0;
    cfg->samplesPerPass = 1;
    cfg->everySphereLoop = 0;
    cfg->frameLanes = 0;
    cfg->lanesFreeRun = 0;
    cfg->oneLaunchFrames = 0;
    return PTSS_OK;
}

int ptss_create(const ptss_scene_desc* scene, const ptss_render_config* cfg, ptss_context** out) {
    if (!scene || !cfg || !out) return fail(PTSS_EINVAL, "null argument");
    if (cfg->structSize != (unsigned int)sizeof(ptss_render_config))
        return fail(PTSS_EINVAL, "cfg->structSize is not this library's sizeof(ptss_render_config): the caller was built against another "
                                 "ptss.h (compare ptss_version() with PTSS_VERSION) or did not start from ptss_default_config");
    if (cfg->width <= 0 || cfg->height <= 0 || (long long)cfg->width * cfg->height > (1ll << 31) - 256)
        return fail(PTSS_EINVAL, "bad frame size");
    if (cfg->maxIterations == 0 || cfg->maxIterations > (unsigned)ptss::kMaxBounces)
        return fail(PTSS_EINVAL, "maxIterations must be in [1, 64]");
    if (cfg->tileWorld <= 0 || cfg->tileRank < 0 || cfg->tileRank >= cfg->tileWorld || cfg->bandRows <= 0)
        return fail(PTSS_EINVAL, "bad tile spec");
    const int spp = cfg->samplesPerPass == 0 ? 1 : cfg->samplesPerPass;
    if (spp < 1 || spp > 64) return fail(PTSS_EINVAL, "samplesPerPass must be in [1, 64]");
    if ((long long)cfg->width * cfg->height >= (1ll << 26)) return fail(PTSS_EINVAL, "frame too large (>= 2^26 pixels)");
    {
        // A ray's word inside its shard's region is addressed in 32 bits (slotWord: 19 planes per block): the rays of one
        // pass — local pixels x sample lanes, rounded up to whole tiles per shard — must stay below 2^32 / 19 (~226
        // million; the whole pool may be larger than 4 GB, regions are based with 64-bit arithmetic).
        const long long rows = localRows(*cfg);
        const unsigned long long rays = ((unsigned long long)cfg->width * rows + 255ull) / 256ull * 256ull * (unsigned long long)spp;
        if ((rays + (unsigned long long)ptss::kShards * ptss::kBlock) * ptss::kRayPlanes >= (1ull << 32))
            return fail(PTSS_EINVAL, "too many rays per pass: width x local rows x samplesPerPass must stay below ~226 million");
    }
    int rc = validateScene(*scene);
    if (rc != PTSS_OK) return rc;

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(PTSS_ENODEVICE, "hipGetDeviceCount found no device (libptss has no CPU path)", e);
    }
    if (cfg->device < 0 || cfg->device >= ndev) return fail(PTSS_ENODEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(cfg->device));

    ptss_context* c = new (std::nothrow) ptss_context();
    if (!c) return fail(PTSS_ENOMEM, "context");
    c->cfg = *cfg;
    c->maxIterations = cfg->maxIterations;
    c->samples = (uint32_t)spp;
    // Camera(), RenderStructs.h:51-52
    c->camera.rotation = q4(1, 0, 0, 0);
    c->camera.position = v3(0, 0, 0);
    c->camera.zNear = -0.1f;
    c->camera.zFar = -100.0f;
    c->camera.fieldOfView = ptm::kPi / 2.0f;

    c->tile = ptss::TileMap{cfg->width, cfg->height, localRows(*cfg), cfg->tileRank, cfg->tileWorld, cfg->bandRows};
    c->numPixels = (uint32_t)cfg->width * (uint32_t)c->tile.localRows;
    const uint32_t gran = ptss::kBlock > 256 ? (uint32_t)ptss::kBlock : 256u;  // pixel planes are whole tiles
    c->capacity = ((c->numPixels + gran - 1) / gran) * gran;
    if (c->capacity == 0) c->capacity = gran;
    // Frame lanes (ptss_device.h): cfg.frameLanes, or by the size of a pass when 0 — launch-shaped passes (a few
    // resident rounds per launch) gain a fifth from a second lane, wide ones nothing.
    int numLanes = cfg->frameLanes;
    if (numLanes < 0 || numLanes > ptss::kMaxLanes) return (delete c, fail(PTSS_EINVAL, "frameLanes must be in [0, 4]"));
    {
        const unsigned long long rays = (unsigned long long)c->numPixels * c->samples;
        // measured (tools/lanes_bench.py / tools/s1_modes.py, Mrays/s with 1 / 2 lanes, one sample per tick, with the lanes coupled on
        // the device — flushKernel's finished-frames counters): 1920x1080 (2.1 M rays per pass) 13,800 / 16,300; 3840x2160, 1,024 spheres
        // (8.3 M) 4,110 / 4,360 (three lanes 4,580, four 3,470); 1280x720 (0.92 M) 10,010 / 11,160; 1024x576 (0.59 M) 8,050 / 9,090;
        // 800x600 (0.48 M) 7,490 / 7,900; 640x480 (0.31 M) 5,480 / 5,380; 512x512 (0.26 M) 4,730 / 4,570 — below ~0.2 ms a pass is ten launch
        // latencies, nothing to overlap; 1920x1080 S = 40 (83 M) 17,760 / 17,750. Four lanes (five streams with the caller's) share
        // hardware queues and serialise. (With the lanes coupled through stream events the gain at 1280x720 was inside the noise.)
        // All of that is the FREE-RUNNING mode (cfg.lanesFreeRun); ordered strictly on the caller's stream — a fork and a join per
        // frame — two lanes ran at 13,180 against one lane's 13,800, so the library's own choice is then one lane.
        // Round 3, wide passes again (tools/lanes_large.py, interleaved, twice): 3840x2160 S = 4, 12 bounces, 1,024 spheres (33 M rays per
        // pass, the late bounces a hundredth of that) 5,958-5,970 / 6,077; 1920x1080 S = 40 (83 M) 18,273-18,294 / 18,420-18,454: a second
        // lane is worth +2.0 % / +0.8 % there. The rule stays at 2^24 all the same: a caller who wants it asks for frameLanes = 2; by
        // default a wide pass keeps one lane, one set of pools (the second doubles 5-16 GB) and launches that do not overlap, so that
        // a kernel's duration means the same in a profile and in ptss_bounce_kernel_time.
        if (numLanes == 0) numLanes = (cfg->lanesFreeRun && rays >= (3ull << 17) && rays <= (1ull << 24)) ? 2 : 1;
    }
    c->lanes.resize((size_t)numLanes);
    uint32_t shardCount0[ptss::kMaxLanes][ptss::kShards] = {{0}};
    {
        // bounce 0 walks S sample planes of `capacity` pixels (capacity = numPixels rounded up to a tile); tile t belongs
        // to shard t % kShards and to round t / kShards, round R to lane R % numLanes
        const uint32_t tilesPerPlane = c->capacity / ptss::kBlock;
        const uint32_t tiles = tilesPerPlane * c->samples;
        const uint32_t rounds = (tiles + ptss::kShards - 1) / ptss::kShards;
        for (int k = 0; k < numLanes; ++k) {
            const uint32_t laneRounds = (rounds + (uint32_t)numLanes - 1 - (uint32_t)k) / (uint32_t)numLanes;
            c->lanes[(size_t)k].regionCap = (laneRounds ? laneRounds : 1) * ptss::kBlock;
            c->lanes[(size_t)k].maxBlocks = (int)(c->lanes[(size_t)k].regionCap / ptss::kBlock) * ptss::kShards;
        }
        for (uint32_t t = 0; t < tiles; ++t) {
            const uint32_t first = (t % tilesPerPlane) * ptss::kBlock;  // first pixel of the tile inside its plane
            uint32_t cnt = 0;
            if (first < c->numPixels) cnt = c->numPixels - first < (uint32_t)ptss::kBlock ? c->numPixels - first : (uint32_t)ptss::kBlock;
            shardCount0[(t / ptss::kShards) % (uint32_t)numLanes][t % ptss::kShards] += cnt;
        }
    }

#define CREATE_TRY(expr) do { if (int _rc = createCheck((expr), #expr)) return (ptss_destroy(c), _rc); } while (0)   // frees what exists

    {
        hipDeviceProp_t prop;
        CREATE_TRY(hipGetDeviceProperties(&prop, cfg->device));
        c->numCUs = prop.multiProcessorCount;
        SceneState st;
        if (int sceneRc = buildSceneState(*scene, *cfg, numLanes, c->lanes[0].maxBlocks, c->numCUs, st)) return (ptss_destroy(c), sceneRc);
        adoptSceneState(c, st);
    }
    CREATE_TRY(hipMalloc(&c->dRngHome, (size_t)ptss::kHomeWords * c->capacity * c->samples * sizeof(uint32_t)));
    for (int k = 0; k < numLanes; ++k)
        if (int laneRc = allocLane(c->lanes[(size_t)k], shardCount0[k], numLanes > 1)) return (ptss_destroy(c), laneRc);
    if (numLanes > 1) CREATE_TRY(hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));
    CREATE_TRY(mallocZeroed(&c->dTotal, kTotalWords * sizeof(unsigned long long)));
    CREATE_TRY(mallocZeroed(&c->dAccumOwned, (size_t)3 * c->capacity * sizeof(uint32_t)));
    c->dAccum = c->dAccumOwned;
    if (cfg->floatAccumulator) CREATE_TRY(mallocZeroed(&c->dFsum, (size_t)3 * c->capacity * c->samples * sizeof(float)));
    if (c->samples > 1) {
        c->stagedTwice = numLanes > 1 && cfg->lanesFreeRun != 0;
        const size_t words = (size_t)c->capacity * c->samples * (c->stagedTwice ? 2 : 1);
        CREATE_TRY(mallocZeroed(&c->dStaged, words * sizeof(uint32_t)));
        if (c->stagedTwice)
            for (int q = 0; q < 2; ++q) CREATE_TRY(hipEventCreateWithFlags(&c->evDisplay[q], hipEventDisableTiming));
    }
    CREATE_TRY(hipEventCreate(&c->evStart));
    CREATE_TRY(hipEventCreate(&c->evStop));
    CREATE_TRY(hipEventCreate(&c->evEpoch));

    CREATE_TRY(seedStreams(c, cfg->seed, nullptr));
    CREATE_TRY(hipEventRecord(c->evEpoch, nullptr));
    CREATE_TRY(hipDeviceSynchronize());

#undef CREATE_TRY

    *out = c;
    return PTSS_OK;
}

int ptss_destroy(ptss_context* c) {
    if (!c) return PTSS_OK;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize();
    drainKernelEvents(c, true);
    for (EventPair& p : c->evFree) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (Lane& ln : c->lanes) releaseLane(ln);
    for (hipEvent_t ev : {c->evFork, c->evDisplay[0], c->evDisplay[1], c->evStart, c->evStop, c->evEpoch})
        if (ev) (void)hipEventDestroy(ev);
    for (SceneImage& im : c->images) (void)hipFree(im.dBlob);
    (void)hipFree(c->dRngHome);
    (void)hipFree(c->dTotal);
    (void)hipFree(c->dAccumOwned);
    (void)hipFree(c->dFsum);
    (void)hipFree(c->dStaged);
    for (float4* plane : c->dDenoise) (void)hipFree(plane);
    delete c;
    return PTSS_OK;
}

int ptss_generate_frame(ptss_context* c, ptss_uchar4* pixels, int ticks) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    hipStream_t st = c->stream;
    HIP_TRY(hipSetDevice(c->cfg.device));  // contexts of several devices may live in one thread
    c->lastTicks = ticks;
    if (c->numPixels == 0) {  // a rank whose tile is empty (more ranks than row bands): nothing to render
        if (c->resetTicksThisFrame) c->lastResetTick = ticks;
        c->resetTicksThisFrame = false;
        c->lastMs = 0.0f;
        return PTSS_OK;
    }

    selectImage(c);
    bool forkNeeded = false;
    if (c->resetTicksThisFrame) {  // CudaTracer.cu:602-608
        forkNeeded = true;
        c->lastResetTick = ticks;
        HIP_TRY(ptss::launchClear(st, frameBuffers(c, 0, pixels, 0)));
        c->resetTicksThisFrame = false;
    }
    const int sample = ticks - c->lastResetTick;
    const int K = (int)c->lanes.size();
    ptss::FrameBuffers fbs[ptss::kMaxLanes];
    for (int k = 0; k < K; ++k) fbs[k] = frameBuffers(c, k, pixels, sample);

    if (c->cfg.syncEachFrame) HIP_TRY(hipEventRecord(c->evStart, st));  // :611

    const int numIterations = c->usePathTracer ? (int)c->maxIterations : 1;  // :620
    const ptss::EyeParams eye = eyeParams(c);
    if (c->cameraDirty) {  // origin-only parts of the primary-ray tests (computeEyeRaysKernel :614 itself is fused into bounce 0)
        forkNeeded = true;
        HIP_TRY(ptss::launchPrimaryPrep(st, c->image().dBlob, c->image().layout, c->camera.position));
        c->cameraDirty = false;
    }
    harvestHints(c);
    RC_TRY(forkLanes(c, forkNeeded));
    if (c->cfg.timeKernels) drainKernelEvents(c, false);
    // the shorter sphere candidate test: bounded geometry AND a camera within the same range (ray origins are the camera or points on primitives)
    const bool bounded = c->image().layout.sphereBounded != 0 && cameraInRange(c->camera);
    RC_TRY(c->image().oneLaunch && K == 1 ? traceOneLaunch(c, fbs[0], numIterations, bounded, eye) : traceBounces(c, fbs, numIterations, bounded, eye));
    RC_TRY(flushAndJoin(c, fbs, numIterations));
    if (c->samples > 1) {
        HIP_TRY(ptss::launchDisplay(st, fbs[0]));  // S > 1: add the pass's staged samples, then the display value
        if (c->stagedTwice) HIP_TRY(hipEventRecord(c->evDisplay[c->frameIndex & 1u], st));
    }
    c->countParity ^= 1;
    c->frameIndex++;

    if (c->cfg.syncEachFrame) {  // :639-642
        HIP_TRY(hipEventRecord(c->evStop, st));
        HIP_TRY(hipEventSynchronize(c->evStop));
        HIP_TRY(hipEventElapsedTime(&c->lastMs, c->evStart, c->evStop));
        // (a 4-byte read-back per frame: only where several lanes wait for each other; a one-launch context is checked by
        // ptss_synchronize and the ptss_read_* calls — its frames are a third of a millisecond)
        return c->lanes.size() > 1 ? checkLaneTimeouts(c) : PTSS_OK;
    }
    return PTSS_OK;
}

int ptss_set_camera(ptss_context* c, const ptss_camera* camera) {
    if (!c || !camera) return fail(PTSS_EINVAL, "null argument");
    c->camera = *camera;
    c->cameraDirty = true;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_get_camera(const ptss_context* c, ptss_camera* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->camera;
    return PTSS_OK;
}

int ptss_request_reset(ptss_context* c) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_set_mode(ptss_context* c, int usePathTracer) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->usePathTracer = usePathTracer != 0;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_set_max_iterations(ptss_context* c, unsigned int maxIterations) {
    if (!c || maxIterations == 0 || maxIterations > (unsigned)ptss::kMaxBounces)
        return fail(PTSS_EINVAL, "maxIterations must be in [1, 64]");
    c->maxIterations = maxIterations;
    return PTSS_OK;
}

int ptss_set_stream(ptss_context* c, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->stream = (hipStream_t)hipStream;
    return PTSS_OK;
}

int ptss_bind_accumulator(ptss_context* c, uint32_t* dev) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    c->dAccum = dev ? dev : c->dAccumOwned;
    return PTSS_OK;
}

int ptss_accumulator_devptr(ptss_context* c, uint32_t** out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->dAccum;
    return PTSS_OK;
}

int ptss_float_accumulator_devptr(ptss_context* c, float** out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->dFsum;
    return PTSS_OK;
}

int ptss_alloc_pixels(ptss_context* c, ptss_uchar4** out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipMalloc(out, (size_t)c->capacity * sizeof(ptss_uchar4)));
    HIP_TRY(hipMemset(*out, 0, (size_t)c->capacity * sizeof(ptss_uchar4)));
    return PTSS_OK;
}

int ptss_free_pixels(ptss_context* c, ptss_uchar4* dev) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    HIP_TRY(hipFree(dev));
    return PTSS_OK;
}

int ptss_local_pixels(const ptss_context* c, size_t* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->numPixels;
    return PTSS_OK;
}

int ptss_local_rows(const ptss_context* c, int* rows, int cap, int* count) {
    if (!c || !count) return fail(PTSS_EINVAL, "null argument");
    int n = 0;
    for (int y = 0; y < c->tile.height; ++y) {
        if ((y / c->tile.bandRows) % c->tile.world != c->tile.rank) continue;
        if (rows) {
            if (n >= cap) return fail(PTSS_ERANGE, "rows[] too small");
            rows[n] = y;
        }
        ++n;
    }
    *count = n;
    return PTSS_OK;
}

int ptss_synchronize(ptss_context* c) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return checkLaneTimeouts(c);
}

int ptss_read_accumulator(ptss_context* c, uint32_t* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    if (count != (size_t)3 * c->numPixels) return fail(PTSS_ERANGE, "count must be 3 * local pixels");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host, c->dAccum, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return checkLaneTimeouts(c);
}

int ptss_read_float_accumulator(ptss_context* c, float* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    if (!c->dFsum) return fail(PTSS_EINVAL, "context was created without floatAccumulator");
    if (count != (size_t)3 * c->numPixels) return fail(PTSS_ERANGE, "count must be 3 * local pixels");
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->samples == 1) {
        HIP_TRY(hipMemcpy(host, c->dFsum, count * sizeof(float), hipMemcpyDeviceToHost));
    } else {  // per-stream sums, added in lane order 0..S-1 (a fixed order: reproducible, and what the oracle does)
        std::vector<float> lane(count);
        for (size_t k = 0; k < count; ++k) host[k] = 0.0f;
        for (uint32_t l = 0; l < c->samples; ++l) {
            HIP_TRY(hipMemcpy(lane.data(), c->dFsum + (size_t)3 * l * c->capacity, count * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t k = 0; k < count; ++k) host[k] = host[k] + lane[k];
        }
    }
    return checkLaneTimeouts(c);
}

int ptss_read_pixels(ptss_context* c, const ptss_uchar4* dev, ptss_uchar4* host, size_t count) {
    if (!c || !dev || !host) return fail(PTSS_EINVAL, "null argument");
    if (count > c->numPixels) return fail(PTSS_ERANGE, "count exceeds local pixels");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host, dev, count * sizeof(ptss_uchar4), hipMemcpyDeviceToHost));
    return checkLaneTimeouts(c);
}

int ptss_read_rng_state(ptss_context* c, size_t local_pixel, uint32_t* out6) { return ptss_read_rng_state_lane(c, local_pixel, 0, out6); }

int ptss_read_rng_state_lane(ptss_context* c, size_t local_pixel, unsigned int lane, uint32_t* out6) {
    if (!c || !out6) return fail(PTSS_EINVAL, "null argument");
    if (local_pixel >= c->numPixels || lane >= c->samples) return fail(PTSS_ERANGE, "pixel or lane out of range");
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out6, c->dRngHome + (size_t)ptss::kHomeWords * ((size_t)lane * c->capacity + local_pixel), 6 * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_last_pass_ms(ptss_context* c, float* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->lastMs;
    return PTSS_OK;
}

int ptss_samples_since_reset(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->resetTicksThisFrame ? 0 : (c->lastTicks - c->lastResetTick + 1) * (int)c->samples;
    return PTSS_OK;
}

int ptss_live_counts(ptss_context* c, uint32_t* out, int cap, int* n) {
    if (!c || !out || !n) return fail(PTSS_EINVAL, "null argument");
    const int numIterations = c->usePathTracer ? (int)c->maxIterations : 1;
    if (cap < numIterations) return fail(PTSS_ERANGE, "out[] too small");
    std::vector<uint32_t> raw(ptss::kCountWords), sum(ptss::kCountWords, 0u);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Lane& ln : c->lanes) {  // the frame's count = its lanes' counts added up
        HIP_TRY(hipMemcpy(raw.data(), ln.dLastCounts, raw.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < raw.size(); ++k) sum[k] += raw[k];
    }
    // a bounce whose input is <= 128 rays did not run (CudaTracer.cu:622): report 0 from there on
    bool stopped = false;
    for (int i = 0; i < numIterations; ++i) {
        uint32_t total = 0;
        for (int s = 0; s < ptss::kShards; ++s) total += sum[ptss::countIndex(i, s)];
        if (total <= (c->tile.world > 1 ? 0u : ptss::kMinLiveRays)) stopped = true;
        out[i] = stopped ? 0u : total;
    }
    *n = numIterations;
    return checkLaneTimeouts(c);
}

int ptss_total_ray_bounces(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long perLane[ptss::kMaxLanes];
    HIP_TRY(hipMemcpy(perLane, c->dTotal, sizeof(perLane), hipMemcpyDeviceToHost));
    *out = 0;
    for (size_t k = 0; k < c->lanes.size(); ++k) *out += perLane[k];
    return checkLaneTimeouts(c);
}

int ptss_guard_timeouts(ptss_context* c, unsigned int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, c->dTotal + ptss::kMaxLanes + 8, sizeof(v), hipMemcpyDeviceToHost));
    *out = v;
    return PTSS_OK;
}

int ptss_one_launch_frames(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = (c->image().oneLaunch && c->lanes.size() == 1) ? 1 : 0;
    return PTSS_OK;
}

int ptss_frame_lanes(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = (int)c->lanes.size();
    return PTSS_OK;
}

int ptss_launched_kernels(const ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    *out = c->launchedKernels;
    return PTSS_OK;
}

// ptss_intersect / ptss_occluded: the context's own scene image (images[0]; the query kernel is exact on every image, so the
// camera's range plays no part), no frame state, the caller's stream
static int rayQuery(ptss_context* c, bool any, const ptss_ray_query* rays, void* out, size_t n, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (n == 0) return PTSS_OK;
    if (!rays || !out) return fail(PTSS_EINVAL, "null buffer with n > 0");
    if (n >= (size_t(1) << 31)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (((uintptr_t)rays | (uintptr_t)out) & (any ? 3u : 15u) || (uintptr_t)rays & 15u)
        return fail(PTSS_EINVAL, "rays and hits must be 16-byte aligned, verdicts 4-byte aligned");
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = hipStream ? static_cast<hipStream_t>(hipStream) : c->stream;
    HIP_TRY(ptss::launchQuery(st, any, im.dBlob, im.layout, im.inLds, rays, out, (uint32_t)n, c->gridCap * ptss::kShards,
                              &c->launchedKernels));
    return PTSS_OK;
}

int ptss_intersect(ptss_context* c, const ptss_ray_query* dev_rays, ptss_ray_hit* dev_hits, size_t n, void* hipStream) {
    return rayQuery(c, false, dev_rays, dev_hits, n, hipStream);
}

int ptss_occluded(ptss_context* c, const ptss_ray_query* dev_rays, uint32_t* dev_occluded, size_t n, void* hipStream) {
    return rayQuery(c, true, dev_rays, dev_occluded, n, hipStream);
}

// ptss_render_features: the scene image the queries use (images[0], exact for every camera), the context's CURRENT camera, no frame state
int ptss_render_features(ptss_context* c, ptss_pixel_feature* dev_features, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features) return fail(PTSS_EINVAL, "dev_features is null");
    if ((uintptr_t)dev_features & 15u) return fail(PTSS_EINVAL, "dev_features must be 16-byte aligned");
    if (c->numPixels == 0) return PTSS_OK;   // a rank whose tile is empty
    const SceneImage& im = c->images[0];
    if (!im.dBlob) return fail(PTSS_EINVAL, "context has no scene image");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = hipStream ? static_cast<hipStream_t>(hipStream) : c->stream;
    const ptss_vec3 defaultColor{c->defaultColor[0], c->defaultColor[1], c->defaultColor[2]};
    HIP_TRY(ptss::launchFeatures(st, im.dBlob, im.layout, im.inLds, c->tile, eyeParams(c), defaultColor, dev_features, c->numPixels,
                                 c->gridCap * ptss::kShards, &c->launchedKernels));
    return PTSS_OK;
}

int ptss_default_denoise_params(ptss_denoise_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(*p);
    p->levels = 5;
    p->sigmaColor = 64.0f;
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.0f;
    return PTSS_OK;
}

// ptss_denoise / ptss_denoise_history: the passes over the context's integer accumulator (fromAccumulator) or over `input`, a plane of
// float4 colours
static int denoisePasses(ptss_context* c, const char* what, const void* input, bool fromAccumulator, const ptss_pixel_feature* dev_features,
                         const ptss_denoise_params* params, ptss_uchar4* dev_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features || !params || !dev_out || (!fromAccumulator && !input)) return fail(PTSS_EINVAL, "null argument");
    if (params->structSize != (unsigned int)sizeof(ptss_denoise_params))
        return fail(PTSS_EINVAL, "params->structSize is not this library's sizeof(ptss_denoise_params): start from ptss_default_denoise_params");
    if (params->levels < 0 || params->levels > PTSS_DENOISE_MAX_LEVELS) return fail(PTSS_EINVAL, "levels must be in [0, 6]");
    if (!(params->sigmaColor > 0.0f) || !(params->sigmaNormal > 0.0f) || !(params->sigmaDepth >= 0.0f))
        return fail(PTSS_EINVAL, "sigmaColor and sigmaNormal must be positive, sigmaDepth not negative");
    if (((uintptr_t)dev_features & 15u) || ((uintptr_t)dev_out & 3u)) return fail(PTSS_EINVAL, "dev_features must be 16-byte aligned, dev_out 4-byte aligned");
    if (!fromAccumulator && ((uintptr_t)input & 15u)) return fail(PTSS_EINVAL, "dev_history must be 16-byte aligned");
    if (c->tile.world > 1)
        return fail(PTSS_EINVAL, (std::string(what) + " needs the whole frame: this context is a pixel-band shard (tileWorld > 1), whose bands of "
                                                       "rows have no neighbours to filter with").c_str());
    if (fromAccumulator) input = c->dAccum;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = hipStream ? static_cast<hipStream_t>(hipStream) : c->stream;
    const int levels = params->levels;
    if (levels >= 2)
        for (float4*& plane : c->dDenoise)
            if (!plane) {
                const hipError_t e = hipMalloc(&plane, (size_t)c->numPixels * sizeof(float4));
                if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PTSS_ENOMEM : PTSS_EHIP, "ptss_denoise: colour planes", e);
            }
    // the display value's scale: displayKernel's / finishPath's inverseTicks of the last frame (frameBuffers)
    const float inverseTicks = 1.f / (float)((int)c->samples * (c->lastTicks - c->lastResetTick + 1));
    const int width = c->tile.width, height = c->tile.height;
    c->denoiseLastPlane = levels >= 2 ? (levels - 2) & 1 : -1;
    c->denoiseLastLevel = levels - 2;
    c->denoiseStream = st;
    for (int i = 0; i < (levels > 0 ? levels : 1); ++i) {
        const bool first = i == 0, last = i + 1 >= levels;
        const void* src = first ? input : c->dDenoise[(i - 1) & 1];
        void* dst = last ? static_cast<void*>(dev_out) : c->dDenoise[i & 1];
        HIP_TRY(ptss::launchDenoise(st, first && fromAccumulator, last, src, dst, dev_features, width, height, ptdn::levelOf(*params, i), inverseTicks,
                                    &c->launchedKernels));
    }
    return PTSS_OK;
}

int ptss_denoise(ptss_context* c, const ptss_pixel_feature* dev_features, const ptss_denoise_params* params, ptss_uchar4* dev_out,
                 void* hipStream) {
    return denoisePasses(c, "ptss_denoise", nullptr, true, dev_features, params, dev_out, hipStream);
}

// the same passes over the colours of a history: an entry is laid out as a colour-plane entry, so every pass is a denoiseKernel<false, *>
int ptss_denoise_history(ptss_context* c, const ptss_history_entry* dev_history, const ptss_pixel_feature* dev_features,
                         const ptss_denoise_params* params, ptss_uchar4* dev_out, void* hipStream) {
    return denoisePasses(c, "ptss_denoise_history", dev_history, false, dev_features, params, dev_out, hipStream);
}

int ptss_default_reproject_params(ptss_reproject_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(*p);
    p->cosNormal = 0.9f;
    p->depthTolerance = 0.02f;
    p->maxHistory = 64.0f;
    p->minCoverage = 0.25f;
    return PTSS_OK;
}

int ptss_reproject(ptss_context* c, const ptss_pixel_feature* dev_features_now, const ptss_camera* prev_camera,
                   const ptss_pixel_feature* dev_features_prev, const ptss_history_entry* dev_history_prev,
                   const ptss_reproject_params* params, ptss_history_entry* dev_history_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_features_now || !dev_history_out) return fail(PTSS_EINVAL, "null argument");
    if (dev_history_prev && (!prev_camera || !dev_features_prev)) return fail(PTSS_EINVAL, "a history needs its camera and its features");
    if (const char* why = ptrp::paramsError(params)) return fail(PTSS_EINVAL, why);
    if (static_cast<const void*>(dev_history_out) == static_cast<const void*>(dev_history_prev))
        return fail(PTSS_EINVAL, "dev_history_out must not be dev_history_prev: a pixel's taps are other pixels' entries");
    if (((uintptr_t)dev_features_now | (uintptr_t)dev_features_prev | (uintptr_t)dev_history_prev | (uintptr_t)dev_history_out) & 15u)
        return fail(PTSS_EINVAL, "features and histories must be 16-byte aligned");
    if (c->tile.world > 1)
        return fail(PTSS_EINVAL, "ptss_reproject needs the whole frame: this context is a pixel-band shard (tileWorld > 1)");
    if (c->numPixels == 0) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = hipStream ? static_cast<hipStream_t>(hipStream) : c->stream;
    // c and n of the accumulator as it stands: the last frame's display scale (ptss_denoise's input), nothing before the first frame
    const int perPixel = (int)c->samples * (c->lastTicks - c->lastResetTick + 1);
    const float inverseTicks = 1.f / (float)perPixel;
    const float n = c->frameIndex == 0 ? 0.0f : (float)perPixel;
    const int width = c->tile.width, height = c->tile.height;
    const ptrp::View now = ptrp::viewOf(c->camera, width, height);
    const ptrp::View prev = dev_history_prev ? ptrp::viewOf(*prev_camera, width, height) : now;
    HIP_TRY(ptss::launchReproject(st, c->dAccum, dev_features_now, dev_features_prev, dev_history_prev, dev_history_out, width, height, now, prev,
                                  ptrp::paramsOf(*params), inverseTicks, n, &c->launchedKernels));
    return PTSS_OK;
}

int ptss_read_denoise_plane(ptss_context* c, float* host_float3, size_t count, int* level) {
    if (!c || !host_float3) return fail(PTSS_EINVAL, "null argument");
    if (c->denoiseLastPlane < 0) return fail(PTSS_EINVAL, "no colour plane: the latest ptss_denoise of this context ran fewer than two levels");
    if (count != (size_t)3 * c->numPixels) return fail(PTSS_ERANGE, "count must be 3 * local pixels");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->denoiseStream));
    std::vector<float4> plane(c->numPixels);
    HIP_TRY(hipMemcpy(plane.data(), c->dDenoise[c->denoiseLastPlane], plane.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t p = 0; p < plane.size(); ++p) {
        host_float3[3 * p] = plane[p].x;
        host_float3[3 * p + 1] = plane[p].y;
        host_float3[3 * p + 2] = plane[p].z;
    }
    if (level) *level = c->denoiseLastLevel;
    return PTSS_OK;
}

// ---- scene updates on a live context -----------------------------------------------------------------------------
int ptss_set_scene(ptss_context* c, const ptss_scene_desc* scene) {
    if (!c || !scene) return fail(PTSS_EINVAL, "null argument");
    RC_TRY(validateScene(*scene));
    HIP_TRY(hipSetDevice(c->cfg.device));
    SceneState st;   // the new blobs exist before the old ones go: on any error the context keeps its scene
    RC_TRY(buildSceneState(*scene, c->cfg, (int)c->lanes.size(), c->lanes[0].maxBlocks, c->numCUs, st));
    if (int rc = quiesce(c)) {
        releaseSceneState(st);
        return rc;
    }
    if (c->updated) (void)hipStreamSynchronize(c->updateStream);
    harvestHints(c);   // (every read-back has landed) ... and the old scene's live counts say nothing about the new one's
    for (Lane& ln : c->lanes) ln.haveHint = false;
    for (SceneImage& im : c->images) (void)hipFree(im.dBlob);
    adoptSceneState(c, st);
    c->cameraDirty = true;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_update_triangles(ptss_context* c, const ptss_triangle* dev_triangles, size_t first, size_t count, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (count == 0) return PTSS_OK;
    if (!dev_triangles) return fail(PTSS_EINVAL, "dev_triangles is null with count > 0");
    if ((uintptr_t)dev_triangles & 3u) return fail(PTSS_EINVAL, "dev_triangles must be 4-byte aligned");
    const size_t T = (size_t)c->images[0].layout.numTriangles;
    if (first >= T || count > T - first) return fail(PTSS_ERANGE, "first .. first + count - 1 leaves the scene's triangles");
    for (const SceneImage& im : c->images)
        if (im.dBlob && im.layout.triClassed)
            return fail(PTSS_EINVAL, "the scene image stores its triangles grouped by edge class (T <= 255), an order that depends on the "
                                     "vertices: replace the scene with ptss_set_scene (repacking so small a scene costs microseconds)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = hipStream ? static_cast<hipStream_t>(hipStream) : c->stream;
    unsigned long long* rejected = c->dTotal + kRejectedWord;
    for (SceneImage& im : c->images) {
        if (!im.dBlob) continue;
        HIP_TRY(ptss::launchSceneUpdate(st, im.dBlob, im.layout, dev_triangles, (uint32_t)first, (uint32_t)count, rejected, &c->launchedKernels));
        rejected = nullptr;   // the second image drops the same records: counted once
        if (ptss::meshImage(im.layout)) HIP_TRY(ptss::launchMeshRefit(st, im.dBlob, im.layout, &c->launchedKernels));
    }
    c->updateStream = st;
    c->updated = true;
    c->cameraDirty = true;   // the camera-origin rows (offPrimTri) belong to the old vertices
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_update_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (c->updated) HIP_TRY(hipStreamSynchronize(c->updateStream));
    HIP_TRY(hipMemcpy(out, c->dTotal + kRejectedWord, sizeof(*out), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_reseed(ptss_context* c, unsigned long long seed) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    HIP_TRY(hipSetDevice(c->cfg.device));
    RC_TRY(quiesce(c));   // no lane is still drawing from the streams
    if (int rc = createCheck(seedStreams(c, seed, c->stream), "ptss_reseed: rngInitKernel")) return rc;
    c->cfg.seed = seed;
    c->resetTicksThisFrame = true;
    return PTSS_OK;
}

int ptss_read_triangle_bounds(ptss_context* c, float* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    const SceneImage& im = c->image();
    if (!ptss::meshImage(im.layout)) return fail(PTSS_EINVAL, "the scene image in use is not a mesh image");
    const size_t leaves = (size_t)im.layout.mesh.numLeaves, groups = (size_t)im.layout.mesh.numGroups;
    if (count != 12 * (leaves + groups)) return fail(PTSS_ERANGE, "count must be 12 * (leaves + groups)");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->updated) HIP_TRY(hipStreamSynchronize(c->updateStream));
    HIP_TRY(hipMemcpy(host, im.dBlob + im.layout.mesh.offLeaf, 12 * leaves * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(host + 12 * leaves, im.dBlob + im.layout.mesh.offGroup, 12 * groups * sizeof(float), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_read_triangle_positions(ptss_context* c, int* host, size_t count) {
    if (!c || !host) return fail(PTSS_EINVAL, "null argument");
    const SceneImage& im = c->image();
    if (!ptss::meshImage(im.layout)) return fail(PTSS_EINVAL, "the scene image in use is not a mesh image");
    if (count != (size_t)im.layout.numTriangles) return fail(PTSS_ERANGE, "count must be the scene's triangle count");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host, im.dBlob + im.layout.offTriPos, count * sizeof(int), hipMemcpyDeviceToHost));
    return PTSS_OK;
}

int ptss_triangle_leaves(const ptss_context* c, int* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    const ptss::SceneLayout& L = c->image().layout;
    *out = ptss::meshImage(L) ? L.mesh.numLeaves : 0;
    return PTSS_OK;
}

int ptss_debug_counters(ptss_context* c, unsigned long long* out8) {
    if (!c || !out8) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
#if PTSS_DIAG
    HIP_TRY(ptss::readDiagCounters(out8));
#else
    for (int k = 0; k < 8; ++k) out8[k] = 0ull;   // the shipped library carries no counter (ptss_diag.h)
#endif
    return PTSS_OK;
}

int ptss_bounce_kernel_time(ptss_context* c, double* total_ms, unsigned long long* launches) {
    if (!c || !total_ms || !launches) return fail(PTSS_EINVAL, "null argument");
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Lane& ln : c->lanes)
        if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
    drainKernelEvents(c, true);
    // union of the launch intervals (one lane: they do not overlap, and this is the sum of the durations)
    std::sort(c->kernelSpans.begin(), c->kernelSpans.end());
    double busy = 0.0, curA = 0.0, curB = -1.0;
    for (const auto& sp : c->kernelSpans) {
        if (curB < curA || sp.first > curB) {
            if (curB >= curA) busy += curB - curA;
            curA = sp.first;
            curB = sp.second;
        } else if (sp.second > curB) {
            curB = sp.second;
        }
    }
    if (curB >= curA) busy += curB - curA;
    *total_ms = busy;
    *launches = c->kernelSpans.size();
    c->kernelSpans.clear();
    HIP_TRY(hipEventRecord(c->evEpoch, c->stream));   // a fresh epoch for the next window: float32 ms stay fine-grained
    HIP_TRY(hipEventSynchronize(c->evEpoch));
    return checkLaneTimeouts(c);
}

}  // extern "C"
