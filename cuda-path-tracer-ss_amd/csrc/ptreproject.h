// ptreproject.h — the arithmetic of ptss_reproject, written once for the gfx950 kernel (ptss_reproject.hip) and
// for the host probe (host_capi.cpp ptss_probe_reproject; tests/test_reproject_cpu.py). Everything is float32 built from ptmath.h
// operations in the order written here, compiled without contraction on both sides, so the two builds agree bit for bit.
//
// A static scene and a moved camera. For pixel p = (x, y) of the current frame, with colour c_p (the accumulator's display value,
// ptdn::displayValue), n samples behind it and first-hit feature f_p:
//   d_p    the pixel-centre eye ray of the current camera, bounce 0's operations with a jitter of 0.5
//   hit:   P = fma(d_p, depth_p, o_now);  v = P - o_prev;  r = |v|          (the distance the previous camera saw P at)
//   miss:  v = d_p                                                          (direction only: the translation is ignored)
//   l = rotate(conj(q_prev), v); rejected unless l.z * zNear_prev > 0       (in front of the previous camera, whatever zNear's sign)
//   fx = (l.x / (l.z s) + 0.5) W - 0.5,  fy = (l.y / ((l.z s) aspect) + 0.5) H - 0.5      s = -2 tan(fov / 2) of the previous camera
//   rejected unless -1 <= fx < W and -1 <= fy < H; x0 = floor(fx), tx = fx - x0 (y alike); taps q = (x0 + i, y0 + j), i, j in 0..1,
//   in the order (0,0) (1,0) (0,1) (1,1), with b_q = (i ? tx : 1 - tx) (j ? ty : 1 - ty).
// A tap counts (v_q = 1) iff it lies inside the frame, b_q > 0, materialIdx_q == materialIdx_p (the hard stop), for hits
// n_p . n_q >= cosNormal and |depth_q - r| <= depthTolerance r (otherwise the previous camera saw something else there: P was
// hidden), and its history entry is finite with weight > 0. Then, over the counting taps,
//   B = sum b_q;  w = min((sum b_q weight_q) / B, maxHistory), 0 if B < minCoverage;  t = w / (n + w)
//   out = c_p + ((sum b_q (c_q - c_p)) / B) t,  clamped per channel to [min, max] of c_p and the counting c_q;  weight = n + w
// Moving triangles (ptss_reproject_motion): for a hit, P is replaced by prevPoint_p of a ptss_pixel_motion row
// (ptmotion.h) — where the surface point was in the previous pose — and nothing else changes.
// — the normalised mean h = sum b c / sum b written around c_p, as the filter's is (ptdenoise.h): a constant image stays constant
// exactly. A rejected pixel, B = 0 or w = 0 give (c_p, n) exactly.
#pragma once
#include "ptdenoise.h"

namespace ptrp {
using namespace ptv;

struct View {   // the constants of one camera, evaluated on the host (viewOf) and handed to the kernel as they are
    quat rotation;   // the camera's
    quat inverse;    // its conjugate
    vec3 position;
    float zNear;
    float s;         // -2 * tan(fov / 2)  (EyeParams, cameraRay)
    float aspect;    // H / W
    float invW, invH;
    float width, height;
};

inline View viewOf(const ptss_camera& cam, int width, int height) {
    View v;
    v.rotation = cam.rotation;
    v.inverse = q4(cam.rotation.w, -cam.rotation.x, -cam.rotation.y, -cam.rotation.z);
    v.position = cam.position;
    v.zNear = cam.zNear;
    v.s = -2 * ptm::tan(cam.fieldOfView * 0.5f);
    v.aspect = (float)height / (float)width;
    v.invW = 1.0f / width;
    v.invH = 1.0f / height;
    v.width = (float)width;
    v.height = (float)height;
    return v;
}

struct Params {   // what the kernel reads of a ptss_reproject_params
    float cosNormal, depthTolerance, maxHistory, minCoverage;
};

// the argument check ptss_reproject and ptss_probe_reproject share; nullptr when the parameters are acceptable
inline const char* paramsError(const ptss_reproject_params* p) {
    if (!p) return "params is null";
    if (p->structSize != (unsigned int)sizeof(ptss_reproject_params))
        return "params->structSize is not this library's sizeof(ptss_reproject_params): start from ptss_default_reproject_params";
    if (!(p->cosNormal >= -1.0f && p->cosNormal <= 1.0f)) return "cosNormal must be in [-1, 1]";
    if (!(p->depthTolerance >= 0.0f && p->depthTolerance < ptm::inf())) return "depthTolerance must be finite and not negative";
    if (!(p->maxHistory >= 0.0f && p->maxHistory < ptm::inf())) return "maxHistory must be finite and not negative";
    if (!(p->minCoverage >= 0.0f && p->minCoverage <= 1.0f)) return "minCoverage must be in [0, 1]";
    return nullptr;
}
inline Params paramsOf(const ptss_reproject_params& p) { return Params{p.cosNormal, p.depthTolerance, p.maxHistory, p.minCoverage}; }

struct Entry {   // a ptss_history_entry
    vec3 colour;
    float weight;
};
struct Geometry {   // the first row of a ptss_pixel_feature
    vec3 normal;
    float depth;
};

PTM_HD bool finite(float v) { return ptm::abs(v) < ptm::inf(); }

// the pixel-centre eye ray of (x, y): bounce 0's operations (ptss_kernels.hip bounceTile / featureKernel, HostOps.cpp cameraRay)
PTM_HD vec3 eyeDirection(const View& c, int x, int y) {
    const float jitteredX = x + 0.5f;
    const float jitteredY = y + 0.5f;
    const vec3 start = v3(((jitteredX * c.invW) - 0.5f) * c.s, 1 * ((jitteredY * c.invH) - 0.5f) * c.s * c.aspect, 1.0f) * c.zNear;
    return normalize(rotate(c.rotation, start));
}

// Pixel (x, y). pointOf(d) -> vec3, the world point a HIT pixel's surface point is looked up at in the previous frame, d being the
// pixel's eye direction (called for hits only): where that point is now (a static scene, the overload below) or where it was in the
// previous pose (ptss_reproject_motion). materialAt(q) -> int, geometryAt(q) -> Geometry (both of the PREVIOUS
// features), historyAt(q) -> Entry, q = y * width + x; each is called only for a tap inside the frame, the material first.
template <class PointOf, class MaterialAt, class GeometryAt, class HistoryAt>
PTM_HD Entry reprojectPixel(int x, int y, int width, int height, vec3 cp, float n, const ptdn::Feature& fp, const View& now, const View& prev,
                            const Params& prm, PointOf pointOf, MaterialAt materialAt, GeometryAt geometryAt, HistoryAt historyAt) {
    const Entry keep{cp, n};
    const bool hit = fp.materialIdx >= 0;
    vec3 v = eyeDirection(now, x, y);
    float range = 0.0f;
    if (hit) {
        v = pointOf(v) - prev.position;
        range = length(v);
    }
    const vec3 l = rotate(prev.inverse, v);
    if (!(l.z * prev.zNear > 0.0f)) return keep;
    const float zs = l.z * prev.s;
    const float fx = (ptm::div(l.x, zs) + 0.5f) * prev.width - 0.5f;
    const float fy = (ptm::div(l.y, zs * prev.aspect) + 0.5f) * prev.height - 0.5f;
    if (!(fx >= -1.0f && fx < prev.width && fy >= -1.0f && fy < prev.height)) return keep;   // (also what keeps NaN and inf from the conversions)
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float tx = fx - flx, ty = fy - fly;
    const float tolerance = prm.depthTolerance * range;
    vec3 dsum = v3(0, 0, 0), lo = cp, hi = cp;
    float bsum = 0.0f, wsum = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int i = k & 1, j = k >> 1;
        const int qx = x0 + i, qy = y0 + j;
        if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
        const float b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
        if (!(b > 0.0f)) continue;
        const int q = qy * width + qx;
        if (materialAt(q) != fp.materialIdx) continue;
        if (hit) {
            const Geometry g = geometryAt(q);
            if (!(dot(fp.normal, g.normal) >= prm.cosNormal)) continue;
            if (!(ptm::abs(g.depth - range) <= tolerance)) continue;
        }
        const Entry e = historyAt(q);
        if (!(finite(e.colour.x) && finite(e.colour.y) && finite(e.colour.z) && finite(e.weight) && e.weight > 0.0f)) continue;
        dsum = madd(e.colour - cp, b, dsum);
        wsum = ptm::fma(e.weight, b, wsum);
        bsum = bsum + b;
        lo = v3(ptm::min(lo.x, e.colour.x), ptm::min(lo.y, e.colour.y), ptm::min(lo.z, e.colour.z));
        hi = v3(ptm::max(hi.x, e.colour.x), ptm::max(hi.y, e.colour.y), ptm::max(hi.z, e.colour.z));
    }
    if (!(bsum > 0.0f)) return keep;
    float w = ptm::min(ptm::div(wsum, bsum), prm.maxHistory);
    if (bsum < prm.minCoverage) w = 0.0f;
    if (!(w > 0.0f)) return keep;
    const float total = n + w;
    const vec3 out = madd(dsum / bsum, ptm::div(w, total), cp);
    return Entry{v3(ptm::clamp(out.x, lo.x, hi.x), ptm::clamp(out.y, lo.y, hi.y), ptm::clamp(out.z, lo.z, hi.z)), total};
}

// A static scene (ptss_reproject): the point is where the eye ray hits, P = fma(d_p, depth_p, o_now).
template <class MaterialAt, class GeometryAt, class HistoryAt>
PTM_HD Entry reprojectPixel(int x, int y, int width, int height, vec3 cp, float n, const ptdn::Feature& fp, const View& now, const View& prev,
                            const Params& prm, MaterialAt materialAt, GeometryAt geometryAt, HistoryAt historyAt) {
    auto pointOf = [&](vec3 d) -> vec3 { return madd(d, fp.depth, now.position); };
    return reprojectPixel(x, y, width, height, cp, n, fp, now, prev, prm, pointOf, materialAt, geometryAt, historyAt);
}

}  // namespace ptrp
