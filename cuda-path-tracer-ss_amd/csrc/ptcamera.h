// ptcamera.h — the camera models of a film (ptss_generate_rays), written once for the gfx950 kernel (ptss_film.hip)
// and for the host probe (host_capi.cpp ptss_probe_film_rays; tests/test_film_cpu.py). Everything is float32 built from ptmath.h
// operations in the order written here, compiled without contraction on both sides, so the two builds agree bit for bit: the host
// build of this header is the specification of the device's rays.
//
// A film is width x height pixels, pixel p = (x, y) = (p % width, p / width), row 0 at the bottom (the frame's convention). The eye ray
// of a pixel takes up to four uniforms of (0, 1] from the ray's own stream, in this order: jx, jy (where in the pixel), u1, u2 (where on
// the lens). draws(kind, jitter) says how many a model takes; with jitter = 0 it takes none and jx = jy = 0.5, lens point = lens centre.
// The constants s = -2 tan(fov / 2), aspect = H / W, invW = 1 / W, invH = 1 / H are evaluated once on the host (filmOf), with the
// expressions of ptss_context.h eyeParams and HostOps.cpp cameraRay, and travel by value.
//
//   PINHOLE     computeEyeRay (CudaTracer.cu:321-343) with bounce 0's operations, i.e. HostOps.cpp cameraRay:
//                 X = x + jx;  Y = y + jy
//                 start = (((X invW) - 0.5) s,  1 ((Y invH) - 0.5) s aspect,  1) * zNear
//                 origin = position;  direction = normalize(rotate(rotation, start))
//   THIN_LENS   the same X, Y and `start`; then, in camera space (a camera looks along sign(zNear) z):
//                 t = div(focusDistance, |start.z|);  f = start * t                      the focus point: on the plane |z| = focusDistance
//                 r = lensRadius sqrt(u1);  sincos(2 pi u2) -> (sn, cs);  l = (r cs, r sn, 0)        the lens point (jitter = 0: l = 0)
//                 origin = position + rotate(rotation, l);  direction = normalize(rotate(rotation, f - l))
//               2 pi is the float 2 * ptm::kPi; 2 pi u2 is one product. Every ray of a pixel sample passes through position + R f.
//   EQUIRECT    lon = ((X invW) - 0.5) (2 pi);  lat = ((Y invH) - 0.5) pi;  sincos(lon) -> (sl, cl);  sincos(lat) -> (se, ce)
//                 c = (sl ce, se, -(cl ce));  origin = position;  direction = normalize(rotate(rotation, c))
//               The film's centre looks along R (0, 0, -1), as the centre ray of a pinhole of the reference's cameras does (zNear < 0,
//               0 < fov < pi); +x on the film turns towards R (+1, 0, 0) and +y towards R (0, +1, 0), the pinhole's senses.
//               fieldOfView and zNear are not read.
// Every ray: tmax = +inf, pad = 0.
#pragma once
#include "ptmath.h"

namespace ptcam {
using namespace ptv;

constexpr float kTwoPi = 2 * ptm::kPi;

struct Film {   // a ptss_film_camera with its host-evaluated constants
    ptss_camera camera;
    float s, aspect, invW, invH;
    int kind, width, height, jitter;
    float lensRadius, focusDistance;
};

// the argument check ptss_generate_rays and ptss_probe_film_rays share; nullptr when the camera is acceptable
inline const char* cameraError(const ptss_film_camera* f) {
    if (!f) return "film camera is null";
    if (f->structSize != (unsigned int)sizeof(ptss_film_camera)) return "structSize is not this library's sizeof(ptss_film_camera)";
    if (f->kind != PTSS_FILM_PINHOLE && f->kind != PTSS_FILM_THIN_LENS && f->kind != PTSS_FILM_EQUIRECT) return "unknown film camera kind";
    if (f->jitter != 0 && f->jitter != 1) return "jitter must be 0 or 1";
    if (f->width <= 0 || f->height <= 0) return "the film's width and height must be positive";
    if (f->kind == PTSS_FILM_THIN_LENS) {
        if (!(f->lensRadius >= 0.0f && f->lensRadius < ptm::inf())) return "lensRadius must be finite and not negative";
        if (!(f->focusDistance > 0.0f && f->focusDistance < ptm::inf())) return "focusDistance must be finite and positive";
    }
    return nullptr;
}

inline Film filmOf(const ptss_film_camera& f) {
    Film o;
    o.camera = f.camera;
    o.s = -2 * ptm::tan(f.camera.fieldOfView * 0.5f);
    o.aspect = (float)f.height / (float)f.width;
    o.invW = 1.0f / f.width;
    o.invH = 1.0f / f.height;
    o.kind = f.kind;
    o.width = f.width;
    o.height = f.height;
    o.jitter = f.jitter;
    o.lensRadius = f.lensRadius;
    o.focusDistance = f.focusDistance;
    return o;
}

PTM_HD int draws(int kind, int jitter) { return jitter ? (kind == PTSS_FILM_THIN_LENS ? 4 : 2) : 0; }

// where on the film the sample of pixel (x, y) lies, in pixels: the X, Y every model starts from (ptss_generate_rays_positions hands them out)
PTM_HD void samplePosition(int x, int y, float jx, float jy, float& X, float& Y) {
    X = x + jx;
    Y = y + jy;
}

// the eye ray of pixel (x, y); jx, jy, u1, u2: the stream's draws in that order (0.5, 0.5 and anything with jitter = 0: u1, u2 are
// then not read)
PTM_HD ptss_ray_query filmRay(const Film& F, int x, int y, float jx, float jy, float u1, float u2) {
    float jitteredX, jitteredY;
    samplePosition(x, y, jx, jy, jitteredX, jitteredY);
    vec3 o = F.camera.position;
    vec3 v;
    if (F.kind == PTSS_FILM_EQUIRECT) {
        const float lon = ((jitteredX * F.invW) - 0.5f) * kTwoPi;
        const float lat = ((jitteredY * F.invH) - 0.5f) * ptm::kPi;
        float sl, cl, se, ce;
        ptm::sincos(lon, sl, cl);
        ptm::sincos(lat, se, ce);
        v = rotate(F.camera.rotation, v3(sl * ce, se, -(cl * ce)));
    } else {
        const vec3 start = v3(((jitteredX * F.invW) - 0.5f) * F.s, 1 * ((jitteredY * F.invH) - 0.5f) * F.s * F.aspect, 1.0f) * F.camera.zNear;
        if (F.kind == PTSS_FILM_THIN_LENS) {
            const float t = ptm::div(F.focusDistance, ptm::abs(start.z));
            const vec3 f = start * t;
            vec3 l = v3(0, 0, 0);
            if (F.jitter) {
                const float r = F.lensRadius * ptm::sqrt(u1);
                float sn, cs;
                ptm::sincos(kTwoPi * u2, sn, cs);
                l = v3(r * cs, r * sn, 0.0f);
            }
            o = F.camera.position + rotate(F.camera.rotation, l);
            v = rotate(F.camera.rotation, f - l);
        } else {
            v = rotate(F.camera.rotation, start);
        }
    }
    ptss_ray_query q;
    q.origin = o;
    q.tmax = ptm::inf();
    q.direction = normalize(v);
    q.pad = 0.0f;
    return q;
}

}  // namespace ptcam
