// host_capi.cpp — extern "C" face of the host mirror (include/ptss_host.h). Host only; no HIP.
#include "ptss_host.h"

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "HostOps.h"
#include "Scene.h"
#include "ptdenoise.h"
#include "ptreproject.h"
#include "ptupsample.h"
#include "ptcamera.h"
#include "ptadaptive.h"
#include "ptlinear.h"
#include "ptlinstats.h"
#include "ptsplat.h"
#include "ptmeter.h"
#include "ptglare.h"
#include "pttone.h"
#include "ptlindn.h"
#include "ptlinrp.h"
#include "ptlinup.h"
#include "ptmotion.h"
#include "ptspecular.h"
#include "ptsurface.h"
#include "ptlightmap.h"
#include "ptquant.h"
#include "ptlocate.h"
#include "ptmesh.h"
#include "ptorder.h"
#include "ptpack.h"
#include "ptstrip.h"
#include "pttri.h"
#include "ptvecops.h"
#include "xorwow.h"

struct ptss_scene {
    Scene scene;
};

// Triangle::intersectRay (Primitives.h:25-83) for n (triangle, ray) pairs in the general form and in the edge-class form
// the kernels pick for that triangle (csrc/pttri.h — the very functions the kernels call, compiled for the host).
namespace {
using namespace ptv;
template <int kC1, int kC2>
void triangleForm(const float* t, const float* o3, const float* d3, float limit, bool primary, float* out) {
    const vec3 v0 = v3(t[0], t[1], t[2]), e1 = v3(t[3], t[4], t[5]), e2 = v3(t[6], t[7], t[8]);
    const vec3 o = v3(o3[0], o3[1], o3[2]), d = v3(d3[0], d3[1], d3[2]);
    pttri::Head h;
    if (primary) {   // what primaryPrepKernel stores, with the general form
        const vec3 s = o - v0, r = cross(s, e1);
        h = pttri::head<kC1, kC2, true>(v0, e1, e2, s, r, dot(e2, r), o, d);
    } else {
        h = pttri::head<kC1, kC2, false>(v0, e1, e2, v3(0, 0, 0), v3(0, 0, 0), 0.0f, o, d);
    }
    float b0 = 0, b1 = 0, b2 = 0;
    const bool pass = pttri::passesHead(h, limit);
    if (pass) pttri::weights<kC1, kC2>(h, d, b0, b1, b2);
    out[0] = (pass && pttri::passesWeights(b0, b1, b2)) ? 1.0f : 0.0f;
    out[1] = h.dist;
    out[2] = b0;
    out[3] = b1;
    out[4] = b2;
    out[5] = h.det;
}

// The plan of ptss_plan_samples and ptss_plan_samples_linear behind their argument checks (csrc/ptadaptive.h): the running sums of
// weight(p, &kind) over the film, the counts of the kinds, and the index under n evenly spaced targets
template <class Weight>
void planSamples(size_t filmPixels, size_t n, unsigned long long* cdf, uint32_t* index, ptss_plan_info* info, Weight weight) {
    ptss_plan_info found{};
    unsigned long long sum = 0;
    for (size_t p = 0; p < filmPixels; ++p) {
        uint32_t kind;
        sum += weight(p, &kind);
        cdf[p] = sum;
        found.activePixels += (kind & ptad::kActive) ? 1u : 0u;
        found.unsampledPixels += (kind & ptad::kUnsampled) ? 1u : 0u;
        found.cappedPixels += (kind & ptad::kCapped) ? 1u : 0u;
    }
    found.totalWeight = sum;
    found.uniform = sum == 0ull ? 1u : 0u;
    for (size_t i = 0; i < n; ++i)
        index[i] = sum == 0ull ? ptad::uniformPixel(i, n, filmPixels) : ptad::pixelOf(cdf, (uint32_t)filmPixels, ptad::target(i, n, sum));
    if (info) *info = found;
}
}  // namespace

extern "C" {

int ptss_scene_create(const char* preset, ptss_scene** out) {
    if (!preset || !out) return PTSS_HOST_EINVAL;
    ptss_scene* s = new (std::nothrow) ptss_scene();
    if (!s) return PTSS_HOST_EINVAL;
    if (!s->scene.buildPreset(preset)) {
        delete s;
        return PTSS_HOST_EINVAL;
    }
    *out = s;
    return PTSS_HOST_OK;
}

void ptss_scene_destroy(ptss_scene* s) { delete s; }

int ptss_scene_describe(const ptss_scene* s, ptss_scene_desc* out) {
    if (!s || !out) return PTSS_HOST_EINVAL;
    *out = s->scene.desc();
    return PTSS_HOST_OK;
}

int ptss_scene_add_obj(ptss_scene* s, const char* path, const float* m, int materialIdx, size_t* added) {
    if (!s || !path || materialIdx < 0 || (size_t)materialIdx >= s->scene.materialsVec.size()) return PTSS_HOST_EINVAL;
    mat4 t = mat4::identity();
    if (m)
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) t.c[c][r] = m[4 * r + c];   // mat4 is column-major
    const long n = s->scene.addObjModel(path, t, materialIdx);
    if (n < 0) return n == -2 ? PTSS_HOST_EIO : PTSS_HOST_EINVAL;
    if (added) *added = (size_t)n;
    return PTSS_HOST_OK;
}

int ptss_camera_default(ptss_camera* out) {
    if (!out) return PTSS_HOST_EINVAL;
    *out = Camera();
    return PTSS_HOST_OK;
}

int ptss_camera_ray(const ptss_camera* cam, int width, int height, int x, int y, float jx, float jy, ptss_ray_query* out) {
    if (!cam || !out || width <= 0 || height <= 0) return PTSS_HOST_EINVAL;
    *out = cameraRay(*cam, width, height, x, y, jx, jy);
    return PTSS_HOST_OK;
}

int ptss_camera_move(ptss_camera* cam, unsigned char key, int* moved) {
    if (!cam) return PTSS_HOST_EINVAL;
    Camera c;
    static_cast<ptss_camera&>(c) = *cam;
    const bool m = moveCamera(c, key);
    *cam = c;
    if (moved) *moved = m ? 1 : 0;
    return PTSS_HOST_OK;
}

int ptss_write_tga(const char* filename, const ptss_uchar4* rgba, int width, int height) {
    if (!filename || !rgba || width <= 0 || height <= 0) return PTSS_HOST_EINVAL;
    return writeTga(filename, rgba, width, height) ? PTSS_HOST_OK : PTSS_HOST_EIO;
}

int ptss_tile_rows(int height, int band_rows, int rank, int world, int* rows, int cap) {
    if (height < 0 || band_rows <= 0 || world <= 0 || rank < 0 || rank >= world) return PTSS_HOST_EINVAL;
    int n = 0;
    for (int y = 0; y < height; ++y) {
        if ((y / band_rows) % world != rank) continue;
        if (rows && n < cap) rows[n] = y;
        ++n;
    }
    return n;
}

int ptss_probe_guard(int op, const float* x, unsigned int* out, size_t n) {
    if (!x || !out || op < 0 || op > 3) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        switch (op) {
            case 0: out[i] = ptm::fast_numerator(x[i]) ? 1u : 0u; break;
            case 1: out[i] = ptm::fast_divisor(x[i]) ? 1u : 0u; break;
            case 2: out[i] = ptm::fast_rcp_operand(x[i]) ? 1u : 0u; break;
            default: out[i] = ptm::in_light_window(x[i]) ? 1u : 0u; break;
        }
    }
    return PTSS_HOST_OK;
}

int ptss_probe_guard_constants(float* out9) {
    if (!out9) return PTSS_HOST_EINVAL;
    const float k[9] = {ptm::kSqrtLo, ptm::kSqrtHi, ptm::kRcpLo, ptm::kRcpHi, ptm::kDivLo, ptm::kDivHi, ptm::kLightD2Lo, ptm::kLightD2Hi,
                        ptm::kFourPi};
    for (int i = 0; i < 9; ++i) out9[i] = k[i];
    return PTSS_HOST_OK;
}

int ptss_probe_scene_guard_flags(const ptss_scene_desc* scene, unsigned int* out) {
    if (!scene || !out) return PTSS_HOST_EINVAL;
    *out = ptpack::sceneGuardFlags(*scene);
    return PTSS_HOST_OK;
}

int ptss_probe_math(int op, const float* x, const float* y, float* out, size_t n) {
    if (!x || !out) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        float s, c;
        switch (op) {
            case 0: ptm::sincos(x[i], s, c); out[i] = s; break;
            case 1: ptm::sincos(x[i], s, c); out[i] = c; break;
            case 2: out[i] = ptm::tan(x[i]); break;
            case 3: out[i] = ptm::atan(x[i]); break;
            case 4: out[i] = ptm::log(x[i]); break;
            case 5: out[i] = ptm::exp(x[i]); break;
            case 6: if (!y) return PTSS_HOST_EINVAL; out[i] = ptm::pow(x[i], y[i]); break;
            case 7: out[i] = ptm::sqrt(x[i]); break;
            default: return PTSS_HOST_EINVAL;
        }
    }
    return PTSS_HOST_OK;
}

int ptss_probe_vector(int op, const float* in, float* out, size_t n) {
    if (!in || !out || op < 0 || op >= ptvecops::kOps) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) ptvecops::apply(op, in + ptvecops::kIn * i, out + ptvecops::kOut * i);
    return PTSS_HOST_OK;
}

int ptss_probe_triangle_forms(const float* tri9, const float* o3, const float* d3, const float* limit, int primary, size_t n, int* cls,
                              float* general6, float* classed6) {
    if (!tri9 || !o3 || !d3 || !limit || !cls || !general6 || !classed6) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        const float* t = tri9 + 9 * i;
        const int c = pttri::triangleClass(v3(t[3], t[4], t[5]), v3(t[6], t[7], t[8]));
        cls[i] = c;
        triangleForm<0, 0>(t, o3 + 3 * i, d3 + 3 * i, limit[i], primary != 0, general6 + 6 * i);
        float* out = classed6 + 6 * i;
        switch (c) {
#define PTSS_TRI_CASE(c1, c2) \
    case (c1) * 4 + (c2): triangleForm<c1, c2>(t, o3 + 3 * i, d3 + 3 * i, limit[i], primary != 0, out); break;
            PTSS_TRI_CASE(0, 1) PTSS_TRI_CASE(0, 2) PTSS_TRI_CASE(0, 3)
            PTSS_TRI_CASE(1, 0) PTSS_TRI_CASE(1, 2) PTSS_TRI_CASE(1, 3)
            PTSS_TRI_CASE(2, 0) PTSS_TRI_CASE(2, 1) PTSS_TRI_CASE(2, 3)
            PTSS_TRI_CASE(3, 0) PTSS_TRI_CASE(3, 1) PTSS_TRI_CASE(3, 2)
#undef PTSS_TRI_CASE
            default: triangleForm<0, 0>(t, o3 + 3 * i, d3 + 3 * i, limit[i], primary != 0, out); break;
        }
    }
    return PTSS_HOST_OK;
}

int ptss_probe_wave_locate(int width, int rank, int world, int bandRows, unsigned int firstBegin, size_t n, int* wave3, int* lane3, int* fast) {
    if (!wave3 || !lane3 || !fast || width <= 0 || bandRows <= 0 || world <= 0 || rank < 0 || rank >= world) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t first = firstBegin + (uint32_t)i;
        const ptloc::WaveOrigin w = ptloc::waveOrigin(width, rank, world, bandRows, first);
        fast[i] = w.oneWrap ? 1 : 0;
        for (uint32_t k = 0; k < ptloc::kStrip; ++k) {
            const ptloc::Coord ref = ptloc::locate(width, rank, world, bandRows, first + k);
            const ptloc::Coord got = w.oneWrap ? ptloc::laneCoord(w, width, k) : ref;   // (the kernel's fallback: locate per lane)
            int* a = wave3 + 3 * (i * ptloc::kStrip + k);
            int* b = lane3 + 3 * (i * ptloc::kStrip + k);
            a[0] = got.x; a[1] = got.gy; a[2] = (int)got.globalIndex;
            b[0] = ref.x; b[1] = ref.gy; b[2] = (int)ref.globalIndex;
        }
    }
    return PTSS_HOST_OK;
}

int ptss_probe_strip_masks(const ptss_scene_desc* scene, const ptss_camera* camera, int width, int height, int bandRows, int rank, int world,
                           unsigned long long* masks, size_t capacity, size_t* numStrips, int* enabled, int* triPos) {
    if (!scene || !camera || !masks || !numStrips || !enabled || width <= 0 || height <= 0 || bandRows <= 0 || world <= 0 || rank < 0 || rank >= world ||
        ptpack::validateScene(*scene))
        return PTSS_HOST_EINVAL;
    int rows = 0;
    for (int y = 0; y < height; ++y)
        if ((y / bandRows) % world == rank) ++rows;
    const uint32_t numPixels = (uint32_t)width * (uint32_t)rows;
    const uint32_t plane = numPixels == 0 ? (uint32_t)ptss::kBlock : ((numPixels + ptss::kBlock - 1) / ptss::kBlock) * ptss::kBlock;   // ptss_create's capacity
    const size_t n = plane / ptloc::kStrip;
    *numStrips = n;
    if (capacity < n) return PTSS_HOST_EINVAL;
    std::vector<ptpack::PackedImage> images;
    try {
        images = ptpack::packImages(*scene, false);
    } catch (const std::bad_alloc&) {
        return PTSS_HOST_EINVAL;
    }
    // the image the frames of this camera use (ptss_api.hip selectImage), and whether bounce 0 culls on it (ptss_generate_frame)
    const bool inRange = ptpack::cameraInRange(*camera);
    const ptpack::PackedImage& im = images[(images.size() > 1 && !inRange) ? 1 : 0];
    const bool on = ptstrip::eligible(im.layout, im.layout.sphereBounded != 0 && inRange);
    *enabled = on ? 1 : 0;
    if (triPos && im.layout.numTriangles > 0) {
        if (im.layout.triClassed || ptss::meshImage(im.layout))
            std::memcpy(triPos, &im.blob[(size_t)im.layout.offTriPos], sizeof(int) * (size_t)im.layout.numTriangles);
        else
            for (int t = 0; t < im.layout.numTriangles; ++t) triPos[t] = t;
    }
    const ptstrip::View view{*camera, -2 * ptm::tan(camera->fieldOfView * 0.5f), (float)height / (float)width, 1.0f / width, 1.0f / height};   // eyeParams
    const ptstrip::Tile tile{width, rank, world, bandRows};
    for (size_t i = 0; i < n; ++i)
        masks[i] = on ? ptstrip::stripMask(view, tile, numPixels, (uint32_t)(i * ptloc::kStrip), reinterpret_cast<const float*>(im.blob.data()), im.layout)
                      : ptstrip::kAll;
    return PTSS_HOST_OK;
}

int ptss_probe_quantize(const float* x, unsigned int* out, size_t n) {
    if (!x || !out) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) out[i] = ptq::quantize_literal(x[i]);
    return PTSS_HOST_OK;
}

int ptss_probe_quant_table(float* out257) {
    if (!out257) return PTSS_HOST_EINVAL;
    float T[ptq::kTableFloats];
    if (!ptq::build_thresholds(T)) return PTSS_HOST_EINVAL;
    for (int k = 0; k <= 256; ++k) out257[k] = T[k];
    return PTSS_HOST_OK;
}

static const uint32_t* jumpTable() {
    static std::vector<uint32_t> table;
    if (table.empty()) {
        table.resize(ptrng::kJumpTableWords);
        ptrng::build_subsequence_table(table.data());
    }
    return table.data();
}

int ptss_probe_mesh_bound(const float* tri9, size_t ntri, const float* o3, const float* d3, size_t n, float margin, int* out, float* bound12) {
    if (!tri9 || ntri == 0 || ntri > (1u << 20) || (n && (!o3 || !d3 || !out))) return PTSS_HOST_EINVAL;
    float b[12];
    ptmesh::buildBound(tri9, (int)ntri, b);
    if (bound12)
        for (int k = 0; k < 12; ++k) bound12[k] = b[k];
    for (size_t i = 0; i < n; ++i) {
        const vec3 o = v3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = v3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
        out[i] = ptmesh::mayTouch(v3(b[0], b[1], b[2]), b[3], v3(b[4], b[5], b[6]), b[7], b[8], b[9], b[10], b[11], o, d, margin) ? 1 : 0;
    }
    return PTSS_HOST_OK;
}

int ptss_probe_mesh_refit(const float* tri9, size_t ntri, float* bounds12) {
    if (!tri9 || !bounds12 || ntri == 0 || ntri > (1u << 20)) return PTSS_HOST_EINVAL;
    const size_t leaves = (ntri + 15) / 16, groups = (leaves + 15) / 16;
    for (size_t k = 0; k < leaves; ++k)
        ptmesh::refitBound(tri9 + 9 * 16 * k, (int)(ntri - 16 * k < 16 ? ntri - 16 * k : 16), 16, bounds12 + 12 * k);
    for (size_t g = 0; g < groups; ++g)
        ptmesh::refitBound(tri9 + 9 * 256 * g, (int)(ntri - 256 * g < 256 ? ntri - 256 * g : 256), ptmesh::kRefitSlots, bounds12 + 12 * (leaves + g));
    return PTSS_HOST_OK;
}

static int probeKdOrder(const ptss_triangle* triangles, size_t n, int* position, bool canonicalZero) {
    if (!triangles || !position || n == 0 || n > (1u << 20)) return PTSS_HOST_EINVAL;
    std::vector<float> v(9 * n);
    for (size_t i = 0; i < n; ++i) {
        const ptss_vec3* p[3] = {&triangles[i].vertex0, &triangles[i].vertex1, &triangles[i].vertex2};
        for (int k = 0; k < 3; ++k) { v[9 * i + 3 * k] = p[k]->x; v[9 * i + 3 * k + 1] = p[k]->y; v[9 * i + 3 * k + 2] = p[k]->z; }
    }
    ptorder::kdPositions(v.data(), (int)n, position, canonicalZero);
    return PTSS_HOST_OK;
}
int ptss_probe_kd_order(const ptss_triangle* triangles, size_t n, int* position) { return probeKdOrder(triangles, n, position, true); }
int ptss_probe_kd_order_signed_zero(const ptss_triangle* triangles, size_t n, int* position) { return probeKdOrder(triangles, n, position, false); }

int ptss_probe_mesh_touch(const float* b, const float* o3, const float* d3, size_t n, float margin, int* out) {
    if (!b || (n && (!o3 || !d3 || !out))) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        const vec3 o = v3(o3[3 * i], o3[3 * i + 1], o3[3 * i + 2]), d = v3(d3[3 * i], d3[3 * i + 1], d3[3 * i + 2]);
        out[i] = ptmesh::mayTouch(v3(b[0], b[1], b[2]), b[3], v3(b[4], b[5], b[6]), b[7], b[8], b[9], b[10], b[11], o, d, margin) ? 1 : 0;
    }
    return PTSS_HOST_OK;
}

int ptss_probe_pack_scene(const ptss_scene_desc* scene, int everySphereLoop, int image, int* numImages, int* inLds, void* layout,
                          size_t layoutBytes, float* blob, size_t blobCapacity, size_t* blobWords) {
    if (!scene || ptpack::validateScene(*scene) || (everySphereLoop != 0 && everySphereLoop != 1)) return PTSS_HOST_EINVAL;
    const int n = ptpack::planImages(*scene, everySphereLoop != 0).numImages;
    if (numImages) *numImages = n;
    if (image < 0 || image >= n || (layout && layoutBytes != sizeof(ptss::SceneLayout))) return PTSS_HOST_EINVAL;
    if (!layout && !blob && !inLds && !blobWords) return PTSS_HOST_OK;
    std::vector<ptpack::PackedImage> images;
    try {
        images = ptpack::packImages(*scene, everySphereLoop != 0);
    } catch (const std::bad_alloc&) {
        return PTSS_HOST_EINVAL;
    }
    const ptpack::PackedImage& im = images[(size_t)image];
    const size_t words = im.blob.size() * 4;
    if (inLds) *inLds = im.inLds ? 1 : 0;
    if (layout) std::memcpy(layout, &im.layout, sizeof(im.layout));
    if (blobWords) *blobWords = words;
    if (blob) {
        if (blobCapacity < words) return PTSS_HOST_EINVAL;
        std::memcpy(blob, im.blob.data(), words * sizeof(float));
    }
    return PTSS_HOST_OK;
}

// the passes of ptss_denoise / ptss_denoise_history, plane to plane, from the colours in plane[0]
static int denoiseColours(std::vector<vec3> (&plane)[2], const ptss_pixel_feature* features, int width, int height, const ptss_denoise_params* params,
                          unsigned char* out_rgba, float* out_float) {
    const size_t n = (size_t)width * (size_t)height;
    auto featureAt = [&](int q) { return ptdn::Feature{features[q].normal, features[q].depth, features[q].materialIdx}; };
    auto depthAt = [&](int q) { return features[q].depth; };
    int cur = 0;
    for (int i = 0; i < params->levels; ++i) {
        const ptdn::Level lv = ptdn::levelOf(*params, i);
        const std::vector<vec3>& src = plane[cur];
        std::vector<vec3>& dst = plane[1 - cur];
        dst.resize(n);
        auto colourAt = [&](int q) { return src[(size_t)q]; };
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) dst[(size_t)y * width + x] = ptdn::filterPixel(x, y, width, height, lv, colourAt, featureAt, depthAt);
        cur = 1 - cur;
    }
    for (size_t p = 0; p < n; ++p) {
        const vec3 v = plane[cur][p];
        if (out_float) { out_float[3 * p] = v.x; out_float[3 * p + 1] = v.y; out_float[3 * p + 2] = v.z; }
        if (out_rgba) { out_rgba[4 * p] = ptdn::toByte(v.x); out_rgba[4 * p + 1] = ptdn::toByte(v.y); out_rgba[4 * p + 2] = ptdn::toByte(v.z); out_rgba[4 * p + 3] = 255; }
    }
    return PTSS_HOST_OK;
}

static bool denoiseArgumentsOk(const void* input, const ptss_pixel_feature* features, int width, int height, const ptss_denoise_params* params) {
    if (!input || !features || !params || width <= 0 || height <= 0) return false;
    if (params->structSize != (unsigned int)sizeof(ptss_denoise_params) || params->levels < 0 || params->levels > PTSS_DENOISE_MAX_LEVELS)
        return false;
    return params->sigmaColor > 0.0f && params->sigmaNormal > 0.0f && params->sigmaDepth >= 0.0f;
}

int ptss_probe_denoise(const uint32_t* accum, float inverseTicks, const ptss_pixel_feature* features, int width, int height,
                       const ptss_denoise_params* params, unsigned char* out_rgba, float* out_float) {
    if (!denoiseArgumentsOk(accum, features, width, height, params)) return PTSS_HOST_EINVAL;
    const size_t n = (size_t)width * (size_t)height;
    std::vector<vec3> plane[2];
    plane[0].resize(n);
    for (size_t p = 0; p < n; ++p) plane[0][p] = ptdn::displayValue(accum[3 * p], accum[3 * p + 1], accum[3 * p + 2], inverseTicks);
    return denoiseColours(plane, features, width, height, params, out_rgba, out_float);
}

int ptss_probe_denoise_history(const ptss_history_entry* history, const ptss_pixel_feature* features, int width, int height,
                               const ptss_denoise_params* params, unsigned char* out_rgba, float* out_float) {
    if (!denoiseArgumentsOk(history, features, width, height, params)) return PTSS_HOST_EINVAL;
    const size_t n = (size_t)width * (size_t)height;
    std::vector<vec3> plane[2];
    plane[0].resize(n);
    for (size_t p = 0; p < n; ++p) plane[0][p] = v3(history[p].r, history[p].g, history[p].b);
    return denoiseColours(plane, features, width, height, params, out_rgba, out_float);
}

int ptss_probe_upsample(const unsigned char* lo_rgba, const ptss_pixel_feature* features_lo, int width, int height,
                        const ptss_pixel_feature* features_hi, const ptss_upsample_params* params, unsigned char* out_rgba, float* out_float4) {
    if (!lo_rgba || !features_lo || !features_hi || !out_rgba || width <= 0 || height <= 0) return PTSS_HOST_EINVAL;
    if (ptup::paramsError(params) || out_rgba == lo_rgba) return PTSS_HOST_EINVAL;
    const int f = params->factor;
    if ((unsigned long long)width * (unsigned long long)height * (unsigned long long)(f * f) >= (1ull << 31)) return PTSS_HOST_EINVAL;
    const ptdn::Level lv = ptup::levelOf(*params);
    const int hiW = width * f, hiH = height * f;
    auto colourAt = [&](int q) {
        uint32_t w;
        std::memcpy(&w, lo_rgba + 4 * (size_t)q, 4);
        return w;
    };
    auto featureAt = [&](int q) { return ptdn::Feature{features_lo[q].normal, features_lo[q].depth, features_lo[q].materialIdx}; };
    auto depthAt = [&](int X, int Y) { return features_hi[(size_t)Y * hiW + X].depth; };
    for (int Y = 0; Y < hiH; ++Y)
        for (int X = 0; X < hiW; ++X) {
            const size_t p = (size_t)Y * hiW + X;
            const ptdn::Feature fp{features_hi[p].normal, features_hi[p].depth, features_hi[p].materialIdx};
            const ptup::Result r = ptup::upsamplePixel(X, Y, width, height, f, lv, fp, colourAt, featureAt, depthAt);
            const uint32_t px = ptup::packBytes(r.colour);
            std::memcpy(out_rgba + 4 * p, &px, 4);
            if (out_float4) { out_float4[4 * p] = r.colour.x; out_float4[4 * p + 1] = r.colour.y; out_float4[4 * p + 2] = r.colour.z; out_float4[4 * p + 3] = r.weight; }
        }
    return PTSS_HOST_OK;
}

int ptss_probe_upsample_axis(int X, int factor, int* x0, int* k, float* fx) {
    if (X < 0 || factor < 1 || factor > ptup::kMaxFactor || !x0 || !k || !fx) return PTSS_HOST_EINVAL;
    const ptup::Axis a = ptup::axisOf(X, factor);
    *x0 = a.x0;
    *k = a.k;
    *fx = a.f1;
    return PTSS_HOST_OK;
}

// ptss_probe_reproject / ptss_probe_reproject_motion: one loop; motion_now != nullptr: the point of a hit comes from its row
static int probeReproject(const uint32_t* accum, float inverseTicks, int n, const ptss_camera* camera_now, const ptss_camera* camera_prev, int width,
                          int height, const ptss_pixel_feature* features_now, const ptss_pixel_motion* motion_now,
                          const ptss_pixel_feature* features_prev, const ptss_history_entry* history_prev, const ptss_reproject_params* params,
                          ptss_history_entry* out) {
    if (!accum || !camera_now || !features_now || !out || width <= 0 || height <= 0 || n < 0) return PTSS_HOST_EINVAL;
    if (history_prev && (!camera_prev || !features_prev)) return PTSS_HOST_EINVAL;
    if (ptrp::paramsError(params) || out == history_prev) return PTSS_HOST_EINVAL;
    const ptrp::View now = ptrp::viewOf(*camera_now, width, height);
    const ptrp::View prev = history_prev ? ptrp::viewOf(*camera_prev, width, height) : now;
    const ptrp::Params prm = ptrp::paramsOf(*params);
    auto materialAt = [&](int q) { return features_prev[q].materialIdx; };
    auto geometryAt = [&](int q) { return ptrp::Geometry{features_prev[q].normal, features_prev[q].depth}; };
    auto historyAt = [&](int q) { return ptrp::Entry{v3(history_prev[q].r, history_prev[q].g, history_prev[q].b), history_prev[q].weight}; };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t p = (size_t)y * width + x;
            const vec3 cp = ptdn::displayValue(accum[3 * p], accum[3 * p + 1], accum[3 * p + 2], inverseTicks);
            ptrp::Entry e{cp, (float)n};
            if (history_prev) {
                const ptdn::Feature fp{features_now[p].normal, features_now[p].depth, features_now[p].materialIdx};
                if (motion_now) {
                    auto pointOf = [&](vec3) { return motion_now[p].prevPoint; };
                    e = ptrp::reprojectPixel(x, y, width, height, cp, (float)n, fp, now, prev, prm, pointOf, materialAt, geometryAt, historyAt);
                } else {
                    e = ptrp::reprojectPixel(x, y, width, height, cp, (float)n, fp, now, prev, prm, materialAt, geometryAt, historyAt);
                }
            }
            out[p] = ptss_history_entry{e.colour.x, e.colour.y, e.colour.z, e.weight};
        }
    return PTSS_HOST_OK;
}

int ptss_probe_reproject(const uint32_t* accum, float inverseTicks, int n, const ptss_camera* camera_now, const ptss_camera* camera_prev,
                         int width, int height, const ptss_pixel_feature* features_now, const ptss_pixel_feature* features_prev,
                         const ptss_history_entry* history_prev, const ptss_reproject_params* params, ptss_history_entry* out) {
    return probeReproject(accum, inverseTicks, n, camera_now, camera_prev, width, height, features_now, nullptr, features_prev, history_prev, params,
                          out);
}

int ptss_probe_reproject_motion(const uint32_t* accum, float inverseTicks, int n, const ptss_camera* camera_now, const ptss_camera* camera_prev,
                                int width, int height, const ptss_pixel_feature* features_now, const ptss_pixel_motion* motion_now,
                                const ptss_pixel_feature* features_prev, const ptss_history_entry* history_prev,
                                const ptss_reproject_params* params, ptss_history_entry* out) {
    if (!motion_now) return PTSS_HOST_EINVAL;
    return probeReproject(accum, inverseTicks, n, camera_now, camera_prev, width, height, features_now, motion_now, features_prev, history_prev,
                          params, out);
}

int ptss_probe_motion(const ptss_ray_query* rays, const ptss_ray_hit* hits, size_t n, const ptss_triangle* triangles_prev, size_t first,
                      size_t count, size_t numTriangles, ptss_pixel_motion* out) {
    if (n > 0 && (!rays || !hits || !out)) return PTSS_HOST_EINVAL;
    if (count > 0 && !triangles_prev) return PTSS_HOST_EINVAL;
    if (count > 0 && (numTriangles >= (size_t(1) << 31) || first >= numTriangles || count > numTriangles - first)) return PTSS_HOST_EINVAL;
    const float* prev = reinterpret_cast<const float*>(triangles_prev);
    for (size_t i = 0; i < n; ++i) {
        const ptss_ray_hit& h = hits[i];
        const ptmo::Motion m = ptmo::pixelMotion(rays[i].direction, rays[i].origin, h.kind, h.primitive, h.distance, h.w1, h.w2, prev,
                                                 count ? (uint32_t)first : 0u, (uint32_t)count);
        out[i] = ptss_pixel_motion{m.prevPoint, m.surface};
    }
    return PTSS_HOST_OK;
}

static ptsp::Material specularMaterial(const ptss_material& m) {
    return ptsp::Material{m.diffAvg, m.specAvg, m.refrAvg, m.specularExponent, m.indexOfRefraction, (int)(unsigned char)m.flags};
}

int ptss_probe_specular_step(const ptss_ray_query* rays, const ptss_ray_hit* hits, size_t n, const ptss_material* materials, size_t numMaterials,
                             ptss_ray_query* next, int* follows) {
    if (n > 0 && (!rays || !hits || !next || !follows)) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i)
        if (hits[i].kind != PTSS_HIT_MISS && (!materials || hits[i].materialIdx < 0 || (size_t)hits[i].materialIdx >= numMaterials))
            return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        const ptss_ray_hit& h = hits[i];
        follows[i] = 0;
        if (h.kind == PTSS_HIT_MISS) continue;
        const ptsp::Step s = ptsp::step(specularMaterial(materials[h.materialIdx]), rays[i].direction, h.point, h.normal);
        if (!s.follows) continue;
        follows[i] = 1;
        next[i] = ptss_ray_query{s.o, ptm::inf(), s.d, 0.0f};
    }
    return PTSS_HOST_OK;
}

int ptss_probe_specular_link(const ptss_ray_query* rays, const ptss_ray_hit* hits, size_t n, const ptss_material* materials, size_t numMaterials,
                             ptss_ray_query* next, int* follows, ptss_vec3* factors) {
    if (n > 0 && !factors) return PTSS_HOST_EINVAL;
    if (const int rc = ptss_probe_specular_step(rays, hits, n, materials, numMaterials, next, follows)) return rc;
    for (size_t i = 0; i < n; ++i) {
        if (!follows[i]) continue;
        const ptss_material& m = materials[hits[i].materialIdx];
        factors[i] = ptsp::linkFactor(specularMaterial(m), m.specularColor, rays[i].direction, hits[i].normal);
    }
    return PTSS_HOST_OK;
}

int ptss_probe_specular_class(const ptss_material* material) {
    return material ? (int)ptsp::classify(specularMaterial(*material)) : -1;
}

int ptss_probe_rng_init(unsigned long long seed, unsigned int subsequence, unsigned int* out6) {
    if (!out6) return PTSS_HOST_EINVAL;
    ptrng::State s = ptrng::seeded(seed);
    ptrng::skip_subsequences(s, subsequence, jumpTable());
    for (int i = 0; i < 5; ++i) out6[i] = s.v[i];
    out6[5] = s.d;
    return PTSS_HOST_OK;
}

int ptss_probe_rng_draw(unsigned int* state6, unsigned int* raw, float* uni, size_t n) {
    if (!state6) return PTSS_HOST_EINVAL;
    ptrng::State s;
    for (int i = 0; i < 5; ++i) s.v[i] = state6[i];
    s.d = state6[5];
    for (size_t i = 0; i < n; ++i) {
        ptrng::State before = s;
        const uint32_t r = ptrng::next(s);
        if (raw) raw[i] = r;
        if (uni) uni[i] = ptrng::uniform(before);
    }
    for (int i = 0; i < 5; ++i) state6[i] = s.v[i];
    state6[5] = s.d;
    return PTSS_HOST_OK;
}

int ptss_probe_rng_jump_table(unsigned int* out, size_t words) {
    if (!out || words != (size_t)ptrng::kJumpTableWords) return PTSS_HOST_EINVAL;
    std::memcpy(out, jumpTable(), words * sizeof(uint32_t));
    return PTSS_HOST_OK;
}

// ptss_probe_film_rays and, with positions, ptss_probe_film_positions
static int probeFilmRays(const ptss_film_camera* film, size_t firstPixel, const uint32_t* index, size_t n, ptss_path_rng* rng, ptss_ray_query* rays,
                         ptss_film_position* positions, unsigned long long* rejected) {
    if (ptcam::cameraError(film)) return PTSS_HOST_EINVAL;
    const unsigned long long filmPixels = (unsigned long long)film->width * (unsigned long long)film->height;
    if (filmPixels >= (1ull << 31) || n >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (n > 0 && (!rng || !rays)) return PTSS_HOST_EINVAL;
    if (!index && (firstPixel > filmPixels || n > filmPixels - firstPixel)) return PTSS_HOST_EINVAL;
    const ptcam::Film F = ptcam::filmOf(*film);
    unsigned long long dropped = 0;
    for (size_t i = 0; i < n; ++i) {
        const unsigned long long p = index ? index[i] : firstPixel + i;
        if (p >= filmPixels) {
            ++dropped;
            if (positions) positions[i] = ptss_film_position{ptm::qnan(), ptm::qnan()};
            continue;
        }
        float jx = 0.5f, jy = 0.5f, u1 = 0.0f, u2 = 0.0f;
        if (F.jitter) {
            ptrng::State st;
            for (int w = 0; w < 5; ++w) st.v[w] = rng[i].v[w];
            st.d = rng[i].d;
            jx = ptrng::uniform(st);
            jy = ptrng::uniform(st);
            if (F.kind == PTSS_FILM_THIN_LENS) {
                u1 = ptrng::uniform(st);
                u2 = ptrng::uniform(st);
            }
            for (int w = 0; w < 5; ++w) rng[i].v[w] = st.v[w];
            rng[i].d = st.d;
        }
        const int x = (int)(p % (unsigned long long)F.width), y = (int)(p / (unsigned long long)F.width);
        rays[i] = ptcam::filmRay(F, x, y, jx, jy, u1, u2);
        if (positions) ptcam::samplePosition(x, y, jx, jy, positions[i].x, positions[i].y);
    }
    if (rejected) *rejected = dropped;
    return PTSS_HOST_OK;
}

int ptss_probe_film_rays(const ptss_film_camera* film, size_t firstPixel, const uint32_t* index, size_t n, ptss_path_rng* rng,
                         ptss_ray_query* rays, unsigned long long* rejected) {
    return probeFilmRays(film, firstPixel, index, n, rng, rays, nullptr, rejected);
}

int ptss_probe_film_positions(const ptss_film_camera* film, size_t firstPixel, const uint32_t* index, size_t n, ptss_path_rng* rng,
                              ptss_ray_query* rays, ptss_film_position* positions, unsigned long long* rejected) {
    if (!positions) return PTSS_HOST_EINVAL;
    return probeFilmRays(film, firstPixel, index, n, rng, rays, positions, rejected);
}

int ptss_probe_accumulate(const ptss_path_result* results, const uint32_t* index, size_t firstPixel, size_t n, ptss_film_entry* film,
                          size_t filmPixels, ptss_uchar4* pixels, ptss_history_entry* history, unsigned long long* rejected) {
    if (filmPixels >= (size_t(1) << 31) || n >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (n > 0 && (!results || !film)) return PTSS_HOST_EINVAL;
    if (!index && (firstPixel > filmPixels || n > filmPixels - firstPixel)) return PTSS_HOST_EINVAL;
    unsigned long long dropped = 0;
    for (size_t i = 0; i < n; ++i) {   // the sums
        const size_t p = index ? index[i] : firstPixel + i;
        if (p >= filmPixels) {
            ++dropped;
            continue;
        }
        film[p].r += ptq::quantize_literal(results[i].radiance.x);
        film[p].g += ptq::quantize_literal(results[i].radiance.y);
        film[p].b += ptq::quantize_literal(results[i].radiance.z);
        film[p].samples += 1u;
    }
    for (size_t i = 0; i < n; ++i) {   // every pixel touched, resolved from its final sums
        const size_t p = index ? index[i] : firstPixel + i;
        if (p >= filmPixels) continue;
        const ptss_film_entry e = film[p];
        const float inv = 1.f / (float)e.samples;
        if (pixels) pixels[p] = ptss_uchar4{(unsigned char)(e.r * inv + 0.5f), (unsigned char)(e.g * inv + 0.5f), (unsigned char)(e.b * inv + 0.5f), 255};
        if (history) {
            const vec3 c = ptdn::displayValue(e.r, e.g, e.b, inv);
            history[p] = ptss_history_entry{c.x, c.y, c.z, (float)e.samples};
        }
    }
    if (rejected) *rejected = dropped;
    return PTSS_HOST_OK;
}

int ptss_probe_accumulate_stats(const ptss_path_result* results, const uint32_t* index, size_t firstPixel, size_t n, ptss_film_entry* film,
                                unsigned long long* moments, size_t filmPixels, ptss_uchar4* pixels, ptss_history_entry* history,
                                unsigned long long* rejected) {
    if (n > 0 && !moments) return PTSS_HOST_EINVAL;
    const int rc = ptss_probe_accumulate(results, index, firstPixel, n, film, filmPixels, pixels, history, rejected);
    if (rc != PTSS_HOST_OK) return rc;
    for (size_t i = 0; i < n; ++i) {
        const size_t p = index ? index[i] : firstPixel + i;
        if (p >= filmPixels) continue;
        moments[p] += ptad::squares(ptq::quantize_literal(results[i].radiance.x), ptq::quantize_literal(results[i].radiance.y),
                                    ptq::quantize_literal(results[i].radiance.z));
    }
    return PTSS_HOST_OK;
}

int ptss_probe_plan_samples(const ptss_film_entry* film, const unsigned long long* moments, size_t filmPixels, const ptss_plan_params* params,
                            size_t n, unsigned long long* cdf, uint32_t* index, ptss_plan_info* info) {
    if (ptad::paramsError(params)) return PTSS_HOST_EINVAL;
    if (filmPixels == 0 || filmPixels >= (size_t(1) << 31) || n >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (n == 0) return PTSS_HOST_OK;
    if (!film || !moments || !cdf || !index) return PTSS_HOST_EINVAL;
    planSamples(filmPixels, n, cdf, index, info, [&](size_t p, uint32_t* kind) {
        return ptad::weight(film[p].r, film[p].g, film[p].b, film[p].samples, moments[p], params->minSamples, params->maxSamples, params->threshold, kind);
    });
    return PTSS_HOST_OK;
}

uint32_t ptss_probe_plan_weight(const ptss_film_entry* entry, unsigned long long moment, const ptss_plan_params* params) {
    if (!entry || ptad::paramsError(params)) return 0xffffffffu;
    return ptad::weight(entry->r, entry->g, entry->b, entry->samples, moment, params->minSamples, params->maxSamples, params->threshold, nullptr);
}

unsigned long long ptss_probe_plan_target(unsigned long long i, unsigned long long n, unsigned long long total) {
    return n ? ptad::target(i, n, total) : 0ull;
}

// ptss_probe_accumulate_linear and ptss_probe_accumulate_linear_stats: the film, the moments or both take the samples (at least one is
// there: the callers have checked), as the device's linearAccumulateKernel<kFilm, kMoments> does
static int probeAccumulateLinear(const ptss_path_result* results, const uint32_t* index, size_t firstPixel, size_t n, ptss_linear_entry* film,
                                 ptss_linear_moment* moments, size_t filmPixels, const ptss_linear_params* params, unsigned long long* rejected) {
    if (filmPixels >= (size_t(1) << 31) || n >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (n > 0 && !results) return PTSS_HOST_EINVAL;
    if (!index && (firstPixel > filmPixels || n > filmPixels - firstPixel)) return PTSS_HOST_EINVAL;
    const ptlin::Scale sc = ptlin::scaleOf(*params);
    unsigned long long dropped = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t p = index ? index[i] : firstPixel + i;
        if (p >= filmPixels) {
            ++dropped;
            continue;
        }
        ptlin::u64 q[3];
        const uint32_t flag = ptlin::sampleToFixed(results[i].radiance.x, results[i].radiance.y, results[i].radiance.z, sc, q);
        if (moments) {
            const ptls::Sample s = ptls::sampleOf(q[0], q[1], q[2]);
            moments[p].sumY += s.y;
            moments[p].sqLo += s.lo;
            moments[p].sqHi += s.hi;
            moments[p].samples += 1ull;
        }
        if (film) {
            film[p].r += q[0];
            film[p].g += q[1];
            film[p].b += q[2];
            film[p].samples += 1u;
            film[p].clamped += flag;
        }
    }
    if (rejected) *rejected = dropped;
    return PTSS_HOST_OK;
}

int ptss_probe_accumulate_linear(const ptss_path_result* results, const uint32_t* index, size_t firstPixel, size_t n, ptss_linear_entry* film,
                                 size_t filmPixels, const ptss_linear_params* params, unsigned long long* rejected) {
    if (ptlin::paramsError(params) || (n > 0 && !film)) return PTSS_HOST_EINVAL;
    return probeAccumulateLinear(results, index, firstPixel, n, film, nullptr, filmPixels, params, rejected);
}

int ptss_probe_accumulate_linear_stats(const ptss_path_result* results, const uint32_t* index, size_t firstPixel, size_t n, ptss_linear_entry* film,
                                       ptss_linear_moment* moments, size_t filmPixels, const ptss_linear_params* params,
                                       unsigned long long* rejected) {
    if (ptlin::paramsError(params) || (n > 0 && !moments)) return PTSS_HOST_EINVAL;
    return probeAccumulateLinear(results, index, firstPixel, n, film, moments, filmPixels, params, rejected);
}

int ptss_probe_plan_samples_linear(const ptss_linear_moment* moments, size_t filmPixels, const ptss_linear_params* params,
                                   const ptss_linear_plan_params* plan, size_t n, unsigned long long* cdf, uint32_t* index, ptss_plan_info* info) {
    if (ptlin::paramsError(params) || ptls::paramsError(plan, params)) return PTSS_HOST_EINVAL;
    if (filmPixels == 0 || filmPixels >= (size_t(1) << 31) || n >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (n == 0) return PTSS_HOST_OK;
    if (!moments || !cdf || !index) return PTSS_HOST_EINVAL;
    const ptls::Rule rule = ptls::ruleOf(*plan, *params);
    planSamples(filmPixels, n, cdf, index, info, [&](size_t p, uint32_t* kind) {
        return ptls::weight(moments[p].sumY, moments[p].sqLo, moments[p].sqHi, moments[p].samples, rule, kind);
    });
    return PTSS_HOST_OK;
}

uint32_t ptss_probe_linear_plan_weight(const ptss_linear_moment* moment, const ptss_linear_params* params, const ptss_linear_plan_params* plan) {
    if (!moment || ptlin::paramsError(params) || ptls::paramsError(plan, params)) return 0xffffffffu;
    return ptls::weight(moment->sumY, moment->sqLo, moment->sqHi, moment->samples, ptls::ruleOf(*plan, *params), nullptr);
}

int ptss_probe_resolve_linear(const ptss_linear_entry* film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                              ptss_history_entry* linear, ptss_uchar4* pixels, ptss_history_entry* history) {
    if (ptlin::paramsError(params)) return PTSS_HOST_EINVAL;
    if (count == 0) return PTSS_HOST_OK;
    if (!film || firstPixel >= (size_t(1) << 31) || count >= (size_t(1) << 31) || firstPixel + count >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    const ptlin::Scale sc = ptlin::scaleOf(*params);
    for (size_t p = firstPixel; p < firstPixel + count; ++p) {
        float lin[4], hist[4];
        uint32_t px;
        ptlin::resolve(film[p].r, film[p].g, film[p].b, film[p].samples, sc, nullptr, lin, &px, hist);
        if (linear) linear[p] = ptss_history_entry{lin[0], lin[1], lin[2], lin[3]};
        if (pixels) pixels[p] = ptss_uchar4{(unsigned char)px, (unsigned char)(px >> 8), (unsigned char)(px >> 16), (unsigned char)(px >> 24)};
        if (history) history[p] = ptss_history_entry{hist[0], hist[1], hist[2], hist[3]};
    }
    return PTSS_HOST_OK;
}

int ptss_probe_splat_paths(const ptss_path_result* results, const ptss_film_position* positions, const size_t* firstPixel, size_t n,
                           ptss_splat_entry* film, int width, int height, const ptss_splat_filter* filter, const ptss_linear_params* params,
                           unsigned long long* dropped, unsigned long long* clamped) {
    if (ptspl::filterError(filter) || ptlin::paramsError(params)) return PTSS_HOST_EINVAL;
    if (width < 1 || height < 1 || width > ptspl::kMaxFilmSide || height > ptspl::kMaxFilmSide) return PTSS_HOST_EINVAL;
    const unsigned long long filmPixels = (unsigned long long)width * (unsigned long long)height;
    if (filmPixels >= (1ull << 31) || n >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (n > 0 && (!results || !positions || !film)) return PTSS_HOST_EINVAL;
    if (firstPixel && (*firstPixel > filmPixels || n > filmPixels - *firstPixel)) return PTSS_HOST_EINVAL;
    const ptspl::Filter F = ptspl::filterOf(*filter);
    const ptlin::Scale sc = ptlin::scaleOf(*params);
    unsigned long long nDropped = 0, nClamped = 0;
    for (size_t i = 0; i < n; ++i) {
        const float X = positions[i].x, Y = positions[i].y;
        bool drop = ptspl::outside(X, F.radius, width) || ptspl::outside(Y, F.radius, height);
        if (firstPixel) {
            const unsigned long long home = *firstPixel + i;
            drop = ptspl::stray(X, Y, (int)(home % (unsigned long long)width), (int)(home / (unsigned long long)width));
        }
        if (drop) {
            ++nDropped;
            continue;
        }
        ptlin::u64 q[3];
        nClamped += ptlin::sampleToFixed(results[i].radiance.x, results[i].radiance.y, results[i].radiance.z, sc, q);
        const int x0 = ptspl::firstTap(F, X), y0 = ptspl::firstTap(F, Y);
        for (int y = y0; y <= y0 + 2 * F.reach; ++y) {
            if (y < 0 || y >= height) continue;
            const uint32_t wy = ptspl::axisWeight(F, Y, y);
            for (int x = x0; x <= x0 + 2 * F.reach; ++x) {
                if (x < 0 || x >= width) continue;
                const uint32_t W = ptspl::tapWeight(ptspl::axisWeight(F, X, x), wy);
                if (W == 0u) continue;
                ptss_splat_entry& e = film[(size_t)y * (size_t)width + (size_t)x];
                e.r += ptspl::contribution(q[0], W);
                e.g += ptspl::contribution(q[1], W);
                e.b += ptspl::contribution(q[2], W);
                e.weight += W;
            }
        }
    }
    if (dropped) *dropped = nDropped;
    if (clamped) *clamped = nClamped;
    return PTSS_HOST_OK;
}

int ptss_probe_resolve_splat(const ptss_splat_entry* film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             ptss_history_entry* linear, ptss_uchar4* pixels, ptss_history_entry* history) {
    if (ptlin::paramsError(params)) return PTSS_HOST_EINVAL;
    if (count == 0) return PTSS_HOST_OK;
    if (!film || firstPixel >= (size_t(1) << 31) || count >= (size_t(1) << 31) || firstPixel + count >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    const ptlin::Scale sc = ptlin::scaleOf(*params);
    for (size_t p = firstPixel; p < firstPixel + count; ++p) {
        float lin[4], hist[4];
        uint32_t px;
        ptspl::resolve(film[p].r, film[p].g, film[p].b, film[p].weight, sc, nullptr, lin, &px, hist);
        if (linear) linear[p] = ptss_history_entry{lin[0], lin[1], lin[2], lin[3]};
        if (pixels) pixels[p] = ptss_uchar4{(unsigned char)px, (unsigned char)(px >> 8), (unsigned char)(px >> 16), (unsigned char)(px >> 24)};
        if (history) history[p] = ptss_history_entry{hist[0], hist[1], hist[2], hist[3]};
    }
    return PTSS_HOST_OK;
}

int ptss_probe_meter_bin(const unsigned long long* entry4, int splat, int* bin, unsigned long long* luminance) {
    if (!entry4 || !bin) return PTSS_HOST_EINVAL;
    const ptlin::u64 r = entry4[0], g = entry4[1], b = entry4[2], w = splat ? entry4[3] : (entry4[3] & 0xffffffffull);
    *bin = splat ? ptmeter::binOfSplat(r, g, b, w) : ptmeter::binOfLinear(r, g, b, (uint32_t)w);
    if (luminance) {
        *luminance = 0ull;
        if (w != 0ull)
            *luminance = splat ? ptmeter::luminance(ptmeter::splatMean(r, w), ptmeter::splatMean(g, w), ptmeter::splatMean(b, w))
                               : ptmeter::luminance(ptmeter::linearMean(r, w), ptmeter::linearMean(g, w), ptmeter::linearMean(b, w));
    }
    return PTSS_HOST_OK;
}

static bool meterRangeOk(const void* film, size_t firstPixel, size_t count, const uint32_t* histogram) {
    return film && histogram && firstPixel < (size_t(1) << 31) && count < (size_t(1) << 31) && firstPixel + count < (size_t(1) << 31);
}

int ptss_probe_meter_linear(const ptss_linear_entry* film, size_t firstPixel, size_t count, uint32_t* histogram) {
    if (count == 0) return PTSS_HOST_OK;
    if (!meterRangeOk(film, firstPixel, count, histogram)) return PTSS_HOST_EINVAL;
    for (size_t p = firstPixel; p < firstPixel + count; ++p) {
        const int bin = ptmeter::binOfLinear(film[p].r, film[p].g, film[p].b, film[p].samples);
        if (bin != ptmeter::kNoBin) histogram[bin] += 1u;
    }
    return PTSS_HOST_OK;
}

int ptss_probe_meter_splat(const ptss_splat_entry* film, size_t firstPixel, size_t count, uint32_t* histogram) {
    if (count == 0) return PTSS_HOST_OK;
    if (!meterRangeOk(film, firstPixel, count, histogram)) return PTSS_HOST_EINVAL;
    for (size_t p = firstPixel; p < firstPixel + count; ++p) {
        const int bin = ptmeter::binOfSplat(film[p].r, film[p].g, film[p].b, film[p].weight);
        if (bin != ptmeter::kNoBin) histogram[bin] += 1u;
    }
    return PTSS_HOST_OK;
}

int ptss_probe_meter_exposure(const uint32_t* histogram, const ptss_linear_params* params, const ptss_meter_params* meter, ptss_meter_state* state) {
    if (ptlin::paramsError(params) || ptmeter::paramsError(meter) || !histogram || !state) return PTSS_HOST_EINVAL;
    ptmeter::update(histogram, ptmeter::ruleOf(*meter, *params), state);
    return PTSS_HOST_OK;
}

int ptss_glare_layout(int width, int height, int levels, ptss_glare_level out[8], size_t* entries) {
    if (!out || !entries || levels < 1 || levels > ptglare::kMaxLevels || ptglare::sidesError(width, height)) return PTSS_HOST_EINVAL;
    *entries = ptglare::layoutOf(width, height, levels, out);
    return PTSS_HOST_OK;
}

// word 3 of a film entry as the glare operations take it: the samples of a linear entry, the weight of a filtered one
static ptlin::u64 glareWeightOf(const unsigned long long* entry4, bool splat) { return splat ? entry4[3] : (entry4[3] & 0xffffffffull); }

static bool glareArgumentsOk(const void* film, int filmKind, int width, int height, const ptss_linear_params* params, const ptss_glare_params* glare,
                             const void* pyramid) {
    if (ptlin::paramsError(params) || ptglare::paramsError(glare, *params) || ptglare::sidesError(width, height)) return false;
    return film && pyramid && (filmKind == PTSS_GLARE_FILM_LINEAR || filmKind == PTSS_GLARE_FILM_SPLAT);
}

int ptss_probe_glare_build(const void* film, int filmKind, int width, int height, const ptss_linear_params* params, const ptss_glare_params* glare,
                           ptss_glare_entry* pyramid) {
    if (!glareArgumentsOk(film, filmKind, width, height, params, glare, pyramid)) return PTSS_HOST_EINVAL;
    const bool splat = filmKind == PTSS_GLARE_FILM_SPLAT;
    const unsigned long long* words = static_cast<const unsigned long long*>(film);
    const ptglare::Rule R = ptglare::ruleOf(*glare, *params);
    const int L = glare->levels;
    ptss_glare_level lv[ptglare::kMaxLevels];
    ptglare::layoutOf(width, height, L, lv);
    // the downs: level 1 from the film's thresholded means, level k from level k - 1
    for (int k = 1; k <= L; ++k) {
        ptss_glare_entry* dst = pyramid + lv[k - 1].first;
        const int w = lv[k - 1].width, h = lv[k - 1].height;
        const int sw = k == 1 ? width : lv[k - 2].width, sh = k == 1 ? height : lv[k - 2].height;
        const ptss_glare_entry* src = k == 1 ? nullptr : pyramid + lv[k - 2].first;
        for (int j = 0; j < h; ++j)
            for (int i = 0; i < w; ++i) {
                ptlin::u64 d[3];
                if (k == 1)
                    ptglare::downTexel(i, j, sw, sh, [&](int x, int y, ptlin::u64* v) {
                        const unsigned long long* e = words + 4 * ((size_t)y * (size_t)sw + (size_t)x);
                        ptglare::sourceOf(e[0], e[1], e[2], glareWeightOf(e, splat), splat, R.threshold, v);
                    }, d);
                else
                    ptglare::downTexel(i, j, sw, sh, [&](int x, int y, ptlin::u64* v) {
                        const ptss_glare_entry& e = src[(size_t)y * (size_t)sw + (size_t)x];
                        v[0] = e.r, v[1] = e.g, v[2] = e.b;
                    }, d);
                dst[(size_t)j * (size_t)w + (size_t)i] = ptss_glare_entry{d[0], d[1], d[2], 0ull};
            }
    }
    // the ups, in place from the coarsest level
    for (int k = L - 1; k >= 1; --k) {
        ptss_glare_entry* dst = pyramid + lv[k - 1].first;
        const ptss_glare_entry* src = pyramid + lv[k].first;
        const int w = lv[k - 1].width, h = lv[k - 1].height, cw = lv[k].width, ch = lv[k].height;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                ptlin::u64 u[3];
                ptglare::upTexel(x, y, cw, ch, [&](int i, int j, ptlin::u64* v) {
                    const ptss_glare_entry& e = src[(size_t)j * (size_t)cw + (size_t)i];
                    v[0] = e.r, v[1] = e.g, v[2] = e.b;
                }, u);
                ptss_glare_entry& e = dst[(size_t)y * (size_t)w + (size_t)x];
                e.r += u[0], e.g += u[1], e.b += u[2];
            }
    }
    return PTSS_HOST_OK;
}

int ptss_probe_resolve_glare(const void* film, int filmKind, size_t firstPixel, size_t count, const ptss_linear_params* params, int width, int height,
                             const ptss_glare_params* glare, const ptss_glare_entry* pyramid, const ptss_meter_state* state,
                             ptss_history_entry* linear, ptss_uchar4* pixels, ptss_history_entry* history) {
    if (ptlin::paramsError(params) || ptglare::paramsError(glare, *params) || ptglare::sidesError(width, height)) return PTSS_HOST_EINVAL;
    if (filmKind != PTSS_GLARE_FILM_LINEAR && filmKind != PTSS_GLARE_FILM_SPLAT) return PTSS_HOST_EINVAL;
    if (count == 0) return PTSS_HOST_OK;
    const size_t filmPixels = (size_t)width * (size_t)height;
    if (!film || !pyramid || firstPixel > filmPixels || count > filmPixels - firstPixel) return PTSS_HOST_EINVAL;
    const bool splat = filmKind == PTSS_GLARE_FILM_SPLAT;
    const unsigned long long* words = static_cast<const unsigned long long*>(film);
    const ptglare::Rule R = ptglare::ruleOf(*glare, *params);
    ptlin::Scale sc = ptlin::scaleOf(*params);
    if (state) sc.exposure = state->exposure * sc.exposure;
    const int cw = ptglare::halfOf(width), ch = ptglare::halfOf(height);
    for (size_t p = firstPixel; p < firstPixel + count; ++p) {
        ptlin::u64 up[3];
        ptglare::upTexel((int)(p % (size_t)width), (int)(p / (size_t)width), cw, ch, [&](int i, int j, ptlin::u64* v) {
            const ptss_glare_entry& e = pyramid[(size_t)j * (size_t)cw + (size_t)i];
            v[0] = e.r, v[1] = e.g, v[2] = e.b;
        }, up);
        const unsigned long long* e = words + 4 * p;
        float lin[4], hist[4];
        uint32_t px;
        ptglare::resolve(e[0], e[1], e[2], glareWeightOf(e, splat), splat, up, R, sc, nullptr, lin, &px, hist);
        if (linear) linear[p] = ptss_history_entry{lin[0], lin[1], lin[2], lin[3]};
        if (pixels) pixels[p] = ptss_uchar4{(unsigned char)px, (unsigned char)(px >> 8), (unsigned char)(px >> 16), (unsigned char)(px >> 24)};
        if (history) history[p] = ptss_history_entry{hist[0], hist[1], hist[2], hist[3]};
    }
    return PTSS_HOST_OK;
}

// ---- tone curves for the two linear films (csrc/pttone.h) ----
int ptss_probe_tone_build(const ptss_tone_params* params, float* table) {
    if (pttone::paramsError(params) || !table) return PTSS_HOST_EINVAL;
    return pttone::buildTable(*params, table) ? PTSS_HOST_OK : PTSS_HOST_ERANGE;   // unsorted: the table is written all the same, its flag set
}

int ptss_probe_tone_value(const ptss_tone_params* params, const float* x, float* v, size_t n) {
    if (pttone::paramsError(params)) return PTSS_HOST_EINVAL;
    if (n == 0) return PTSS_HOST_OK;
    if (!x || !v) return PTSS_HOST_EINVAL;
    const pttone::Stage S = pttone::stageOf(*params, params->curve);
    for (size_t i = 0; i < n; ++i) v[i] = pttone::valueOf(S, x[i]);
    return PTSS_HOST_OK;
}

int ptss_probe_tone_level(const float* table, int bits, const float* x, uint32_t* level, size_t n) {
    if (bits != 8 && bits != 10) return PTSS_HOST_EINVAL;
    if (n == 0) return PTSS_HOST_OK;
    if (!table || !x || !level) return PTSS_HOST_EINVAL;
    for (size_t i = 0; i < n; ++i) level[i] = pttone::levelCount(table, pttone::topOf(bits), x[i]);
    return PTSS_HOST_OK;
}

int ptss_probe_resolve_toned(const void* film, int filmKind, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             const ptss_tone_params* tone, const float* table, const ptss_meter_state* state, int width, int height,
                             const ptss_glare_params* glare, const ptss_glare_entry* pyramid, ptss_history_entry* linear, uint32_t* pixels,
                             ptss_history_entry* history) {
    if (ptlin::paramsError(params) || pttone::paramsError(tone)) return PTSS_HOST_EINVAL;
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return PTSS_HOST_EINVAL;
    if ((glare == nullptr) != (pyramid == nullptr)) return PTSS_HOST_EINVAL;
    if (glare && (ptglare::paramsError(glare, *params) || ptglare::sidesError(width, height))) return PTSS_HOST_EINVAL;
    if (count == 0) return PTSS_HOST_OK;
    if (!film || !table || firstPixel >= (size_t(1) << 31) || count >= (size_t(1) << 31) || firstPixel + count >= (size_t(1) << 31)) return PTSS_HOST_EINVAL;
    if (glare) {
        const size_t filmPixels = (size_t)width * (size_t)height;
        if (firstPixel > filmPixels || count > filmPixels - firstPixel) return PTSS_HOST_EINVAL;
    }
    const bool splat = filmKind == PTSS_FILM_SPLAT;
    const unsigned long long* words = static_cast<const unsigned long long*>(film);
    const pttone::Rule R = pttone::ruleOf(*tone);
    ptglare::Rule G{};
    if (glare) G = ptglare::ruleOf(*glare, *params);
    ptlin::Scale sc = ptlin::scaleOf(*params);
    if (state) sc.exposure = state->exposure * sc.exposure;
    const int cw = ptglare::halfOf(width), ch = ptglare::halfOf(height);
    const uint32_t K = R.shown.K;
    for (size_t p = firstPixel; p < firstPixel + count; ++p) {
        ptlin::u64 up[3] = {0ull, 0ull, 0ull};
        if (glare)
            ptglare::upTexel((int)(p % (size_t)width), (int)(p / (size_t)width), cw, ch, [&](int i, int j, ptlin::u64* v) {
                const ptss_glare_entry& e = pyramid[(size_t)j * (size_t)cw + (size_t)i];
                v[0] = e.r, v[1] = e.g, v[2] = e.b;
            }, up);
        const unsigned long long* e = words + 4 * p;
        float lin[4], hist[4];
        uint32_t px;
        pttone::resolve(e[0], e[1], e[2], glareWeightOf(e, splat), splat, glare ? up : nullptr, &G, sc, R,
                        [&](float x) { return pttone::levelCount(table, K, x); }, lin, &px, hist);
        if (linear) linear[p] = ptss_history_entry{lin[0], lin[1], lin[2], lin[3]};
        if (pixels) pixels[p] = px;
        if (history) history[p] = ptss_history_entry{hist[0], hist[1], hist[2], hist[3]};
    }
    return PTSS_HOST_OK;
}

// ---- the denoiser of the two linear films (csrc/ptlindn.h) ----
int ptss_probe_denoise_linear(const void* film, int filmKind, int width, int height, const ptss_linear_moment* moments,
                              const ptss_pixel_feature* features, const ptss_linear_params* params, const ptss_denoise_linear_params* denoise,
                              ptss_linear_entry* out, float* out_plane) {
    if (ptlin::paramsError(params) || ptldn::paramsError(denoise) || ptldn::sidesError(width, height)) return PTSS_HOST_EINVAL;
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return PTSS_HOST_EINVAL;
    if (!film || !moments || !features || !out || (const void*)out == film) return PTSS_HOST_EINVAL;
    const bool splat = filmKind == PTSS_FILM_SPLAT;
    const unsigned long long* words = static_cast<const unsigned long long*>(film);
    unsigned long long* result = reinterpret_cast<unsigned long long*>(out);
    const ptldn::Rule R = ptldn::ruleOf(*denoise, *params);
    const size_t n = (size_t)width * (size_t)height;
    const int L = denoise->levels;
    std::vector<ptldn::Row> plane[2];
    plane[0].resize(n);
    if (L > 1) plane[1].resize(n);
    for (size_t p = 0; p < n; ++p) {
        const unsigned long long* e = words + 4 * p;
        plane[0][p] = ptldn::prepare(e[0], e[1], e[2], e[3], splat, moments[p].sumY, moments[p].sqLo, moments[p].sqHi, moments[p].samples, R);
        if (L == 0) ptldn::finishMeans(e[0], e[1], e[2], e[3], splat, result + 4 * p);
    }
    std::vector<ptldn::Row> final;
    if (L > 0) final.resize(n);
    auto featureAt = [&](int qx, int qy) {
        const ptss_pixel_feature& f = features[(size_t)qy * (size_t)width + (size_t)qx];
        return ptdn::Feature{f.normal, f.depth, f.materialIdx};
    };
    for (int i = 0; i < L; ++i) {
        const std::vector<ptldn::Row>& src = plane[ptldn::sourcePlane(i)];
        std::vector<ptldn::Row>& dst = i + 1 == L ? final : plane[1 - ptldn::sourcePlane(i)];
        auto rowAt = [&](int qx, int qy) { return src[(size_t)qy * (size_t)width + (size_t)qx]; };
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) dst[(size_t)y * (size_t)width + (size_t)x] = ptldn::filterPixel(x, y, width, height, 1 << i, R, rowAt, featureAt);
    }
    if (L > 0)
        for (size_t p = 0; p < n; ++p) ptldn::finishRow(final[p], words[4 * p + 3], splat, R, result + 4 * p);
    if (out_plane) {
        const std::vector<ptldn::Row>& shown = L > 0 ? final : plane[0];
        for (size_t p = 0; p < n; ++p) {
            out_plane[4 * p] = shown[p].c.x, out_plane[4 * p + 1] = shown[p].c.y, out_plane[4 * p + 2] = shown[p].c.z;
            out_plane[4 * p + 3] = shown[p].v;
        }
    }
    return PTSS_HOST_OK;
}

int ptss_probe_denoise_linear_finish(const float* rgb, unsigned long long word3, int filmKind, const ptss_linear_params* params,
                                     unsigned long long* out4) {
    if (!rgb || !out4 || ptlin::paramsError(params) || (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT)) return PTSS_HOST_EINVAL;
    ptss_denoise_linear_params d{};
    d.sigmaLuminance = d.sigmaNormal = d.sigmaDepth = 1.f;
    const ptldn::Rule R = ptldn::ruleOf(d, *params);
    const bool splat = filmKind == PTSS_FILM_SPLAT;
    const ptldn::Row row{v3(rgb[0], rgb[1], rgb[2]), ptldn::weightOf(word3, splat) == 0ull ? ptldn::kEmpty : 0.f};
    ptldn::finishRow(row, word3, splat, R, out4);
    return PTSS_HOST_OK;
}

// ---- carrying the two linear films across a camera move (csrc/ptlinrp.h) ----
extern "C++" {
template <bool Moments>
static void probeReprojectLinear(const ptcam::Film& now, const ptss_pixel_feature* features_now, const ptss_pixel_motion* motion_now,
                                 const ptlrp::Prev& prev, const ptss_pixel_feature* features_prev, const unsigned long long* film_prev, bool splat,
                                 const ptss_linear_moment* moments_prev, const ptlrp::Rule& R, unsigned long long* film_out,
                                 ptss_linear_moment* moments_out, ptss_reproject_linear_info* info) {
    auto materialAt = [&](size_t q) { return features_prev[q].materialIdx; };
    auto geometryAt = [&](size_t q) { return ptrp::Geometry{features_prev[q].normal, features_prev[q].depth}; };
    auto entryAt = [&](size_t q, unsigned long long* e) {
        for (int k = 0; k < 4; ++k) e[k] = film_prev[4 * q + k];
    };
    auto momentAt = [&](size_t q, unsigned long long* m) {
        m[0] = moments_prev[q].sumY, m[1] = moments_prev[q].sqLo, m[2] = moments_prev[q].sqHi, m[3] = moments_prev[q].samples;
    };
    for (int y = 0; y < now.height; ++y)
        for (int x = 0; x < now.width; ++x) {
            const size_t p = (size_t)y * (size_t)now.width + (size_t)x;
            const ptdn::Feature fp{features_now[p].normal, features_now[p].depth, features_now[p].materialIdx};
            auto pointOf = [&](vec3 o, vec3 d) -> vec3 { return motion_now ? vec3(motion_now[p].prevPoint) : madd(d, fp.depth, o); };
            ptlrp::Seed s;
            ptlrp::seedPixel<Moments>(x, y, fp, now, prev, R, splat, pointOf, materialAt, geometryAt, entryAt, momentAt, s);
            for (int k = 0; k < 4; ++k) film_out[4 * p + k] = s.film[k];
            if (Moments) moments_out[p] = ptss_linear_moment{s.moment[0], s.moment[1], s.moment[2], s.moment[3]};
            if (info) {
                info->seeded += s.status == ptlrp::kSeeded;
                info->offFilm += s.status == ptlrp::kOffFilm;
                info->noTap += s.status == ptlrp::kNoTap;
                info->noVariance += s.noVariance;
            }
        }
}
}   // extern "C++"

int ptss_probe_reproject_linear(const ptss_film_camera* now, const ptss_pixel_feature* features_now, const ptss_pixel_motion* motion_now,
                                const ptss_film_camera* prev, const ptss_pixel_feature* features_prev, const void* film_prev, int filmKind,
                                const ptss_linear_moment* moments_prev, const ptss_linear_params* film,
                                const ptss_reproject_linear_params* params, void* film_out, ptss_linear_moment* moments_out,
                                ptss_reproject_linear_info* info) {
    if (!now || !prev || !film || !params) return PTSS_HOST_EINVAL;
    if (ptlrp::paramsError(params) || ptlrp::cameraError(now) || ptlrp::cameraError(prev) || ptlin::paramsError(film)) return PTSS_HOST_EINVAL;
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return PTSS_HOST_EINVAL;
    if (ptlrp::buffersError(now, features_now, prev, features_prev, film_prev, moments_prev, film_out, moments_out)) return PTSS_HOST_EINVAL;
    const ptcam::Film F = ptlrp::nowOf(*now);
    const ptlrp::Prev P = ptlrp::prevOf(*prev);
    const ptlrp::Rule R = ptlrp::ruleOf(*params, *film);
    const bool splat = filmKind == PTSS_FILM_SPLAT;
    if (moments_prev)
        probeReprojectLinear<true>(F, features_now, motion_now, P, features_prev, static_cast<const unsigned long long*>(film_prev), splat, moments_prev,
                                   R, static_cast<unsigned long long*>(film_out), moments_out, info);
    else
        probeReprojectLinear<false>(F, features_now, motion_now, P, features_prev, static_cast<const unsigned long long*>(film_prev), splat, nullptr, R,
                                    static_cast<unsigned long long*>(film_out), nullptr, info);
    return PTSS_HOST_OK;
}

int ptss_probe_reproject_linear_finish(const float* h, float w, int hasVariance, float s2, int filmKind, const ptss_linear_params* film,
                                       const ptss_reproject_linear_params* params, unsigned long long* film4, unsigned long long* moment4) {
    if (!h || !film4 || !moment4 || ptlin::paramsError(film) || ptlrp::paramsError(params)) return PTSS_HOST_EINVAL;
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return PTSS_HOST_EINVAL;
    if (hasVariance && !(s2 >= 0.f && s2 <= ptlrp::kMaxVariance)) return PTSS_HOST_EINVAL;
    const ptlrp::Rule R = ptlrp::ruleOf(*params, *film);
    const float kf = ptlrp::historyCount(w, R.maxHistory);
    for (int k = 0; k < 4; ++k) film4[k] = moment4[k] = 0ull;
    if (!(kf >= 1.0f)) return PTSS_HOST_OK;
    unsigned long long m[3];
    ptlrp::filmRow(v3(h[0], h[1], h[2]), (unsigned long long)kf, filmKind == PTSS_FILM_SPLAT, R, m, film4);
    ptlrp::momentRow(m, (unsigned long long)kf, hasVariance != 0, s2, moment4);
    return PTSS_HOST_OK;
}

// ---- upsampling the two linear films (csrc/ptlinup.h) ----
int ptss_probe_upsample_linear(const void* film_lo, int filmKind, int width, int height, const ptss_pixel_feature* features_lo,
                               const ptss_pixel_feature* features_hi, const ptss_linear_params* film, const ptss_upsample_linear_params* params,
                               ptss_linear_entry* film_hi, ptss_upsample_linear_info* info) {
    if (!film_lo || !features_lo || !features_hi || !film || !params || !film_hi) return PTSS_HOST_EINVAL;
    if (ptlup::paramsError(params) || ptlin::paramsError(film)) return PTSS_HOST_EINVAL;
    if (filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT) return PTSS_HOST_EINVAL;
    if (ptlup::sidesError(width, height, params->factor)) return PTSS_HOST_ERANGE;
    const int f = params->factor, hiW = width * f, hiH = height * f;
    if (ptlup::rangesOverlap(film_hi, 32 * (size_t)hiW * (size_t)hiH, film_lo, 32 * (size_t)width * (size_t)height)) return PTSS_HOST_EINVAL;
    const ptlup::Rule R = ptlup::ruleOf(*params, *film);
    const bool splat = filmKind == PTSS_FILM_SPLAT;
    const unsigned long long* lo = static_cast<const unsigned long long*>(film_lo);
    unsigned long long* hi = reinterpret_cast<unsigned long long*>(film_hi);
    auto tapAt = [&](int, int, int cx, int cy, unsigned long long* e) {
        const size_t q = (size_t)cy * (size_t)width + (size_t)cx;
        for (int k = 0; k < 4; ++k) e[k] = lo[4 * q + k];
    };
    auto featureAt = [&](int, int, int cx, int cy) {
        const ptss_pixel_feature& g = features_lo[(size_t)cy * (size_t)width + (size_t)cx];
        return ptdn::Feature{g.normal, g.depth, g.materialIdx};
    };
    auto depthAt = [&](int x, int y) { return features_hi[(size_t)y * (size_t)hiW + (size_t)x].depth; };
    for (int Y = 0; Y < hiH; ++Y)
        for (int X = 0; X < hiW; ++X) {
            const size_t p = (size_t)Y * (size_t)hiW + (size_t)X;
            const ptdn::Feature fp{features_hi[p].normal, features_hi[p].depth, features_hi[p].materialIdx};
            const int status = ptlup::upsamplePixel<false>(X, Y, width, height, R, splat, fp, tapAt, featureAt, depthAt, hi + 4 * p);
            if (info) {
                info->filtered += status == ptlup::kFiltered;
                info->fallback += status == ptlup::kFallback;
                info->empty += status == ptlup::kEmpty;
            }
        }
    return PTSS_HOST_OK;
}

// ---- rays from surface points, the gutter fill, the atlas (csrc/ptsurface.h) ----
int ptss_probe_surface_rays(const ptss_triangle* triangles, size_t numTriangles, const ptss_sphere* spheres, size_t numSpheres,
                            const ptss_surface_params* params, const ptss_surface_point* points, size_t numPoints, size_t firstPoint,
                            const uint32_t* index, size_t n, ptss_path_rng* rng, ptss_ray_query* rays, ptss_ray_hit* surfels,
                            unsigned long long* rejected) {
    if (ptsurf::paramsError(params)) return PTSS_HOST_EINVAL;
    if (n >= (size_t(1) << 31) || numPoints >= (size_t(1) << 31)) return PTSS_HOST_ERANGE;
    if (rejected) *rejected = 0;
    if (n == 0) return PTSS_HOST_OK;
    if (!points || !rng || !rays || (numTriangles > 0 && !triangles) || (numSpheres > 0 && !spheres)) return PTSS_HOST_EINVAL;
    if (!index && (firstPoint > numPoints || n > numPoints - firstPoint)) return PTSS_HOST_ERANGE;
    unsigned long long dropped = 0;
    for (size_t i = 0; i < n; ++i) {
        const unsigned long long p = index ? index[i] : firstPoint + i;
        if (p >= numPoints) {
            ++dropped;
            continue;
        }
        const ptss_surface_point pt = points[p];
        const uint32_t prim = (uint32_t)pt.surface & ~ptsurf::kTriangleBit;
        const bool triangle = ((uint32_t)pt.surface & ptsurf::kTriangleBit) != 0u;
        bool ok = pt.surface >= 0 && ptsurf::flagsAccepted(pt.flags);
        ok = ok && (triangle ? prim < numTriangles && ptsurf::triangleAccepted(pt.a, pt.b) : prim < numSpheres && ptsurf::sphereAccepted(pt.a, pt.b));
        if (!ok) {
            ++dropped;
            continue;
        }
        ptsurf::Surfel s;
        int materialIdx;
        if (triangle) {
            const ptss_triangle& t = triangles[prim];
            s = ptsurf::triangleSurfel(t.vertex0, t.vertex1 - t.vertex0, t.vertex2 - t.vertex0, t.normal0, t.normal1, t.normal2, pt.a, pt.b, pt.flags);
            materialIdx = t.materialIdx;
        } else {
            const ptss_sphere& sp = spheres[prim];
            s = ptsurf::sphereSurfel(sp.position, sp.radius * sp.radius, pt.a, pt.b, pt.flags);
            materialIdx = sp.materialIdx;
        }
        float u1 = 0.0f, u2 = 0.0f;
        if (ptsurf::draws(params->mode)) {
            ptrng::State st;
            for (int w = 0; w < 5; ++w) st.v[w] = rng[i].v[w];
            st.d = rng[i].d;
            u1 = ptrng::uniform(st);
            u2 = ptrng::uniform(st);
            for (int w = 0; w < 5; ++w) rng[i].v[w] = st.v[w];
            rng[i].d = st.d;
        }
        rays[i] = ptsurf::surfaceRay(s, params->mode, params->maxDistance, u1, u2);
        if (surfels) surfels[i] = ptsurf::surfelHit(s, materialIdx, triangle ? PTSS_HIT_TRIANGLE : PTSS_HIT_SPHERE, (int)prim, pt.a, pt.b);
    }
    if (rejected) *rejected = dropped;
    return PTSS_HOST_OK;
}

int ptss_probe_dilate_linear(const ptss_linear_entry* film, int width, int height, ptss_linear_entry* out) {
    if (!film || !out || film == out) return PTSS_HOST_EINVAL;
    if (ptsurf::dilateSidesError(width, height)) return PTSS_HOST_ERANGE;
    auto at = [&](int x, int y) {
        const ptss_linear_entry& e = film[(size_t)y * (size_t)width + (size_t)x];
        return ptsurf::Texel{e.r, e.g, e.b, e.samples, e.clamped};
    };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const ptsurf::Texel t = ptsurf::dilateTexel(x, y, width, height, at);
            out[(size_t)y * (size_t)width + (size_t)x] = ptss_linear_entry{t.r, t.g, t.b, t.samples, t.clamped};
        }
    return PTSS_HOST_OK;
}

int ptss_surface_atlas(const ptss_triangle* triangles, size_t first, size_t count, float texelsPerUnit, int minSide, int maxSide, int atlasWidth,
                       ptss_surface_point* points, uint32_t* texels, size_t capacity, int* atlasHeight, size_t* numPoints) {
    static_assert(PTSS_HOST_EINVAL == -1 && PTSS_HOST_ERANGE == -3, "ptsurf::atlas returns these");
    return ptsurf::atlas(triangles, first, count, texelsPerUnit, minSide, maxSide, atlasWidth, points, texels, capacity, atlasHeight, numPoints);
}

// ---- light maps read back: the blocks of the atlas, the lookup (csrc/ptsurface.h, csrc/ptlightmap.h) ----
int ptss_surface_atlas_blocks(const ptss_triangle* triangles, size_t firstTriangle, size_t numTriangles, const ptss_sphere* spheres,
                              size_t firstSphere, size_t numSpheres, float texelsPerUnit, int minSide, int maxSide, int atlasWidth,
                              ptss_surface_block* blocksTri, ptss_surface_block* blocksSph, ptss_surface_point* points, uint32_t* texels,
                              size_t capacity, int* atlasHeight, size_t* numPoints) {
    return ptsurf::atlasBlocks(triangles, firstTriangle, numTriangles, spheres, firstSphere, numSpheres, texelsPerUnit, minSide, maxSide, atlasWidth,
                               blocksTri, blocksSph, points, texels, capacity, atlasHeight, numPoints);
}

// chain == nullptr: the plain lookup; else ptlightmap.h's step 6 with chain[i].throughput (the caller has refused a null chain with n > 0)
static int lookupLightmapProbe(const ptss_material* materials, size_t numMaterials, const ptss_lightmap_params* params,
                               const ptss_linear_params* film, const ptss_surface_block* blocksTri, const ptss_surface_block* blocksSph,
                               const ptss_linear_entry* map, const ptss_ray_hit* hits, const ptss_chain_result* chain, size_t n,
                               ptss_linear_entry* out, uint32_t* info) {
    if (ptlm::paramsError(params) || ptlin::paramsError(film)) return PTSS_HOST_EINVAL;
    if (ptlm::rangeError(params) || n >= (size_t(1) << 31) || numMaterials >= (size_t(1) << 31)) return PTSS_HOST_ERANGE;
    if (n == 0) return PTSS_HOST_OK;
    if (!map || !hits || !out || (params->numTriangleBlocks > 0 && !blocksTri) || (params->numSphereBlocks > 0 && !blocksSph) ||
        (numMaterials > 0 && !materials))
        return PTSS_HOST_EINVAL;
    if (ptlrp::rangesOverlap(out, 32 * n, map, 32 * (size_t)params->atlasWidth * (size_t)params->atlasHeight)) return PTSS_HOST_EINVAL;
    const ptlm::Rule R = ptlm::ruleOf(*params, *film, (int)numMaterials);
    auto block = [](const ptss_surface_block* table, int row) { return ptlm::Block{table[row].x, table[row].y, table[row].width, table[row].height}; };
    auto at = [&](uint32_t texel) { return ptlm::Texel{map[texel].r, map[texel].g, map[texel].b, map[texel].samples}; };
    auto material = [&](int idx, int row) { return row == 0 ? materials[idx].diffuseColor : materials[idx].emmitance; };
    for (size_t i = 0; i < n; ++i) {
        const ptss_ray_hit& g = hits[i];
        const ptlm::Hit h{g.normal, g.materialIdx, g.kind, g.primitive, g.w1, g.w2};
        ptlm::u64 m[3];
        const int verdict = ptlm::lookup(
            h, R, [&](int row) { return block(blocksTri, row); }, [&](int row) { return block(blocksSph, row); }, at, material, m);
        if (chain && verdict == ptlm::kFiltered) {
            m[0] = ptlm::tint(m[0], chain[i].throughput.x);
            m[1] = ptlm::tint(m[1], chain[i].throughput.y);
            m[2] = ptlm::tint(m[2], chain[i].throughput.z);
        }
        out[i] = ptss_linear_entry{m[0], m[1], m[2], verdict == ptlm::kFiltered ? 1u : 0u, 0u};
        if (info) ++info[verdict];
    }
    return PTSS_HOST_OK;
}

int ptss_probe_lookup_lightmap(const ptss_material* materials, size_t numMaterials, const ptss_lightmap_params* params,
                               const ptss_linear_params* film, const ptss_surface_block* blocksTri, const ptss_surface_block* blocksSph,
                               const ptss_linear_entry* map, const ptss_ray_hit* hits, size_t n, ptss_linear_entry* out, uint32_t* info) {
    return lookupLightmapProbe(materials, numMaterials, params, film, blocksTri, blocksSph, map, hits, nullptr, n, out, info);
}

int ptss_probe_lookup_lightmap_chain(const ptss_material* materials, size_t numMaterials, const ptss_lightmap_params* params,
                                     const ptss_linear_params* film, const ptss_surface_block* blocksTri, const ptss_surface_block* blocksSph,
                                     const ptss_linear_entry* map, const ptss_ray_hit* hits, const ptss_chain_result* chain, size_t n,
                                     ptss_linear_entry* out, uint32_t* info) {
    if (ptlm::paramsError(params) || ptlin::paramsError(film)) return PTSS_HOST_EINVAL;
    if (ptlm::rangeError(params) || n >= (size_t(1) << 31) || numMaterials >= (size_t(1) << 31)) return PTSS_HOST_ERANGE;
    if (n == 0) return PTSS_HOST_OK;
    if (!chain || !out || !hits) return PTSS_HOST_EINVAL;
    if (ptlrp::rangesOverlap(out, 32 * n, chain, 32 * n) || ptlrp::rangesOverlap(out, 32 * n, hits, 48 * n)) return PTSS_HOST_EINVAL;
    return lookupLightmapProbe(materials, numMaterials, params, film, blocksTri, blocksSph, map, hits, chain, n, out, info);
}

}  // extern "C"
