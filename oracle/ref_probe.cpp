// ref_probe.cpp — driver of the reference's OWN code compiled for the CPU (TEST INFRASTRUCTURE; oracle/build.py build_ref).
//
// This file holds no line of the reference. It #includes the reference's CudaTracer.cu and Scene.cpp, found through -I: the
// reference directory for Scene.cpp and the headers, oracle/_ref/ for the copy of CudaTracer.cu in which build_ref() has turned
// every kernel<<<grid, block>>>(args) into REF_LAUNCH(kernel, grid, block, args) (the one thing g++ cannot parse). CUDA, cuRAND,
// Thrust, glm and the window libraries are the stand-ins under oracle/ref_shim/. What comes out is oracle/_ref/libref_probe.so:
// one extern "C" probe per reference function, the reference's scene builders, and its generateFrame loop, for
// tests/test_reference_*.py and tests/golden/make_reference_golden.py. Neither the library nor anything derived from the
// reference's text is committed.
//
// Every probe is batched: n cases per call, float32 arrays, records in the layouts of include/ptss_types.h (asserted below to be
// the reference's). oracle/oracle.cpp exports the same probes as oracle_fn_* over the oracle's functions.
#include <cstdint>
#include <cstring>
#include <vector>

#include <omp.h>

#define main ref_reference_main   // CudaTracer.cu:649 — its main() opens a window; the driver below does main's set-up itself
#include "CudaTracer.cu"
#undef main
#include "Scene.cpp"

unsigned int ref_rand_state = 1u;   // msvc_rand.h

static_assert(sizeof(vec3) == 12 && sizeof(quat) == 16, "glm stand-in: packed floats");
static_assert(sizeof(Sphere) == 20 && sizeof(Triangle) == 76 && sizeof(Material) == 76 && offsetof(Material, flags) == 72, "ptss_types.h");
static_assert(sizeof(PointLight) == 24 && sizeof(AreaLight) == 32 && sizeof(Camera) == 40 && sizeof(curandState) == 24, "ptss_types.h");

namespace {

struct Held {   // the scene the probes run against: the reference's five vectors and a RendererData that points into them
    std::vector<Sphere> spheres;
    std::vector<Triangle> triangles;
    std::vector<Material> materials;
    std::vector<PointLight> pointLights;
    std::vector<AreaLight> areaLights;
    RendererData data;
    void bind() {
        memset(&data, 0, sizeof(data));
        data.defaultColor = vec3(0, 0, 0);   // CudaTracer.cu:653
        data.spheres = spheres.data();
        data.numSpheres = spheres.size();
        data.triangles = triangles.data();
        data.numTriangles = triangles.size();
        data.materials = materials.data();
        data.pointLights = pointLights.data();
        data.numPointLights = pointLights.size();
        data.areaLights = areaLights.data();
        data.numAreaLights = areaLights.size();
    }
} held;

inline vec3 ld3(const float* p) { return vec3(p[0], p[1], p[2]); }
inline void st3(float* p, const vec3& v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
inline void stState(uint32_t* p, const curandState& s) {
    for (int i = 0; i < 5; ++i) p[i] = s.v[i];
    p[5] = s.d;
}
inline Ray rayOf(const float* r6) { return Ray(ld3(r6), ld3(r6 + 3)); }
inline void stHit(float* out8, float d, const SurfaceElement& se) {
    out8[0] = d;
    st3(out8 + 1, se.point);
    st3(out8 + 4, se.normal);
    out8[7] = (float)se.materialIdx;
}
inline SurfaceElement zeroSurfel() { return SurfaceElement(vec3(0, 0, 0), vec3(0, 0, 0), 0); }

struct Frames {
    ProgramData* data = nullptr;
    std::vector<uchar4> pixels;
    std::vector<long> counts;   // rays launched per bounce of the last frame
};

}  // namespace

extern "C" {

// ---- scenes -------------------------------------------------------------------------------------------
// kind 0: Scene::build() as committed (Scene.cpp:17-32); kind 1: addDefinedSpheres(4) then addCornellBox(8), the scene of the
// reference's image.tga (the host mirror's "cornell"). The C runtime's rand() starts from its unseeded state each time.
// Material::roughness is left unset by every constructor (RenderStructs.h:95-105); the frame loop reads it wherever flags & 0x03
// is non-zero (CudaTracer.cu:258-261), which includes the PURE_REFLECTION mirror. So that runs repeat, the driver sets it to 0 in
// every material that does not carry the whole COOK_TORRANCE value — the materials whose roughness the reference's scene code
// never assigns — the same choice as the oracle's ("Deviations").
int ref_build_scene(int kind) {
    ref_rand_state = 1u;
    Scene scene;
    if (kind == 0) {
        scene.build();
    } else if (kind == 1) {
        scene.addDefinedSpheres(4);
        scene.addCornellBox(8);
    } else {
        return -1;
    }
    for (Material& m : scene.materialsVec)
        if ((m.flags & MAT_FLAG_COOK_TORRANCE) != MAT_FLAG_COOK_TORRANCE) m.roughness = 0.0f;
    held.spheres = scene.spheresVec;
    held.triangles = scene.trianglesVec;
    held.materials = scene.materialsVec;
    held.pointLights = scene.pointLightsVec;
    held.areaLights = scene.areaLightsVec;
    held.bind();
    return 0;
}
// any scene, as records of include/ptss_types.h
void ref_set_scene(const void* spheres, size_t numSpheres, const void* triangles, size_t numTriangles, const void* materials,
                   size_t numMaterials, const void* pointLights, size_t numPointLights, const void* areaLights, size_t numAreaLights) {
    held.spheres.assign((const Sphere*)spheres, (const Sphere*)spheres + numSpheres);
    held.triangles.assign((const Triangle*)triangles, (const Triangle*)triangles + numTriangles);
    held.materials.assign((const Material*)materials, (const Material*)materials + numMaterials);
    held.pointLights.assign((const PointLight*)pointLights, (const PointLight*)pointLights + numPointLights);
    held.areaLights.assign((const AreaLight*)areaLights, (const AreaLight*)areaLights + numAreaLights);
    held.bind();
}
void ref_scene_counts(size_t* out5) {
    out5[0] = held.spheres.size();
    out5[1] = held.triangles.size();
    out5[2] = held.materials.size();
    out5[3] = held.pointLights.size();
    out5[4] = held.areaLights.size();
}
void ref_scene_copy(void* spheres, void* triangles, void* materials, void* pointLights, void* areaLights) {
    if (!held.spheres.empty()) memcpy(spheres, held.spheres.data(), sizeof(Sphere) * held.spheres.size());
    if (!held.triangles.empty()) memcpy(triangles, held.triangles.data(), sizeof(Triangle) * held.triangles.size());
    if (!held.materials.empty()) memcpy(materials, held.materials.data(), sizeof(Material) * held.materials.size());
    if (!held.pointLights.empty()) memcpy(pointLights, held.pointLights.data(), sizeof(PointLight) * held.pointLights.size());
    if (!held.areaLights.empty()) memcpy(areaLights, held.areaLights.data(), sizeof(AreaLight) * held.areaLights.size());
}

// ---- Primitives.h ---------------------------------------------------------------------------------------
// sph4 = centre, radius; ray6 = origin, direction; out8 = distance, point, normal, materialIdx (surfel zeroed before the call)
void ref_sphere(int n, const float* sph4, const float* ray6, const float* tmax, int updateSurfel, int* hit, float* out8) {
    for (int i = 0; i < n; ++i) {
        const Sphere sp(ld3(sph4 + 4 * i), sph4[4 * i + 3], 7);
        SurfaceElement se = zeroSurfel();
        float d = tmax[i];
        hit[i] = sp.intersectRay(rayOf(ray6 + 6 * i), d, se, updateSurfel != 0) ? 1 : 0;
        stHit(out8 + 8 * i, d, se);
    }
}
// tri18 = vertex0..2, normal0..2
void ref_triangle(int n, const float* tri18, const float* ray6, const float* tmax, int updateSurfel, int* hit, float* out8) {
    for (int i = 0; i < n; ++i) {
        const float* t = tri18 + 18 * i;
        const Triangle tri(ld3(t), ld3(t + 3), ld3(t + 6), ld3(t + 9), ld3(t + 12), ld3(t + 15), 3);
        SurfaceElement se = zeroSurfel();
        float d = tmax[i];
        hit[i] = tri.intersectRay(rayOf(ray6 + 6 * i), d, se, updateSurfel != 0) ? 1 : 0;
        stHit(out8 + 8 * i, d, se);
    }
}
// the two intersection loops of pathTraceKernel (CudaTracer.cu:121-141) over the held scene, with `distance` starting at tmax.
// kind 0 miss / 1 sphere / 2 triangle and prim = the index of the last primitive that accepted.
void ref_closest_hit(int n, const float* ray6, const float* tmax, int* kind, int* prim, float* out8) {
    for (int i = 0; i < n; ++i) {
        const Ray ray = rayOf(ray6 + 6 * i);
        float d = tmax[i];
        SurfaceElement se = zeroSurfel();
        kind[i] = 0;
        prim[i] = -1;
        for (size_t k = 0; k < held.data.numSpheres; ++k)
            if (held.data.spheres[k].intersectRay(ray, d, se)) { kind[i] = 1; prim[i] = (int)k; }
        for (size_t k = 0; k < held.data.numTriangles; ++k)
            if (held.data.triangles[k].intersectRay(ray, d, se)) { kind[i] = 2; prim[i] = (int)k; }
        if (!kind[i]) se.materialIdx = -1;
        stHit(out8 + 8 * i, d, se);
    }
}

// the two loops of lineOfSight (CudaTracer.cu:438-452) on a ray given as such: 1 where some primitive accepts within tmax
void ref_any_hit(int n, const float* ray6, const float* tmax, int* blocked) {
    for (int i = 0; i < n; ++i) {
        const Ray ray = rayOf(ray6 + 6 * i);
        float d = tmax[i];
        SurfaceElement se = zeroSurfel();
        blocked[i] = 0;
        for (size_t k = 0; k < held.data.numSpheres && !blocked[i]; ++k)
            if (held.data.spheres[k].intersectRay(ray, d, se, false)) blocked[i] = 1;
        for (size_t k = 0; k < held.data.numTriangles && !blocked[i]; ++k)
            if (held.data.triangles[k].intersectRay(ray, d, se, false)) blocked[i] = 1;
    }
}

// ---- CudaTracer.cu, function by function ---------------------------------------------------------------------
// out4 = w_i, distance2
void ref_line_of_sight(int n, const float* normal, const float* p0, const float* p1, int* visible, float* out4) {
    for (int i = 0; i < n; ++i) {
        vec3 w_i(0, 0, 0);
        float d2 = 0;
        visible[i] = lineOfSight(held.data, ld3(normal + 3 * i), ld3(p0 + 3 * i), ld3(p1 + 3 * i), w_i, d2) ? 1 : 0;
        st3(out4 + 4 * i, w_i);
        out4[4 * i + 3] = d2;
    }
}
// out6 = cosI after the call, sinT2, n1, n2, n, Fresnel reflectance
void ref_fresnel(int n, const float* refrIndex, const float* cosIin, float* out6) {
    for (int i = 0; i < n; ++i) {
        float cosI = cosIin[i], sinT2, n1, n2, nn;
        computeSinT2AndRefractiveIndexes(refrIndex[i], cosI, sinT2, n1, n2, nn);
        float* o = out6 + 6 * i;
        o[0] = cosI; o[1] = sinT2; o[2] = n1; o[3] = n2; o[4] = nn;
        o[5] = computeFresnelForReflectance(cosI, sinT2, n1, n2, nn);
    }
}
// out6 = origin, direction of the ray afterwards
void ref_refl_surfel(int n, const float* dir, const float* point, const float* normal, const float* cosI, float* out6) {
    for (int i = 0; i < n; ++i) {
        Ray ray(vec3(0, 0, 0), ld3(dir + 3 * i));
        reflRay(ray, SurfaceElement(ld3(point + 3 * i), ld3(normal + 3 * i), 0), cosI[i]);
        st3(out6 + 6 * i, ray.origin);
        st3(out6 + 6 * i + 3, ray.direction);
    }
}
void ref_refl_normal(int n, const float* dir, const float* point, const float* normal, float* out6) {
    for (int i = 0; i < n; ++i) {
        Ray ray(vec3(0, 0, 0), ld3(dir + 3 * i));
        reflRay(ray, ld3(point + 3 * i), ld3(normal + 3 * i));
        st3(out6 + 6 * i, ray.origin);
        st3(out6 + 6 * i + 3, ray.direction);
    }
}
void ref_refr(int n, const float* dir, const float* point, const float* normal, const float* cosI, const float* sinT2, const float* nn,
              int* active, float* out6) {
    for (int i = 0; i < n; ++i) {
        Ray ray(vec3(0, 0, 0), ld3(dir + 3 * i));
        refrRay(ray, SurfaceElement(ld3(point + 3 * i), ld3(normal + 3 * i), 0), cosI[i], sinT2[i], nn[i]);
        active[i] = ray.active ? 1 : 0;
        st3(out6 + 6 * i, ray.origin);
        st3(out6 + 6 * i + 3, ray.direction);
    }
}
// out4 = x, y, z, w
void ref_rotate_v2v(int n, const float* source, const float* target, float* out4) {
    for (int i = 0; i < n; ++i) {
        const quat q = rotateVectorToVector(ld3(source + 3 * i), ld3(target + 3 * i));
        out4[4 * i] = q.x; out4[4 * i + 1] = q.y; out4[4 * i + 2] = q.z; out4[4 * i + 3] = q.w;
    }
}
// kind 0 Lambert(axis), 1 Phong(axis, param = exponent), 2 Beckmann(axis, param = roughness); case i draws from
// curand_init(seed, i, 0); state6 = v[0..4], d afterwards
void ref_sampler(int kind, int n, const float* axis, const float* param, unsigned long long seed, float* out3, uint32_t* state6) {
    for (int i = 0; i < n; ++i) {
        curandState st;
        curand_init(seed, (unsigned long long)i, 0, &st);
        const vec3 a = ld3(axis + 3 * i);
        const vec3 d = kind == 0 ? randomDirectionLambert(a, st) : kind == 1 ? randomDirectionPhong(a, param[i], st) : randomDirectionBeckmann(a, param[i], st);
        st3(out3 + 3 * i, d);
        stState(state6 + 6 * i, st);
    }
}
void ref_area_light_point(int n, const int* light, unsigned long long seed, float* out3, uint32_t* state6) {
    for (int i = 0; i < n; ++i) {
        curandState st;
        curand_init(seed, (unsigned long long)i, 0, &st);
        st3(out3 + 3 * i, getAreaLightPoint(held.data.areaLights[light[i]], held.data.triangles, st));
        stState(state6 + 6 * i, st);
    }
}
void ref_shade(int n, const float* point, const float* normal, const int* materialIdx, unsigned long long seed, float* out3, uint32_t* state6) {
    for (int i = 0; i < n; ++i) {
        curandState st;
        curand_init(seed, (unsigned long long)i, 0, &st);
        const SurfaceElement se(ld3(point + 3 * i), ld3(normal + 3 * i), materialIdx[i]);
        st3(out3 + 3 * i, shade(held.data, se, held.data.materials[materialIdx[i]], st));
        stState(state6 + 6 * i, st);
    }
}
// cam10 = rotation x, y, z, w; position; zNear, zFar, fieldOfView (ptss_camera). The state of pixel (x, y): sequence y * DIM + x.
void ref_eye_ray(int n, const int* x, const int* y, const float* cam10, unsigned long long seed, float* out6, uint32_t* state6) {
    Camera cam;
    memcpy(&cam, cam10, sizeof(cam));
    for (int i = 0; i < n; ++i) {
        curandState st;
        curand_init(seed, (unsigned long long)(y[i] * DIM + x[i]), 0, &st);
        const Ray r = computeEyeRay(x[i], y[i], cam, st);
        st3(out6 + 6 * i, r.origin);
        st3(out6 + 6 * i + 3, r.direction);
        stState(state6 + 6 * i, st);
    }
}
// materials: n records of ptss_material. out9 = origin, direction of the ray afterwards, the returned colour.
void ref_scatter(int n, const float* dir, const float* point, const float* normal, const void* materials, const float* cosI,
                 const float* distance, unsigned long long seed, int* active, float* out9, uint32_t* state6) {
    for (int i = 0; i < n; ++i) {
        curandState st;
        curand_init(seed, (unsigned long long)i, 0, &st);
        Material m;
        memcpy(&m, (const char*)materials + sizeof(Material) * i, sizeof(Material));
        Ray ray(vec3(0, 0, 0), ld3(dir + 3 * i));
        const SurfaceElement se(ld3(point + 3 * i), ld3(normal + 3 * i), 0);
        const vec3 c = computeIndirectRadianceAndScatter(ray, se, m, cosI[i], distance[i], cosI[i] <= 0.0f, st);
        active[i] = ray.active ? 1 : 0;
        st3(out9 + 9 * i, ray.origin);
        st3(out9 + 9 * i + 3, ray.direction);
        st3(out9 + 9 * i + 6, c);
        stState(state6 + 6 * i, st);
    }
}
// writeToPixelsKernel itself (CudaTracer.cu:63-104) with ticks = 0 on zeroed totals: the totals afterwards are the 8-bit samples.
void ref_tonemap(int n, const float* radiance, uint32_t* out) {
    const int perBlock = 256, channels = 3;
    const int rays = (n + channels - 1) / channels;
    const int blocks = (rays + perBlock - 1) / perBlock;
    std::vector<Ray> r((size_t)blocks * perBlock, Ray(vec3(0, 0, 0), vec3(0, 0, 1)));
    std::vector<uint3> totals(r.size(), uint3{0, 0, 0});
    std::vector<uchar4> pixels(r.size());
    for (size_t k = 0; k < r.size(); ++k) {
        r[k].pixelOffset = (int)k;
        float c[3] = {0, 0, 0};
        for (int ch = 0; ch < channels; ++ch)
            if ((long)k * channels + ch < n) c[ch] = radiance[k * channels + ch];
        r[k].radiance0 = vec3(c[0], c[1], c[2]);
    }
    REF_LAUNCH(writeToPixelsKernel, dim3(blocks, 1), dim3(16, 16), pixels.data(), totals.data(), r.data(), 0);
    for (int i = 0; i < n; ++i) {
        const uint3& t = totals[i / channels];
        out[i] = i % channels == 0 ? t.x : (i % channels == 1 ? t.y : t.z);
    }
}
int ref_move_camera(float* cam10, int key) {
    Camera cam;
    memcpy(&cam, cam10, sizeof(cam));
    const bool moved = moveCamera(cam, (unsigned char)key);
    memcpy(cam10, &cam, sizeof(cam));
    return moved ? 1 : 0;
}
void ref_default_camera(float* cam10) {
    const Camera cam;
    memcpy(cam10, &cam, sizeof(cam));
}
// curand_init(seed, sequence, 0) of the stand-in, then n draws: state6 at the start, raw draws, uniforms (oracle.probe_rng's contract)
void ref_rng(unsigned long long seed, unsigned sequence, int n, uint32_t* state6, uint32_t* raw, float* uni) {
    curandState st;
    curand_init(seed, sequence, 0, &st);
    stState(state6, st);
    for (int i = 0; i < n; ++i) {
        curandState b = st;
        raw[i] = curand(&st);
        uni[i] = curand_uniform(&b);
    }
}

// ---- whole frames: main()'s set-up (CudaTracer.cu:666-724) over the held scene, then the reference's generateFrame -----------
void* ref_frames_create(unsigned int seed, int usePathTracer) {
    Frames* f = new Frames();
    ProgramData* data = new ProgramData();
    const size_t n = (size_t)DIM * DIM;
    Ray* rays;
    curandState* states;
    uint3* totals;
    cudaMalloc((void**)&rays, sizeof(Ray) * n);
    cudaMalloc(&states, sizeof(curandState) * n);
    cudaMalloc((void**)&totals, sizeof(uint3) * n);
    data->camera = Camera();
    data->renderData = held.data;
    data->renderData.rays = rays;
    data->renderData.curandStates = states;
    data->totalPixelColors = totals;
    data->resetTicksThisFrame = true;
    data->usePathTracer = usePathTracer != 0;
    cudaEventCreate(&data->start);
    cudaEventCreate(&data->stop);
    (void)ref_xorwow::jumps();
    ref_clock_seed = seed;
    REF_LAUNCH(curandSetupKernel, dim3(DIM / 16, DIM / 16), dim3(16, 16), states);
    f->data = data;
    f->pixels.resize(n);
    return f;
}
void ref_frames_destroy(void* h) {
    Frames* f = (Frames*)h;
    cudaFree(f->data->renderData.rays);
    cudaFree(f->data->renderData.curandStates);
    cudaFree(f->data->totalPixelColors);
    cudaEventDestroy(f->data->start);
    cudaEventDestroy(f->data->stop);
    delete f->data;
    delete f;
}
void ref_frames_step(void* h, int ticks) {
    Frames* f = (Frames*)h;
    ref_partition_log.clear();
    std::cout.setstate(std::ios_base::failbit);   // generateFrame prints a status line per frame
    generateFrame(f->pixels.data(), f->data, ticks);
    std::cout.clear();
    // rays launched per bounce, from what the loop of CudaTracer.cu:622-633 did: bounce 0 starts from DIM * DIM rays, bounce i + 1
    // from the actives that partition i counted; each launches numRays / 96 blocks of 96 (:623) while numRays > 128 (:622)
    const unsigned numIterations = f->data->usePathTracer ? f->data->maxIterations : 1;
    f->counts.assign(numIterations, 0);
    long numRays = (long)DIM * DIM;
    for (unsigned i = 0; i < numIterations && numRays > 128; ++i) {
        f->counts[i] = (numRays / 96) * 96;
        if (i != numIterations - 1) {
            if (2 * i + 1 >= ref_partition_log.size() || ref_partition_log[2 * i] != numRays) { f->counts.assign(numIterations, -1); break; }
            numRays = ref_partition_log[2 * i + 1];
        }
    }
}
void ref_frames_totals(void* h, uint32_t* out) { memcpy(out, ((Frames*)h)->data->totalPixelColors, sizeof(uint3) * DIM * DIM); }
void ref_frames_pixels(void* h, unsigned char* out) { memcpy(out, ((Frames*)h)->pixels.data(), 4 * (size_t)DIM * DIM); }
int ref_frames_counts(void* h, long* out, int cap) {
    Frames* f = (Frames*)h;
    const int n = (int)f->counts.size();
    for (int i = 0; i < n && i < cap; ++i) out[i] = f->counts[i];
    return n;
}
// the live rays entering each bounce (before the division by 96), for the bound on the skipped rays
int ref_frames_live(void* h, long* out, int cap) {
    int n = 0;
    if (cap > 0) out[n++] = (long)DIM * DIM;
    for (size_t k = 1; k < ref_partition_log.size() && n < cap; k += 2) out[n++] = ref_partition_log[k];
    (void)h;
    return n;
}
void ref_frames_set_mode(void* h, int usePathTracer) {   // what the space bar does (CudaTracer.cu:763-764)
    Frames* f = (Frames*)h;
    f->data->usePathTracer = usePathTracer != 0;
    f->data->resetTicksThisFrame = true;
}
void ref_frames_set_max_iterations(void* h, unsigned maxIterations) { ((Frames*)h)->data->maxIterations = maxIterations; }
void ref_set_threads(int n) {
    if (n > 0) omp_set_num_threads(n);
}
int ref_dim(void) { return DIM; }

}  // extern "C"
