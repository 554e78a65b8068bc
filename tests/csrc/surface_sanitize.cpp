// surface_sanitize.cpp — a stand-alone host program over the probes of the surface rays, the gutter fill and the atlas
// (ptss_probe_surface_rays, ptss_probe_dilate_linear, ptss_surface_atlas: the host build of csrc/ptsurface.h), meant to
// be compiled with -fsanitize=address,undefined together with host/*.cpp and run on the CPU (tests/test_surface_cpu.py does). Every
// buffer is a heap block of exactly the size the call may touch — the triangles and spheres as many records as the counts say, the
// points numPoints rows of 16 B, the streams n records of 24 B, the rays n rows of 32 B, the surfels n rows of 48 B, the films
// width * height entries of 32 B, the atlas outputs `capacity` entries — so a gather through a bad primitive number, a bad index, a
// neighbour outside a film or a texel beyond the capacity is an error. The points hold one of every kind the call rejects.
// Prints "surface_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                             \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "surface_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

template <class T>
static T* block(size_t n) {
    return (T*)malloc(n ? n * sizeof(T) : 1);
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    size_t calls = 0;
    // ---- the rays ----
    const size_t T = 5, S = 3;
    ptss_triangle* tri = block<ptss_triangle>(T);
    ptss_sphere* sph = block<ptss_sphere>(S);
    for (size_t t = 0; t < T; ++t) {
        const float k = (float)t;
        tri[t] = ptss_triangle{{k, 0.f, -k}, {k + 1.f, 0.25f, -k}, {k, 1.f, -k - 1.f}, {0.f, 1.f, 0.f}, {0.f, t % 2 ? -1.f : 1.f, 0.f}, {0.f, 1.f, 0.f}, (int)t};
    }
    tri[4].normal0 = tri[4].normal1 = tri[4].normal2 = ptss_vec3{0.f, -1.f, -0.f};   // a ceiling
    for (size_t k = 0; k < S; ++k) sph[k] = ptss_sphere{{(float)k, 1.f, -2.f}, 0.5f + (float)k, (int)k};
    const int TRI = 0x40000000;
    const ptss_surface_point pts[] = {
        {TRI | 0, 0.25f, 0.25f, 0u}, {TRI | 4, 0.f, 0.f, 1u},   {TRI | 3, 1.f, 0.f, 0u},     {TRI | 2, 0.f, 1.f, 1u},    {0, 0.f, 0.f, 0u},
        {2, 1.f, 1.f, 1u},           {1, 0.5f, 0.5f, 0u},       {-1, 0.2f, 0.2f, 0u},        {TRI | 5, 0.2f, 0.2f, 0u},  {TRI | 0x3fffffff, 0.2f, 0.2f, 0u},
        {3, 0.2f, 0.2f, 0u},         {0x3fffffff, 0.2f, 0.2f, 0u}, {(int)0x80000000u, 0.2f, 0.2f, 0u}, {(int)0xc0000001u, 0.2f, 0.2f, 0u}, {TRI | 1, 0.2f, 0.2f, 2u},
        {TRI | 1, 0.2f, 0.2f, 0xfffffffeu}, {TRI | 1, -0.1f, 0.2f, 0u}, {TRI | 1, 0.2f, -0.1f, 0u}, {TRI | 1, 0.7f, 0.7f, 0u}, {TRI | 1, nan, 0.2f, 0u},
        {TRI | 1, 0.2f, inf, 0u},    {1, -0.1f, 0.5f, 0u},      {1, 0.5f, 1.5f, 0u},         {1, nan, nan, 0u}};
    const size_t P = sizeof(pts) / sizeof(pts[0]), good = 7;
    ptss_surface_point* points = block<ptss_surface_point>(P);
    memcpy(points, pts, sizeof(pts));
    for (int mode = 0; mode < 2; ++mode)
        for (int withIndex = 0; withIndex < 2; ++withIndex)
            for (int withSurfels = 0; withSurfels < 2; ++withSurfels) {
                const size_t n = withIndex ? P + 4 : P;
                const ptss_surface_params params = {(unsigned int)sizeof(ptss_surface_params), mode, mode ? inf : 3.f, 0u};
                uint32_t* index = withIndex ? block<uint32_t>(n) : nullptr;
                if (index) {
                    for (size_t i = 0; i < P; ++i) index[i] = (uint32_t)((i * 7) % P);   // a permutation (7 and 24 are coprime)
                    index[P] = (uint32_t)P, index[P + 1] = 0x80000000u, index[P + 2] = 0xffffffffu, index[P + 3] = 0u;   // three beyond, one duplicate
                }
                ptss_path_rng* rng = block<ptss_path_rng>(n);
                ptss_ray_query* rays = block<ptss_ray_query>(n);
                ptss_ray_hit* surfels = withSurfels ? block<ptss_ray_hit>(n) : nullptr;
                for (size_t i = 0; i < n; ++i) rng[i] = ptss_path_rng{{(uint32_t)(i + 1), 362436069u, 521288629u, 88675123u, 5783321u}, 6615241u + (uint32_t)i};
                memset(rays, 0xab, n * sizeof(ptss_ray_query));
                unsigned long long rejected = 77;
                EXPECT(ptss_probe_surface_rays(tri, T, sph, S, &params, points, P, 0, index, n, rng, rays, surfels, &rejected) == 0);
                EXPECT(rejected == (unsigned long long)(P - good + (withIndex ? 3 : 0)));
                ++calls;
                size_t written = 0;
                for (size_t i = 0; i < n; ++i) {
                    uint32_t first;
                    memcpy(&first, &rays[i].pad, 4);
                    if (first == 0xababababu) continue;
                    ++written;
                    const float len = rays[i].direction.x * rays[i].direction.x + rays[i].direction.y * rays[i].direction.y + rays[i].direction.z * rays[i].direction.z;
                    EXPECT(std::fabs(len - 1.f) < 1e-5f && rays[i].pad == 0.f && rays[i].tmax == params.maxDistance);
                    if (surfels) EXPECT(surfels[i].distance == 0.f && (surfels[i].kind == 1 || surfels[i].kind == 2));
                }
                EXPECT(written == good + (withIndex ? 1 : 0));
                // a range that leaves the points, without an index
                if (!withIndex) EXPECT(ptss_probe_surface_rays(tri, T, sph, S, &params, points, P, 1, nullptr, n, rng, rays, surfels, &rejected) != 0);
                // no spheres, no triangles: every point of the missing kind is rejected, nothing is read
                EXPECT(ptss_probe_surface_rays(nullptr, 0, sph, S, &params, points, P, 0, index, n, rng, rays, surfels, &rejected) == 0);
                EXPECT(ptss_probe_surface_rays(tri, T, nullptr, 0, &params, points, P, 0, index, n, rng, rays, surfels, &rejected) == 0);
                calls += 2;
                free(surfels);
                free(rays);
                free(rng);
                free(index);
            }
    EXPECT(ptss_probe_surface_rays(tri, T, sph, S, nullptr, points, P, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != 0);
    free(points);

    // ---- the atlas ----
    {
        size_t K = 0;
        int H = 0;
        EXPECT(ptss_surface_atlas(tri, 0, T, 3.f, 1, 16, 20, nullptr, nullptr, 0, &H, &K) == 0 && K > 0 && H > 0);
        const size_t capacities[] = {K, K / 2, 1, 0};
        for (size_t capacity : capacities) {
            ptss_surface_point* out = block<ptss_surface_point>(capacity);
            uint32_t* texels = block<uint32_t>(capacity);
            size_t K2 = 0;
            int H2 = 0;
            EXPECT(ptss_surface_atlas(tri, 0, T, 3.f, 1, 16, 20, out, texels, capacity, &H2, &K2) == 0 && K2 == K && H2 == H);
            EXPECT(ptss_surface_atlas(tri, 0, T, 3.f, 1, 16, 20, out, nullptr, capacity, nullptr, &K2) == 0 && K2 == K);
            for (size_t k = 0; k < capacity; ++k) EXPECT(texels[k] < (uint32_t)(20 * H) && out[k].a + out[k].b < 1.f && out[k].a > 0.f && out[k].b > 0.f);
            calls += 2;
            free(texels);
            free(out);
        }
        EXPECT(ptss_surface_atlas(tri, 2, 3, 1.f, 2, 2, 2, nullptr, nullptr, 0, &H, &K) == 0 && K == 9 && H == 8);   // one block a shelf
        EXPECT(ptss_surface_atlas(tri, 0, T, 1.f, 1, 16, 8, nullptr, nullptr, 0, &H, &K) != 0);                      // maxSide > atlasWidth
        EXPECT(ptss_surface_atlas(nullptr, 0, 0, 1.f, 1, 4, 8, nullptr, nullptr, 0, &H, &K) == 0 && K == 0 && H == 0);
    }
    free(sph);
    free(tri);

    // ---- the gutter fill ----
    const int sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {2, 2}, {17, 9}, {33, 3}};
    const unsigned long long top = ~0ull;
    for (const auto& size : sizes) {
        const int w = size[0], h = size[1];
        const size_t N = (size_t)w * (size_t)h;
        for (int pattern = 0; pattern < 4; ++pattern) {
            ptss_linear_entry* film = block<ptss_linear_entry>(N);
            ptss_linear_entry* out = block<ptss_linear_entry>(N);
            for (size_t p = 0; p < N; ++p) {
                const bool empty = pattern == 0 ? (p * 7 + p / 3) % 3 != 0 : pattern == 1 ? true : pattern == 2 ? false : (p % (size_t)w + p / (size_t)w) % 2 == 0;
                film[p] = empty ? ptss_linear_entry{0ull, 0ull, 0ull, 0u, 0u}
                                : ptss_linear_entry{top - p, 1ull << 63, (unsigned long long)p * 12345ull, 0xfffffff0u + (uint32_t)(p % 8), (uint32_t)p};
            }
            memset(out, 0xcd, N * sizeof(ptss_linear_entry));
            EXPECT(ptss_probe_dilate_linear(film, w, h, out) == 0);
            EXPECT(ptss_probe_dilate_linear(out, w, h, film) == 0);   // the second pass, back into the first buffer
            EXPECT(ptss_probe_dilate_linear(film, w, h, film) != 0);
            calls += 2;
            free(out);
            free(film);
        }
    }
    if (failures) return 1;
    printf("surface_sanitize ok: %zu calls\n", calls);
    return 0;
}
