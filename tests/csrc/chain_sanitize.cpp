// chain_sanitize.cpp — a stand-alone host program over the two host probes of the chain query (ptss_probe_specular_link,
// ptss_probe_lookup_lightmap_chain: the host builds of csrc/ptspecular.h's link factor and csrc/ptlightmap.h's step 6),
// meant to be compiled with -fsanitize=address,undefined together with host/*.cpp and run on the CPU (tests/test_chain_cpu.py does).
// Every buffer is a heap block of exactly the size the call may touch. The links cover the four material kinds the factor tells
// apart, a terminal one, misses, incidence from both sides, grazing and not finite directions; the chain rows hold throughputs that are
// not numbers, negative, above 1 and huge beside ordinary ones. Prints "chain_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "chain_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

template <class T>
static T* block(size_t n) {
    return (T*)malloc(n ? n * sizeof(T) : 1);
}

static ptss_material materialOf(float diff, float spec, float refr, float exponent, float ior, int flags, ptss_vec3 colour) {
    ptss_material m;
    memset(&m, 0, sizeof(m));
    m.specularColor = colour;
    m.diffAvg = diff, m.specAvg = spec, m.refrAvg = refr, m.specularExponent = exponent, m.indexOfRefraction = ior;
    m.flags = (char)flags;
    return m;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    size_t calls = 0;

    // ---- the link ----
    const size_t M = 6;
    ptss_material* mat = block<ptss_material>(M);
    const ptss_vec3 tintColour = {0.75f, 0.5f, 0.25f};
    mat[0] = materialOf(0.f, 0.9f, 0.f, inf, 1.5f, 1, tintColour);    // a flagged mirror
    mat[1] = materialOf(0.f, 0.8f, 0.f, inf, 1.5f, 0, tintColour);    // an unflagged mirror: Fresnel-weighted
    mat[2] = materialOf(0.f, 0.5f, 0.5f, inf, 1.5f, 0, tintColour);   // glass with a specular lobe
    mat[3] = materialOf(0.f, 0.f, 1.f, inf, 1.5f, 0, tintColour);     // glass without one
    mat[4] = materialOf(0.7f, 0.1f, 0.f, 20.f, 1.5f, 0, tintColour);  // terminal
    mat[5] = materialOf(0.f, 0.5f, 0.5f, inf, nan, 0, tintColour);    // glass whose index is not a number: nothing finite comes out
    const ptss_vec3 dirs[] = {{0.f, 0.f, -1.f},          {0.6f, 0.f, -0.8f},  {0.99999f, 0.f, -0.004472f}, {0.f, 0.f, 1.f},  {0.8f, 0.f, 0.6f},
                              {0.9999f, 0.f, 0.014142f}, {1.f, 0.f, 0.f},     {nan, 0.f, -1.f},            {inf, 0.f, -1.f}, {0.f, 0.f, 0.f}};
    const size_t D = sizeof(dirs) / sizeof(dirs[0]);
    const size_t n = (M + 1) * D;   // the last D hits are misses
    ptss_ray_query* rays = block<ptss_ray_query>(n);
    ptss_ray_hit* hits = block<ptss_ray_hit>(n);
    for (size_t i = 0; i < n; ++i) {
        const size_t m = i / D;
        rays[i] = ptss_ray_query{{0.f, 0.f, 2.f}, inf, dirs[i % D], 0.f};
        memset(&hits[i], 0, sizeof(ptss_ray_hit));
        hits[i].kind = m < M ? PTSS_HIT_TRIANGLE : PTSS_HIT_MISS;
        hits[i].materialIdx = m < M ? (int)m : -1;
        hits[i].normal = ptss_vec3{0.f, 0.f, 1.f};
        hits[i].point = ptss_vec3{0.25f, -0.5f, 0.f};
        hits[i].distance = 2.f;
    }
    ptss_ray_query* next1 = block<ptss_ray_query>(n);
    ptss_ray_query* next2 = block<ptss_ray_query>(n);
    int* follows1 = block<int>(n);
    int* follows2 = block<int>(n);
    ptss_vec3* factors = block<ptss_vec3>(n);
    memset(next1, 0xab, n * sizeof(ptss_ray_query));
    memset(next2, 0xab, n * sizeof(ptss_ray_query));
    memset(factors, 0xab, n * sizeof(ptss_vec3));
    EXPECT(ptss_probe_specular_step(rays, hits, n, mat, M, next1, follows1) == 0);
    EXPECT(ptss_probe_specular_link(rays, hits, n, mat, M, next2, follows2, factors) == 0);
    calls += 2;
    EXPECT(memcmp(next1, next2, n * sizeof(ptss_ray_query)) == 0 && memcmp(follows1, follows2, n * sizeof(int)) == 0);
    size_t followed = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t m = i / D;
        unsigned char untouched[sizeof(ptss_vec3)];
        memset(untouched, 0xab, sizeof(untouched));
        if (!follows2[i]) {
            EXPECT(memcmp(&factors[i], untouched, sizeof(untouched)) == 0);
            continue;
        }
        ++followed;
        EXPECT(m < 4);
        if (m == 0) EXPECT(factors[i].x == tintColour.x * 0.9f && factors[i].y == tintColour.y * 0.9f && factors[i].z == tintColour.z * 0.9f);
        if (m == 3 && follows2[i]) EXPECT(factors[i].x == factors[i].y && factors[i].y == factors[i].z);   // refracted: one number
        if (m < 4 && std::isfinite(dirs[i % D].x)) EXPECT(factors[i].x >= 0.f && factors[i].x <= 1.f);
    }
    EXPECT(followed >= 3 * D - 6);
    EXPECT(follows2[3 * D + 5] == 0);   // glass without a specular lobe, from inside beyond the critical angle: the chain ends
    EXPECT(follows2[2 * D + 5] == 1);   // with one: total internal reflection
    // refusals: whatever the step refuses, and a null factors
    EXPECT(ptss_probe_specular_link(rays, hits, n, mat, M, next2, follows2, nullptr) != 0);
    EXPECT(ptss_probe_specular_link(nullptr, hits, n, mat, M, next2, follows2, factors) != 0);
    EXPECT(ptss_probe_specular_link(rays, hits, n, mat, 2, next2, follows2, factors) != 0);   // a materialIdx outside the table
    EXPECT(ptss_probe_specular_link(nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr) == 0);
    calls += 4;

    // ---- the tinted lookup: a small atlas, its own points as hits ----
    const size_t T = 4;
    ptss_triangle* tri = block<ptss_triangle>(T);
    for (size_t t = 0; t < T; ++t) {
        const float k = (float)t + 1.f;
        tri[t] = ptss_triangle{{0.f, 0.f, 0.f}, {k, 0.f, 0.f}, {0.f, 0.5f * k, 0.f}, {0.f, 0.f, 1.f}, {0.f, 0.f, 1.f}, {0.f, 0.f, 1.f}, (int)(t % 2)};
    }
    const int W = 16;
    size_t K = 0;
    int H = 0;
    EXPECT(ptss_surface_atlas_blocks(tri, 0, T, nullptr, 0, 0, 2.f, 1, 8, W, nullptr, nullptr, nullptr, nullptr, 0, &H, &K) == 0 && K > 0 && H > 0);
    ptss_surface_block* bt = block<ptss_surface_block>(T);
    ptss_surface_point* points = block<ptss_surface_point>(K);
    uint32_t* texels = block<uint32_t>(K);
    EXPECT(ptss_surface_atlas_blocks(tri, 0, T, nullptr, 0, 0, 2.f, 1, 8, W, bt, nullptr, points, texels, K, &H, &K) == 0);
    const size_t P = (size_t)W * (size_t)H;
    ptss_linear_entry* map = block<ptss_linear_entry>(P);
    memset(map, 0, P * sizeof(ptss_linear_entry));
    for (size_t k = 0; k < K; ++k) {
        const unsigned s = (unsigned)(k % 3) + 1u;
        map[texels[k]] = ptss_linear_entry{(~0ull / 8) * s, (unsigned long long)k * 977ull * s, 5ull * s, s, 0u};
    }
    const float through[] = {1.f, 0.5f, 0.f, -0.f, -1.f, 2.f, 1e30f, inf, -inf, nan, 1.f / 65536.f, 0.999999f, 1e-30f, 0.25f};
    const size_t Q = sizeof(through) / sizeof(through[0]);
    const size_t N = K + 3;   // the atlas' own points, then a miss, a bad primitive and a bad kind
    ptss_ray_hit* lh = block<ptss_ray_hit>(N);
    ptss_chain_result* chain = block<ptss_chain_result>(N);
    ptss_chain_result* ones = block<ptss_chain_result>(N);
    memset(lh, 0, N * sizeof(ptss_ray_hit));
    for (size_t k = 0; k < N; ++k) {
        lh[k].normal = ptss_vec3{0.f, 0.f, 1.f};
        if (k < K) lh[k].kind = 2, lh[k].primitive = (int)(points[k].surface & 0x3fffffff), lh[k].w1 = points[k].a, lh[k].w2 = points[k].b;
        chain[k] = ptss_chain_result{{through[k % Q], through[(k / Q) % Q], through[(k + 5) % Q]}, (unsigned)(k % 9), {nan, inf, 0.f}, nan};
        ones[k] = ptss_chain_result{{1.f, 1.f, 1.f}, 0u, {0.f, 0.f, -1.f}, 1.f};
    }
    lh[K + 1].kind = 2, lh[K + 1].primitive = 2147483647;
    lh[K + 2].kind = 7;
    ptss_linear_entry* plain = block<ptss_linear_entry>(N);
    ptss_linear_entry* tinted = block<ptss_linear_entry>(N);
    ptss_linear_params film = {(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.f, 0u};
    ptss_material* lmat = block<ptss_material>(2);
    memset(lmat, 0, 2 * sizeof(ptss_material));
    lmat[0].diffuseColor = ptss_vec3{0.5f, 1.f, 0.25f};
    lmat[1].diffuseColor = ptss_vec3{1.f, 0.125f, 0.75f};
    lmat[1].emmitance = ptss_vec3{2.f, 0.f, 0.5f};
    for (int filter = 0; filter < 2; ++filter)
        for (unsigned flags = 0; flags < 4; ++flags) {
            ptss_lightmap_params p = {(unsigned int)sizeof(ptss_lightmap_params), W, H, filter, flags, 0, (int)T, 0, 0, 0u};
            uint32_t info0[4] = {0u, 0u, 0u, 0u}, info1[4] = {0u, 0u, 0u, 0u}, info2[4] = {3u, 3u, 3u, 3u};
            EXPECT(ptss_probe_lookup_lightmap(lmat, 2, &p, &film, bt, nullptr, map, lh, N, plain, info0) == 0);
            memset(tinted, 0xcd, N * sizeof(ptss_linear_entry));
            EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &p, &film, bt, nullptr, map, lh, ones, N, tinted, info1) == 0);
            EXPECT(memcmp(plain, tinted, N * sizeof(ptss_linear_entry)) == 0 && memcmp(info0, info1, sizeof(info0)) == 0);
            EXPECT(info0[0] == K && info0[2] == 2u && info0[3] == 1u);
            memset(tinted, 0xcd, N * sizeof(ptss_linear_entry));
            EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &p, &film, bt, nullptr, map, lh, chain, N, tinted, info2) == 0);
            calls += 3;
            for (int v = 0; v < 4; ++v) EXPECT(info2[v] == info0[v] + 3u);
            for (size_t k = 0; k < N; ++k) {
                EXPECT(tinted[k].samples == plain[k].samples && tinted[k].clamped == 0u);
                EXPECT(tinted[k].r <= plain[k].r && tinted[k].g <= plain[k].g && tinted[k].b <= plain[k].b);   // clamped at 1
                const float t = chain[k].throughput.x;
                if (t >= 1.f) EXPECT(tinted[k].r == plain[k].r);
                if (!(t > 0.f)) EXPECT(tinted[k].r == 0ull);
            }
        }
    {   // refusals
        ptss_lightmap_params ok = {(unsigned int)sizeof(ptss_lightmap_params), W, H, 1, 0u, 0, (int)T, 0, 0, 0u};
        ptss_lightmap_params p = ok;
        p.filter = 2;
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &p, &film, bt, nullptr, map, lh, chain, N, tinted, nullptr) != 0);
        p = ok, p.atlasHeight = 0;
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &p, &film, bt, nullptr, map, lh, chain, N, tinted, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &ok, &film, bt, nullptr, map, lh, nullptr, N, tinted, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &ok, &film, bt, nullptr, map, lh, chain, N, (ptss_linear_entry*)chain, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &ok, &film, bt, nullptr, map, lh, chain, N, map, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &ok, &film, nullptr, nullptr, map, lh, chain, N, tinted, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap_chain(lmat, 2, &ok, &film, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == 0);   // n = 0
        calls += 7;
    }
    free(lmat), free(tinted), free(plain), free(ones), free(chain), free(lh), free(map), free(texels), free(points), free(bt), free(tri);
    free(factors), free(follows2), free(follows1), free(next2), free(next1), free(hits), free(rays), free(mat);
    if (failures) return 1;
    printf("chain_sanitize ok: %zu calls, %zu links, %zu hits\n", calls, n, N);
    return 0;
}
