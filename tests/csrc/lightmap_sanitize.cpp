// lightmap_sanitize.cpp — a stand-alone host program over the atlas with blocks and the light-map lookup (ptss_surface_atlas_blocks,
// ptss_probe_lookup_lightmap: the host builds of csrc/ptsurface.h and csrc/ptlightmap.h), meant to be compiled with
// -fsanitize=address,undefined together with host/*.cpp and run on the CPU (tests/test_lightmap_cpu.py does). Every buffer is a heap
// block of exactly the size the call may touch — the block tables as many rows as params counts, the map atlasWidth * atlasHeight
// entries, the materials as many as the count says, hits and rows n each, the atlas outputs `capacity` entries — so a gather through
// a bad block row, a bad primitive or material number or a tap outside a block's map is an error. The hits and block rows hold one of
// every kind the lookup rejects. Prints "lightmap_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "lightmap_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                           \
        }                                                                         \
    } while (0)

template <class T>
static T* block(size_t n) {
    return (T*)malloc(n ? n * sizeof(T) : 1);
}

static ptss_ray_hit hitOf(int kind, int primitive, float w1, float w2, ptss_vec3 normal, int material) {
    ptss_ray_hit h;
    memset(&h, 0, sizeof(h));
    h.kind = kind, h.primitive = primitive, h.w1 = w1, h.w2 = w2, h.normal = normal, h.materialIdx = material;
    return h;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    size_t calls = 0;
    const size_t T = 6, S = 3, M = 2;
    ptss_triangle* tri = block<ptss_triangle>(T);
    ptss_sphere* sph = block<ptss_sphere>(S);
    ptss_material* mat = block<ptss_material>(M);
    for (size_t t = 0; t < T; ++t) {
        const float k = (float)t + 1.f;
        tri[t] = ptss_triangle{{0.f, 0.f, 0.f}, {k, 0.f, 0.f}, {0.f, 0.5f * k, 0.f}, {0.f, 0.f, 1.f}, {0.f, 0.f, 1.f}, {0.f, 0.f, 1.f}, (int)(t % M)};
    }
    for (size_t k = 0; k < S; ++k) sph[k] = ptss_sphere{{(float)k, 1.f, -2.f}, 0.25f + 0.5f * (float)k, (int)(k % M)};
    memset(mat, 0, M * sizeof(ptss_material));
    mat[0].diffuseColor = ptss_vec3{0.5f, 1.f, 0.f};
    mat[1].diffuseColor = ptss_vec3{nan, 1e30f, -2.f};
    mat[1].emmitance = ptss_vec3{3.f, inf, nan};

    // ---- the atlas with blocks ----
    const int W = 24;
    size_t K = 0;
    int H = 0;
    EXPECT(ptss_surface_atlas_blocks(tri, 0, T, sph, 0, S, 2.f, 1, 12, W, nullptr, nullptr, nullptr, nullptr, 0, &H, &K) == 0 && K > 0 && H > 0);
    ptss_surface_block* bt = block<ptss_surface_block>(T);
    ptss_surface_block* bs = block<ptss_surface_block>(S);
    const size_t capacities[] = {K, K / 2, 1, 0};
    ptss_surface_point* points = nullptr;
    uint32_t* texels = nullptr;
    for (size_t capacity : capacities) {
        ptss_surface_point* out = block<ptss_surface_point>(capacity);
        uint32_t* tx = block<uint32_t>(capacity);
        size_t K2 = 0;
        int H2 = 0;
        EXPECT(ptss_surface_atlas_blocks(tri, 0, T, sph, 0, S, 2.f, 1, 12, W, bt, bs, out, tx, capacity, &H2, &K2) == 0 && K2 == K && H2 == H);
        EXPECT(ptss_surface_atlas_blocks(tri, 0, T, sph, 0, S, 2.f, 1, 12, W, nullptr, bs, out, nullptr, capacity, nullptr, &K2) == 0 && K2 == K);
        for (size_t k = 0; k < capacity; ++k) EXPECT(tx[k] < (uint32_t)(W * H));
        calls += 2;
        if (capacity == K) {
            points = out, texels = tx;
        } else {
            free(tx);
            free(out);
        }
    }
    for (size_t k = 0; k < S; ++k) EXPECT(bs[k].width == 2 * bs[k].height && bs[k].x + bs[k].width <= W && bs[k].y + bs[k].height <= H);
    {   // the triangle part is ptss_surface_atlas'
        size_t K3 = 0, K4 = 0;
        int H3 = 0, H4 = 0;
        EXPECT(ptss_surface_atlas(tri, 0, T, 2.f, 1, 12, W, nullptr, nullptr, 0, &H3, &K3) == 0);
        EXPECT(ptss_surface_atlas_blocks(tri, 0, T, nullptr, 0, 0, 2.f, 1, 12, W, bt, nullptr, nullptr, nullptr, 0, &H4, &K4) == 0 && K3 == K4 && H3 == H4);
        EXPECT(ptss_surface_atlas_blocks(tri, 0, T, sph, 0, S, 2.f, 1, 13, W, nullptr, nullptr, nullptr, nullptr, 0, &H4, &K4) != 0);   // 2 maxSide > width
        EXPECT(ptss_surface_atlas_blocks(tri, 0, T, nullptr, 0, S, 2.f, 1, 12, W, nullptr, nullptr, nullptr, nullptr, 0, &H4, &K4) != 0);
        EXPECT(ptss_surface_atlas_blocks(tri, 0, T, sph, 0, S, 2.f, 1, 12, W, bt, bs, nullptr, nullptr, 0, &H4, &K4) == 0);   // bt, bs as the lookup takes them
    }

    // ---- the lookup: a map of exactly W * H entries ----
    const size_t P = (size_t)W * (size_t)H;
    ptss_linear_entry* map = block<ptss_linear_entry>(P);
    memset(map, 0, P * sizeof(ptss_linear_entry));
    for (size_t k = 0; k < K; ++k) {
        const unsigned n = k % 5 == 0 ? 1u : (unsigned)(k % 7) + 2u;
        map[texels[k]] = ptss_linear_entry{(~0ull / 64) * n, (unsigned long long)k * 1000ull * n + n / 2, 77ull * n, n, 0u};
    }
    // the block tables with one of every rejected row appended, each table exactly as long as its count
    const ptss_surface_block badRows[] = {{-1, 0, 2, 2},      {0, -1, 2, 2},          {0, 0, -2, 2},      {0, 0, 2, -2},         {0, 0, 2, 0},
                                          {W - 1, 0, 2, 2},   {0, H - 1, 2, 2},       {2147483647, 0, 2, 2}, {0, 2147483647, 1, 1}, {0, 0, 8193, 1},
                                          {0, 0, 1, 4097},    {0, 0, -2147483647 - 1, 1}, {-2147483647 - 1, 0, 1, 1}, {3, 3, 0, 5}};
    const size_t B = sizeof(badRows) / sizeof(badRows[0]);
    ptss_surface_block* bt2 = block<ptss_surface_block>(T + B);
    ptss_surface_block* bs2 = block<ptss_surface_block>(S + B);
    memcpy(bt2, bt, T * sizeof(*bt));
    memcpy(bt2 + T, badRows, sizeof(badRows));
    memcpy(bs2, bs, S * sizeof(*bs));
    memcpy(bs2 + S, badRows, sizeof(badRows));

    std::vector<ptss_ray_hit> hits;
    const ptss_vec3 up = {0.f, 0.f, 1.f};
    for (size_t k = 0; k < K; ++k) {   // the atlas' own points
        const ptss_surface_point& p = points[k];
        if (p.surface & 0x40000000) {
            hits.push_back(hitOf(2, p.surface & 0x3fffffff, p.a, p.b, up, (int)(k % M)));
        } else {
            const float lon = (p.a - 0.5f) * 6.2831853f, lat = (p.b - 0.5f) * 3.14159265f;
            hits.push_back(hitOf(1, p.surface, 0.f, 0.f, ptss_vec3{std::sin(lon) * std::cos(lat), std::sin(lat), -std::cos(lon) * std::cos(lat)}, (int)(k % M)));
        }
    }
    const float places[] = {0.f, 1.f, -0.f, 0.5f, -3.f, 7.f, 1e30f, -1e30f, 3.4e38f, 1e-40f, 0.3333333f};
    for (float a : places)
        for (float b : places) hits.push_back(hitOf(2, (int)(hits.size() % T), a, b, up, 0));
    const ptss_vec3 normals[] = {{0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {1, 0, 0}, {-1, 0, 0}, {0, 0, 0}, {-1e-20f, 0, 1}, {1e-20f, 0, 1},
                                 {3e38f, 3e38f, 3e38f}, {-0.f, -0.f, -0.f}, {1e-45f, 1e-45f, -1e-45f}};
    for (const ptss_vec3& n : normals) hits.push_back(hitOf(1, (int)(hits.size() % S), 0.f, 0.f, n, 1));
    for (size_t k = 0; k < B; ++k) {
        hits.push_back(hitOf(2, (int)(T + k), 0.25f, 0.25f, up, 0));
        hits.push_back(hitOf(1, (int)(S + k), 0.f, 0.f, up, 0));
    }
    const int prims[] = {-1, (int)(T + B), (int)(S + B), 2147483647, -2147483647 - 1};
    for (int prim : prims) {
        hits.push_back(hitOf(2, prim, 0.25f, 0.25f, up, 0));
        hits.push_back(hitOf(1, prim, 0.f, 0.f, up, 0));
    }
    const int kinds[] = {0, 3, -1, 2147483647, -2147483647 - 1};
    for (int kind : kinds) hits.push_back(hitOf(kind, 0, 0.25f, 0.25f, up, 0));
    hits.push_back(hitOf(2, 0, nan, 0.25f, up, 0));
    hits.push_back(hitOf(2, 0, 0.25f, inf, up, 0));
    hits.push_back(hitOf(1, 0, 0.f, 0.f, ptss_vec3{nan, 0.f, 0.f}, 0));
    hits.push_back(hitOf(1, 0, 0.f, 0.f, ptss_vec3{0.f, -inf, 0.f}, 0));
    const int materials[] = {-1, (int)M, 2147483647, -2147483647 - 1};
    for (int m : materials) hits.push_back(hitOf(2, 0, 0.25f, 0.25f, up, m));

    const size_t n = hits.size();
    ptss_ray_hit* dh = block<ptss_ray_hit>(n);
    memcpy(dh, hits.data(), n * sizeof(ptss_ray_hit));
    ptss_linear_entry* out = block<ptss_linear_entry>(n);
    ptss_linear_params film = {(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.f, 0u};
    for (int filter = 0; filter < 2; ++filter)
        for (unsigned flags = 0; flags < 4; ++flags)
            for (int first = 0; first < 2; ++first) {
                ptss_lightmap_params p = {(unsigned int)sizeof(ptss_lightmap_params), W, H, filter, flags, first, (int)(T + B) - first, first, (int)(S + B) - first, 0u};
                uint32_t info[4] = {5u, 5u, 5u, 5u};
                memset(out, 0xcd, n * sizeof(ptss_linear_entry));
                EXPECT(ptss_probe_lookup_lightmap(mat, M, &p, &film, bt2 + first, bs2 + first, map, dh, n, out, info) == 0);
                ++calls;
                EXPECT((size_t)info[0] + info[1] + info[2] + info[3] == n + 20);
                EXPECT(info[3] > 5u + 2 * (B - 1) && info[2] > 5u && info[0] > 5u);
                size_t filtered = 0;
                for (size_t i = 0; i < n; ++i) {
                    EXPECT(out[i].clamped == 0u && out[i].samples <= 1u);
                    if (out[i].samples == 1u) ++filtered;
                    else EXPECT(out[i].r == 0ull && out[i].g == 0ull && out[i].b == 0ull);
                }
                EXPECT(filtered == info[0] - 5u);
                // without materials every hit is rejected under a flag and nothing is read through materialIdx
                EXPECT(ptss_probe_lookup_lightmap(nullptr, 0, &p, &film, bt2 + first, bs2 + first, map, dh, n, out, nullptr) == 0);
                // no tables: no blocks
                ptss_lightmap_params none = p;
                none.numTriangleBlocks = none.numSphereBlocks = 0;
                uint32_t info2[4] = {0u, 0u, 0u, 0u};
                EXPECT(ptss_probe_lookup_lightmap(mat, M, &none, &film, nullptr, nullptr, map, dh, n, out, info2) == 0 && info2[0] == 0u && info2[1] == 0u);
                calls += 2;
            }
    {   // refusals
        ptss_lightmap_params ok = {(unsigned int)sizeof(ptss_lightmap_params), W, H, 1, 0u, 0, (int)T, 0, (int)S, 0u};
        ptss_lightmap_params p = ok;
        p.filter = 2;
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &p, &film, bt2, bs2, map, dh, n, out, nullptr) != 0);
        p = ok, p.flags = 4u;
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &p, &film, bt2, bs2, map, dh, n, out, nullptr) != 0);
        p = ok, p.atlasWidth = 0;
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &p, &film, bt2, bs2, map, dh, n, out, nullptr) != 0);
        p = ok, p.numTriangleBlocks = -1;
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &p, &film, bt2, bs2, map, dh, n, out, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &ok, &film, bt2, bs2, map, dh, n, map, nullptr) != 0);   // out overlaps the map
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &ok, &film, nullptr, bs2, map, dh, n, out, nullptr) != 0);
        EXPECT(ptss_probe_lookup_lightmap(mat, M, &ok, &film, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == 0);   // n = 0
    }
    free(out), free(dh), free(bs2), free(bt2), free(map), free(texels), free(points), free(bs), free(bt), free(mat), free(sph), free(tri);
    if (failures) return 1;
    printf("lightmap_sanitize ok: %zu calls, %zu hits\n", calls, n);
    return 0;
}
