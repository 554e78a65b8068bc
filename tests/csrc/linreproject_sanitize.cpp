// linreproject_sanitize.cpp — a stand-alone host program over the probes of ptss_reproject_linear (ptss_probe_reproject_linear,
// ptss_probe_reproject_linear_finish: the host build of csrc/ptlinrp.h), meant to be compiled with
// -fsanitize=address,undefined together with host/*.cpp and run on the CPU (tests/test_linreproject_cpu.py does). Every buffer is a
// heap block of exactly the size the call may touch — the previous film, moments and features prev.width * prev.height entries of 32 B,
// the new features, film and moments now.width * now.height — so a tap that leaves the previous film is an error. The features hold
// misses, NaNs, infinities and huge depths, the films and moments random words, the cameras stand up to 1e15 away and differ in kind
// and size: no NaN may reach an integer conversion (undefined behaviour) and no index may leave a buffer.
// Prints "linreproject_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                                \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "linreproject_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                             \
        }                                                                           \
    } while (0)

static unsigned long long state = 0x9e3779b97f4a7c15ull;
static unsigned long long next() {   // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return state * 0x2545f4914f6cdd1dull;
}

static ptss_film_camera cameraOf(int kind, int w, int h, float px, float py, float pz, float yaw) {
    ptss_film_camera f;
    memset(&f, 0, sizeof f);
    f.structSize = (unsigned int)sizeof f;
    f.kind = kind;
    f.camera.rotation = ptss_quat{0.f, std::sin(yaw / 2), 0.f, std::cos(yaw / 2)};
    f.camera.position = ptss_vec3{px, py, pz};
    f.camera.zNear = -0.1f;
    f.camera.zFar = 100.f;
    f.camera.fieldOfView = 0.9f;
    f.width = w, f.height = h;
    f.lensRadius = 0.05f, f.focusDistance = 4.f;
    f.jitter = 1;
    return f;
}

static void fillFeatures(ptss_pixel_feature* features, size_t P, int flavour) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t p = 0; p < P; ++p) {
        ptss_pixel_feature& f = features[p];
        const int kind = (int)((p * 13 + p / 5 + (size_t)flavour) % 13);
        f.normal = ptss_vec3{kind == 3 ? nan : 0.f, 0.f, kind == 4 ? -1.f : 1.f};
        f.depth = kind == 5 ? 1e30f : (kind == 6 ? nan : (kind == 8 ? inf : (kind == 9 ? -3.f : 3.f + 0.01f * (float)(p % 97))));
        f.albedo = ptss_vec3{0.5f, 0.5f, 0.5f};
        f.materialIdx = kind == 7 ? 3 : (int)(p % 2);
        if (kind < 2) {   // a miss
            f.normal = ptss_vec3{0.f, 0.f, 0.f};
            f.depth = inf;
            f.materialIdx = -1;
        }
    }
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 5}, {7, 4}, {33, 9}, {70, 37}};
    const ptss_linear_params scales[] = {{(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.5f, 0u},
                                         {(unsigned int)sizeof(ptss_linear_params), 0, 1099511627776.f, 1.f, 0u},
                                         {(unsigned int)sizeof(ptss_linear_params), 32, 256.f, 1.f, 0u}};
    const float far[] = {0.f, 0.25f, 1e15f, -3e30f};
    size_t calls = 0, seeded = 0;
    for (const auto& sn : sizes)
        for (const auto& sp : sizes) {
            const size_t Pn = (size_t)sn[0] * (size_t)sn[1], Pp = (size_t)sp[0] * (size_t)sp[1];
            ptss_pixel_feature* fnow = (ptss_pixel_feature*)malloc(Pn * sizeof(ptss_pixel_feature));
            ptss_pixel_feature* fprev = (ptss_pixel_feature*)malloc(Pp * sizeof(ptss_pixel_feature));
            ptss_pixel_motion* motion = (ptss_pixel_motion*)malloc(Pn * sizeof(ptss_pixel_motion));
            unsigned long long* film = (unsigned long long*)malloc(Pp * 32);
            unsigned long long* moments = (unsigned long long*)malloc(Pp * 32);
            unsigned long long* out = (unsigned long long*)malloc(Pn * 32);
            ptss_linear_moment* mout = (ptss_linear_moment*)malloc(Pn * 32);
            for (int round = 0; round < 12; ++round) {
                const int kindNow = round % 3, kindPrev = (round / 3) % 3, splat = round & 1;
                fillFeatures(fnow, Pn, round);
                fillFeatures(fprev, Pp, round % 2);   // every other round the two agree where the sizes do
                for (size_t p = 0; p < Pn; ++p) {
                    const int k = (int)(next() % 7);
                    motion[p].prevPoint = ptss_vec3{k == 0 ? nan : 0.1f * (float)(p % 11), k == 1 ? inf : 0.2f, k == 2 ? 1e38f : -3.f};
                    motion[p].surface = 0;
                }
                for (size_t w = 0; w < 4 * Pp; ++w) {
                    // random words; a third of the entries small enough to be a film the library filled, a tenth empty
                    const unsigned long long r = next();
                    const bool small = (w / 4) % 3 == 0;
                    film[w] = small ? (w % 4 == 3 ? (splat ? (r % 9) << 16 : r % 9) : r % (1ull << 30)) : r;
                    if (w % 4 == 3 && (w / 4) % 10 == 0) film[w] = 0ull;
                    moments[w] = small ? (w % 4 == 3 ? r % 9 : r % (1ull << 44)) : next();
                }
                const ptss_film_camera now = cameraOf(kindNow, sn[0], sn[1], far[round % 4], 0.f, 0.5f, 0.1f * (float)round);
                const ptss_film_camera prev = cameraOf(kindPrev, sp[0], sp[1], 0.f, far[(round / 2) % 4], 0.f, round == 7 ? 3.1f : 0.05f);
                ptss_reproject_linear_params prm = {(unsigned int)sizeof(ptss_reproject_linear_params), round % 2 ? -1.f : 0.9f, round % 3 ? 0.02f : 3e38f,
                                                    round % 4 ? 0.25f : 0.f, round % 5 ? 64u : (1u << 23) - 1u, 0u};
                const bool withMoments = round % 4 != 3, withMotion = round % 5 == 2;
                ptss_reproject_linear_info info = {0, 0, 0, 0};
                memset(out, 0xab, Pn * 32);
                memset(mout, 0xab, Pn * 32);
                EXPECT(ptss_probe_reproject_linear(&now, fnow, withMotion ? motion : nullptr, &prev, fprev, film, splat,
                                                   withMoments ? (const ptss_linear_moment*)moments : nullptr, &scales[round % 3], &prm, out,
                                                   withMoments ? mout : nullptr, &info) == 0);
                ++calls;
                EXPECT(info.seeded + info.offFilm + info.noTap == Pn);
                EXPECT(info.noVariance <= info.seeded);
                seeded += info.seeded;
                size_t counted = 0;
                for (size_t p = 0; p < Pn; ++p) {
                    const unsigned long long K = splat ? out[4 * p + 3] >> 16 : out[4 * p + 3];
                    EXPECT(K <= prm.maxHistory);
                    if (splat) EXPECT((out[4 * p + 3] & 65535ull) == 0ull);
                    if (K == 0ull) EXPECT(out[4 * p] == 0ull && out[4 * p + 1] == 0ull && out[4 * p + 2] == 0ull);
                    if (withMoments) EXPECT(K == 0ull ? mout[p].samples == 0ull : (mout[p].samples == K || mout[p].samples == 1ull));
                    counted += K != 0ull;
                }
                EXPECT(counted == info.seeded);
                // refusals: aliased outputs, moments on one side only
                EXPECT(ptss_probe_reproject_linear(&now, fnow, nullptr, &prev, fprev, film, splat, nullptr, &scales[0], &prm, film, nullptr, nullptr) != 0);
                EXPECT(ptss_probe_reproject_linear(&now, fnow, nullptr, &prev, fprev, film, splat, (const ptss_linear_moment*)moments, &scales[0], &prm, out,
                                                   nullptr, nullptr) != 0);
            }
            free(mout);
            free(out);
            free(moments);
            free(film);
            free(motion);
            free(fprev);
            free(fnow);
        }
    EXPECT(seeded > 0);
    float* h = (float*)malloc(12);
    unsigned long long* row = (unsigned long long*)malloc(32);
    unsigned long long* mrow = (unsigned long long*)malloc(32);
    const float colours[] = {0.f, -1.f, nan, inf, -inf, 0.5f, 1e-40f, 65536.f, 1e30f};
    const float counts[] = {0.f, 0.4f, 0.5f, 1.5f, 2.5f, 63.5f, 64.5f, 1e30f, inf, nan, -2.f};
    const float variances[] = {0.f, 0.3f, 0.5f, 1e6f, 16777216.f, 1e20f, 1208925819614629174706176.f};
    ptss_reproject_linear_params prm = {(unsigned int)sizeof(ptss_reproject_linear_params), 0.9f, 0.02f, 0.25f, (1u << 23) - 1u, 0u};
    for (float c : colours)
        for (float w : counts)
            for (float s2 : variances)
                for (int splat = 0; splat < 2; ++splat)
                    for (int has = 0; has < 2; ++has) {
                        h[0] = c, h[1] = 0.25f, h[2] = c;
                        EXPECT(ptss_probe_reproject_linear_finish(h, w, has, s2, splat, &scales[(int)calls % 3], &prm, row, mrow) == 0);
                        ++calls;
                    }
    EXPECT(ptss_probe_reproject_linear_finish(h, 2.f, 1, nan, 0, &scales[0], &prm, row, mrow) != 0);
    EXPECT(ptss_probe_reproject_linear_finish(h, 2.f, 1, -1.f, 0, &scales[0], &prm, row, mrow) != 0);
    EXPECT(ptss_probe_reproject_linear_finish(h, 2.f, 1, inf, 0, &scales[0], &prm, row, mrow) != 0);
    free(mrow);
    free(row);
    free(h);
    if (failures) return 1;
    printf("linreproject_sanitize ok: %zu calls, %zu pixels seeded\n", calls, seeded);
    return 0;
}
