// linupsample_sanitize.cpp — a stand-alone host program over the probe of the linear films' upsample (ptss_probe_upsample_linear: the
// host build of csrc/ptlinup.h), meant to be compiled with -fsanitize=address,undefined together with host/*.cpp and
// run on the CPU (tests/test_linupsample_cpu.py does). Every buffer is a heap block of exactly the size the call may touch — the lo
// film and lo features width * height entries of 32 B, the hi features and the hi film factor^2 times as many, the info 24 B — so a
// tap, a wrapped column or a depth neighbour that leaves its frame is an error. The sizes are the ones at which a border or the wrap
// of a film one or two columns wide matters; the films hold entries without samples, means up to 2^40 and words no call of the
// library leaves, the features hold misses (an infinite depth), NaNs and huge depths.
// Prints "linupsample_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                               \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "linupsample_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                            \
        }                                                                          \
    } while (0)

static void fillFeatures(ptss_pixel_feature* features, size_t P, size_t salt) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t p = 0; p < P; ++p) {
        ptss_pixel_feature& f = features[p];
        const int kind = (int)((p * 13 + p / 5 + salt) % 11);
        f.normal = ptss_vec3{kind == 3 ? nan : 0.6f, 0.f, kind == 4 ? -0.8f : 0.8f};
        f.depth = kind == 5 ? 1e30f : (kind == 6 ? nan : 2.f + 0.01f * (float)(p % 97));
        f.albedo = ptss_vec3{0.5f, 0.5f, 0.5f};
        f.materialIdx = kind == 7 ? 3 : (int)((p / 3) % 2);
        if (kind < 2) {   // a miss
            f.normal = ptss_vec3{0.f, 0.f, 0.f};
            f.depth = inf;
            f.materialIdx = -1;
        }
    }
}

int main() {
    const unsigned long long top = ~0ull;
    const unsigned long long values[] = {0, 1, 2, 3, 64, 1ull << 20, (1ull << 20) + 1, 1ull << 40, (1ull << 40) - 1, 3ull << 40, 1ull << 58, 1ull << 62, 1ull << 63, top, top - 1};
    const unsigned long long weights[] = {1, 0, 3, 65536, 5, 65535, 0, 3ull << 16, (1ull << 32) - 1, 1ull << 32, (1ull << 39) - 1, 1ull << 48, top};
    const size_t V = sizeof(values) / sizeof(values[0]), W = sizeof(weights) / sizeof(weights[0]);
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 5}, {3, 3}, {7, 4}, {31, 7}, {33, 9}, {17, 3}};
    const ptss_linear_params scales[] = {{(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.5f, 0u},
                                         {(unsigned int)sizeof(ptss_linear_params), 0, 1099511627776.f, 1.f, 0u},
                                         {(unsigned int)sizeof(ptss_linear_params), 32, 256.f, 1.f, 0u}};
    size_t calls = 0;
    for (const auto& size : sizes) {
        const int w = size[0], h = size[1];
        const size_t P = (size_t)w * (size_t)h;
        for (int splat = 0; splat < 2; ++splat) {
            unsigned long long* film = (unsigned long long*)malloc(P * 32);
            ptss_pixel_feature* lo = (ptss_pixel_feature*)malloc(P * sizeof(ptss_pixel_feature));
            for (size_t p = 0; p < P; ++p) {
                film[4 * p] = values[p % V];
                film[4 * p + 1] = values[(p * 7 + 3) % V];
                film[4 * p + 2] = values[(p / 3 + p) % V];
                film[4 * p + 3] = splat ? weights[(p * 5 + 1) % W] : ((weights[p % W] & 0xffffffffull) | (p % 4 << 32));
            }
            fillFeatures(lo, P, 0);
            for (int factor = 1; factor <= 4; ++factor)
                for (unsigned int flags = 0; flags < 2; ++flags) {
                    const size_t Q = P * (size_t)(factor * factor);
                    const ptss_linear_params& params = scales[(factor + w) % 3];
                    const ptss_upsample_linear_params up = {(unsigned int)sizeof(ptss_upsample_linear_params), factor, factor % 2 ? 0.1f : 1e-20f,
                                                            factor % 3 ? 4.f : 1e20f, flags, 0u};
                    ptss_pixel_feature* hi = (ptss_pixel_feature*)malloc(Q * sizeof(ptss_pixel_feature));
                    ptss_linear_entry* out = (ptss_linear_entry*)malloc(Q * sizeof(ptss_linear_entry));
                    ptss_upsample_linear_info* info = (ptss_upsample_linear_info*)malloc(sizeof(ptss_upsample_linear_info));
                    fillFeatures(hi, Q, (size_t)factor);
                    memset(out, 0xab, Q * sizeof(ptss_linear_entry));
                    *info = ptss_upsample_linear_info{0ull, 0ull, 0ull};
                    EXPECT(ptss_probe_upsample_linear(film, splat, w, h, lo, hi, &params, &up, out, info) == 0);
                    EXPECT(ptss_probe_upsample_linear(film, splat, w, h, lo, hi, &params, &up, out, nullptr) == 0);
                    calls += 2;
                    EXPECT(info->filtered + info->fallback + info->empty == (unsigned long long)Q);
                    unsigned long long empty = 0;
                    for (size_t p = 0; p < Q; ++p) {
                        EXPECT(out[p].clamped == 0u);
                        if (out[p].samples == 0u) {
                            EXPECT(out[p].r == 0ull && out[p].g == 0ull && out[p].b == 0ull);
                            ++empty;
                        }
                    }
                    EXPECT(empty == info->empty);
                    // an output that overlaps the input film is refused
                    EXPECT(ptss_probe_upsample_linear(film, splat, w, h, lo, hi, &params, &up, (ptss_linear_entry*)film, info) != 0);
                    free(info);
                    free(out);
                    free(hi);
                }
            free(lo);
            free(film);
        }
    }
    if (failures) return 1;
    printf("linupsample_sanitize ok: %zu calls\n", calls);
    return 0;
}
