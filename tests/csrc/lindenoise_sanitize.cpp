// lindenoise_sanitize.cpp — a stand-alone host program over the probes of the linear denoiser (ptss_probe_denoise_linear,
// ptss_probe_denoise_linear_finish: the host build of csrc/ptlindn.h), meant to be compiled with
// -fsanitize=address,undefined together with host/*.cpp and run on the CPU (tests/test_lindenoise_cpu.py does). Every buffer is a heap
// block of exactly the size the call may touch — film, moments, features and out width * height entries of 32 B, the plane width *
// height rows of 16 B — so a tap that leaves the frame is an error. The sizes are the ones at which a border or a spacing larger than
// the frame matters; the films hold entries without samples, means up to 2^40 and words no call of the library leaves, the moments hold
// words that wrap, the features hold misses (an infinite depth), NaNs and huge depths.
// Prints "lindenoise_sanitize ok" and returns 0 when every call answered as expected.
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
            fprintf(stderr, "lindenoise_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

int main() {
    const unsigned long long top = ~0ull;
    const unsigned long long values[] = {0, 1, 2, 3, 64, 1ull << 20, (1ull << 20) + 1, 1ull << 40, (1ull << 40) - 1, 3ull << 40, 1ull << 58, 1ull << 62, 1ull << 63, top, top - 1};
    const unsigned long long weights[] = {1, 0, 3, 65536, 5, 65535, 0, 3ull << 16, (1ull << 32) - 1, 1ull << 32, (1ull << 39) - 1, 1ull << 48, top};
    const unsigned long long counts[] = {0, 1, 2, 3, 8, 1000, (1ull << 23) - 1, 1ull << 40, top};
    const size_t V = sizeof(values) / sizeof(values[0]), W = sizeof(weights) / sizeof(weights[0]), K = sizeof(counts) / sizeof(counts[0]);
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 5}, {3, 3}, {7, 4}, {31, 7}, {33, 9}, {70, 37}, {129, 3}};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const ptss_linear_params scales[] = {{(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.5f, 0u},
                                         {(unsigned int)sizeof(ptss_linear_params), 0, 1099511627776.f, 1.f, 0u},
                                         {(unsigned int)sizeof(ptss_linear_params), 32, 256.f, 1.f, 0u}};
    size_t calls = 0;
    for (const auto& size : sizes) {
        const int w = size[0], h = size[1];
        const size_t P = (size_t)w * (size_t)h;
        for (int splat = 0; splat < 2; ++splat) {
            unsigned long long* film = (unsigned long long*)malloc(P * 32);
            unsigned long long* moments = (unsigned long long*)malloc(P * 32);
            ptss_pixel_feature* features = (ptss_pixel_feature*)malloc(P * sizeof(ptss_pixel_feature));
            for (size_t p = 0; p < P; ++p) {
                film[4 * p] = values[p % V];
                film[4 * p + 1] = values[(p * 7 + 3) % V];
                film[4 * p + 2] = values[(p / 3 + p) % V];
                film[4 * p + 3] = splat ? weights[(p * 5 + 1) % W] : ((weights[p % W] & 0xffffffffull) | (p % 4 << 32));
                moments[4 * p] = values[(p * 3 + 1) % V];
                moments[4 * p + 1] = values[(p * 5 + 2) % V];
                moments[4 * p + 2] = values[(p * 11 + 4) % V];
                moments[4 * p + 3] = counts[(p * 2 + p / 7) % K];
                ptss_pixel_feature& f = features[p];
                const int kind = (int)((p * 13 + p / 5) % 11);
                f.normal = ptss_vec3{kind == 3 ? nan : 0.6f, 0.f, kind == 4 ? -0.8f : 0.8f};
                f.depth = kind == 5 ? 1e30f : (kind == 6 ? nan : 2.f + 0.01f * (float)(p % 97));
                f.albedo = ptss_vec3{0.5f, 0.5f, 0.5f};
                f.materialIdx = kind == 7 ? 3 : (int)(p % 2);
                if (kind < 2) {   // a miss
                    f.normal = ptss_vec3{0.f, 0.f, 0.f};
                    f.depth = inf;
                    f.materialIdx = -1;
                }
            }
            for (int levels = 0; levels <= PTSS_DENOISE_MAX_LEVELS; ++levels) {
                const ptss_linear_params& params = scales[(levels + w) % 3];
                ptss_denoise_linear_params denoise = {(unsigned int)sizeof(ptss_denoise_linear_params), levels, levels % 2 ? 3.f : 1e-20f, 0.1f, levels % 3 ? 4.f : 1e20f, {0u, 0u, 0u}};
                ptss_linear_entry* out = (ptss_linear_entry*)malloc(P * sizeof(ptss_linear_entry));
                float* plane = (levels % 2) ? (float*)malloc(P * 16) : nullptr;
                memset(out, 0xab, P * sizeof(ptss_linear_entry));
                EXPECT(ptss_probe_denoise_linear(film, splat, w, h, (const ptss_linear_moment*)moments, features, &params, &denoise, out, plane) == 0);
                ++calls;
                for (size_t p = 0; p < P; ++p) {
                    const unsigned long long weight = splat ? film[4 * p + 3] : (film[4 * p + 3] & 0xffffffffull);
                    if (weight == 0ull) {
                        EXPECT(out[p].r == 0ull && out[p].g == 0ull && out[p].b == 0ull && out[p].samples == 0u && out[p].clamped == 0u);
                        if (plane) EXPECT(plane[4 * p + 3] == -1.f);
                    } else {
                        EXPECT(out[p].samples != 0u);
                        if (!splat) EXPECT(out[p].samples == (uint32_t)weight && out[p].clamped == (uint32_t)(film[4 * p + 3] >> 32));
                        if (plane) EXPECT(plane[4 * p + 3] >= 0.f);   // never NaN, never the mark of an empty pixel
                    }
                }
                EXPECT(ptss_probe_denoise_linear(film, splat, w, h, (const ptss_linear_moment*)moments, features, &params, &denoise, (ptss_linear_entry*)film, plane) != 0);
                free(plane);
                free(out);
            }
            free(features);
            free(moments);
            free(film);
        }
    }
    float* rgb = (float*)malloc(12);
    unsigned long long* row = (unsigned long long*)malloc(32);
    const float colours[] = {0.f, -1.f, nan, inf, -inf, 0.5f, 1e-40f, 65536.f, 1e30f};
    for (float c : colours)
        for (unsigned long long w3 : weights)
            for (int splat = 0; splat < 2; ++splat) {
                rgb[0] = c, rgb[1] = 0.25f, rgb[2] = c;
                EXPECT(ptss_probe_denoise_linear_finish(rgb, w3, splat, &scales[0], row) == 0);
                ++calls;
            }
    free(row);
    free(rgb);
    if (failures) return 1;
    printf("lindenoise_sanitize ok: %zu calls\n", calls);
    return 0;
}
