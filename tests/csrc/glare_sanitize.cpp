// glare_sanitize.cpp — a stand-alone host program over the glare probes (ptss_glare_layout, ptss_probe_glare_build,
// ptss_probe_resolve_glare: the host build of csrc/ptglare.h), meant to be compiled with -fsanitize=address,undefined
// together with host/*.cpp and run on the CPU (tests/test_glare_cpu.py does). Every buffer is a heap block of exactly the size the call may
// touch — the film width * height entries, the pyramid the entries ptss_glare_layout counts, the outputs one row per pixel, the state 48
// bytes — so a tap that leaves a level, a level that leaves the pyramid or a pixel past the range is an error. The sizes are the ones at
// which a clamp or a rounded-up half matters (one pixel, one row, one column, odd and even sides); the films hold entries without samples,
// means up to 2^40, and sums and weights no call of the library leaves (2^64 - 1, weights of 2^39 - 1 and beyond), whose words wrap.
// Prints "glare_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "glare_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    const unsigned long long top = ~0ull;
    const unsigned long long values[] = {0, 1, 2, 3, 64, 1ull << 20, (1ull << 20) + 1, 1ull << 40, (1ull << 40) - 1, 3ull << 40, 1ull << 58, 1ull << 62, 1ull << 63, top, top - 1};
    const unsigned long long weights[] = {1, 0, 3, 65536, 5, 65535, 0, 3ull << 16, (1ull << 32) - 1, 1ull << 32, (1ull << 39) - 1, 1ull << 48, top};
    const size_t V = sizeof(values) / sizeof(values[0]), W = sizeof(weights) / sizeof(weights[0]);
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 5}, {3, 3}, {2, 2}, {7, 4}, {37, 21}, {64, 48}, {65, 34}, {129, 3}};
    ptss_linear_params params = {(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.5f, 0u};
    const float thresholds[] = {0.f, 0.75f, 1048576.f};
    const float strengths[] = {0.f, 1.f / 65536.f, 0.1f, 1.f};
    size_t builds = 0, resolves = 0;
    for (const auto& size : sizes) {
        const int w = size[0], h = size[1];
        const size_t P = (size_t)w * (size_t)h;
        for (int splat = 0; splat < 2; ++splat) {
            unsigned long long* film = (unsigned long long*)malloc(P * 32);
            for (size_t p = 0; p < P; ++p) {
                film[4 * p] = values[p % V];
                film[4 * p + 1] = values[(p * 7 + 3) % V];
                film[4 * p + 2] = values[(p / 3 + p) % V];
                film[4 * p + 3] = splat ? weights[(p * 5 + 1) % W] : ((weights[p % W] & 0xffffffffull) | (p % 4 << 32));   // a linear entry's high half: clamped
            }
            for (int levels = 1; levels <= PTSS_GLARE_MAX_LEVELS; ++levels) {
                ptss_glare_level* lv = (ptss_glare_level*)malloc(8 * sizeof(ptss_glare_level));
                size_t entries = 0;
                EXPECT(ptss_glare_layout(w, h, levels, lv, &entries) == 0);
                EXPECT(entries >= (size_t)levels && lv[0].first == 0ull && lv[0].width == (w + 1) / 2 && lv[0].height == (h + 1) / 2);
                EXPECT(lv[levels - 1].first + (unsigned long long)lv[levels - 1].width * (unsigned long long)lv[levels - 1].height == entries);
                free(lv);
                ptss_glare_entry* pyr = (ptss_glare_entry*)malloc(entries * sizeof(ptss_glare_entry));
                memset(pyr, 0xab, entries * sizeof(ptss_glare_entry));
                const float threshold = thresholds[(levels + w) % 3];
                ptss_glare_params glare = {(unsigned int)sizeof(ptss_glare_params), levels, levels % 2 ? PTSS_GLARE_MIX : PTSS_GLARE_ADD, threshold, strengths[levels % 4], 0u};
                EXPECT(ptss_probe_glare_build(film, splat, w, h, &params, &glare, pyr) == 0);
                ++builds;
                bool fourthZero = true;
                for (size_t e = 0; e < entries; ++e) fourthZero = fourthZero && pyr[e].zero == 0ull;
                EXPECT(fourthZero);   // every entry was written
                ptss_history_entry* lin = (ptss_history_entry*)malloc(P * sizeof(ptss_history_entry));
                ptss_uchar4* px = (ptss_uchar4*)malloc(P * sizeof(ptss_uchar4));
                ptss_history_entry* hist = (ptss_history_entry*)malloc(P * sizeof(ptss_history_entry));
                ptss_meter_state* state = (ptss_meter_state*)calloc(1, sizeof(ptss_meter_state));
                state->exposure = 0.5f;
                memset(px, 0, P * sizeof(ptss_uchar4));
                // the whole film, ranges that end at its end and start at its start, one pixel, nothing; every combination of outputs
                EXPECT(ptss_probe_resolve_glare(film, splat, 0, P, &params, w, h, &glare, pyr, nullptr, lin, px, hist) == 0);
                bool opaque = true;
                for (size_t p = 0; p < P; ++p) opaque = opaque && px[p].w == 255;
                EXPECT(opaque);
                EXPECT(ptss_probe_resolve_glare(film, splat, P / 2, P - P / 2, &params, w, h, &glare, pyr, state, lin, nullptr, nullptr) == 0);
                EXPECT(ptss_probe_resolve_glare(film, splat, 0, P / 2, &params, w, h, &glare, pyr, state, nullptr, px, nullptr) == 0);
                EXPECT(ptss_probe_resolve_glare(film, splat, P - 1, 1, &params, w, h, &glare, pyr, nullptr, nullptr, nullptr, hist) == 0);
                EXPECT(ptss_probe_resolve_glare(film, splat, P, 0, &params, w, h, &glare, pyr, nullptr, lin, px, hist) == 0);
                EXPECT(ptss_probe_resolve_glare(film, splat, 0, P, &params, w, h, &glare, pyr, nullptr, nullptr, nullptr, nullptr) == 0);
                EXPECT(ptss_probe_resolve_glare(film, splat, 0, P + 1, &params, w, h, &glare, pyr, nullptr, lin, px, hist) != 0);
                EXPECT(ptss_probe_resolve_glare(film, splat, P, 1, &params, w, h, &glare, pyr, nullptr, lin, px, hist) != 0);
                resolves += 6;
                free(state);
                free(hist);
                free(px);
                free(lin);
                free(pyr);
            }
            free(film);
        }
    }
    // what is refused is refused before a buffer is touched: the buffers here are one byte long
    {
        char* tiny = (char*)malloc(1);
        ptss_glare_params glare = {(unsigned int)sizeof(ptss_glare_params), 9, PTSS_GLARE_MIX, 0.f, 0.1f, 0u};
        EXPECT(ptss_probe_glare_build(tiny, 0, 4, 4, &params, &glare, (ptss_glare_entry*)tiny) != 0);
        glare.levels = 3;
        glare.strength = std::numeric_limits<float>::quiet_NaN();
        EXPECT(ptss_probe_glare_build(tiny, 0, 4, 4, &params, &glare, (ptss_glare_entry*)tiny) != 0);
        glare.strength = 0.5f;
        glare.threshold = std::numeric_limits<float>::infinity();
        EXPECT(ptss_probe_resolve_glare(tiny, 1, 0, 16, &params, 4, 4, &glare, (const ptss_glare_entry*)tiny, nullptr, nullptr, (ptss_uchar4*)tiny, nullptr) != 0);
        glare.threshold = 0.f;
        EXPECT(ptss_probe_glare_build(tiny, 2, 4, 4, &params, &glare, (ptss_glare_entry*)tiny) != 0);
        EXPECT(ptss_probe_glare_build(tiny, 0, 0, 4, &params, &glare, (ptss_glare_entry*)tiny) != 0);
        EXPECT(ptss_probe_glare_build(tiny, 0, 1 << 22, 512, &params, &glare, (ptss_glare_entry*)tiny) != 0);
        size_t entries = 5;
        EXPECT(ptss_glare_layout(4, 4, 0, (ptss_glare_level*)tiny, &entries) != 0 && entries == 5);
        free(tiny);
    }
    if (failures) return 1;
    printf("glare_sanitize ok: %zu builds, %zu resolves\n", builds, resolves);
    return 0;
}
