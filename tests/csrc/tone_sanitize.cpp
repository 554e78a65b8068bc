// tone_sanitize.cpp — a stand-alone host program over the tone probes (ptss_probe_tone_build, ptss_probe_tone_value, ptss_probe_tone_level,
// ptss_probe_resolve_toned: the host build of csrc/pttone.h), meant to be compiled with -fsanitize=address,undefined
// together with host/*.cpp and run on the CPU (tests/test_tone_cpu.py does). Every buffer is a heap block of exactly the size the call may
// touch — the table 2^bits + 4 floats, the film width * height entries, the pyramid the entries ptss_glare_layout counts, the outputs one
// row per pixel, the state 48 bytes — so a search that leaves the table, a tap that leaves a level or a pixel past the range is an error.
// The films hold entries without samples, means up to 2^40, and sums and weights no call of the library leaves, whose words wrap; the
// states hold NaN, 0, +inf and negative exposures, whose float-to-integer conversions must stay defined.
// Prints "tone_sanitize ok" and returns 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "ptss_host.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "tone_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static ptss_tone_params toneOf(int curve, int transfer, int bits, unsigned flags) {
    ptss_tone_params t = {(unsigned int)sizeof(ptss_tone_params), curve, transfer, bits, flags, 4.f, {2.51f, 0.03f, 2.43f, 0.59f, 0.14f}, 0u};
    return t;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const unsigned long long top = ~0ull;
    const unsigned long long values[] = {0, 1, 2, 3, 64, 1ull << 20, (1ull << 20) + 1, 1ull << 40, (1ull << 40) - 1, 3ull << 40, 1ull << 58, 1ull << 62, 1ull << 63, top, top - 1};
    const unsigned long long weights[] = {1, 0, 3, 65536, 5, 65535, 0, 3ull << 16, (1ull << 32) - 1, 1ull << 32, (1ull << 39) - 1, 1ull << 48, top};
    const size_t V = sizeof(values) / sizeof(values[0]), W = sizeof(weights) / sizeof(weights[0]);
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 5}, {3, 3}, {33, 9}};
    const float exposures[] = {1.f, nan, 0.f, inf, -2.f};
    const float xs[] = {nan, -inf, -1.f, -0.f, 0.f, 1e-45f, 1e-30f, 0.0031308f, 0.5f, 1.f, 4.f, 1e6f, 1099511627776.f, 3.4e38f, inf};
    const size_t X = sizeof(xs) / sizeof(xs[0]);
    ptss_linear_params params = {(unsigned int)sizeof(ptss_linear_params), 20, 65536.f, 1.5f, 0u};
    size_t builds = 0, resolves = 0;
    for (int curve = 0; curve < 3; ++curve)
        for (int transfer = 0; transfer < 2; ++transfer)
            for (int bits = 8; bits <= 10; bits += 2)
                for (unsigned flags = 0; flags < 2; ++flags) {
                    const ptss_tone_params tone = toneOf(curve, transfer, bits, flags);
                    const size_t floats = ((size_t)1 << bits) + 4;
                    const unsigned K = (1u << bits) - 1u;
                    float* table = (float*)malloc(floats * sizeof(float));
                    memset(table, 0x5a, floats * sizeof(float));
                    EXPECT(ptss_probe_tone_build(&tone, table) == 0);
                    ++builds;
                    EXPECT(table[0] == -inf && table[K + 2] == 0.f && std::isnan(table[K + 1]) && std::isnan(table[K + 3]) && std::isnan(table[K + 4]));
                    float* x = (float*)malloc(X * sizeof(float));
                    float* v = (float*)malloc(X * sizeof(float));
                    uint32_t* level = (uint32_t*)malloc(X * sizeof(uint32_t));
                    memcpy(x, xs, sizeof(xs));
                    EXPECT(ptss_probe_tone_value(&tone, x, v, X) == 0);
                    EXPECT(ptss_probe_tone_level(table, bits, x, level, X) == 0);
                    EXPECT(std::isnan(v[0]) && level[0] == 0u && level[1] == 0u && level[4] == 0u && level[X - 1] == K);
                    for (size_t i = 1; i < X; ++i) EXPECT(!std::isnan(v[i]) && v[i] >= 0.f && v[i] <= 1.f && level[i] <= K);
                    free(level);
                    free(v);
                    free(x);
                    for (const auto& size : sizes) {
                        const int w = size[0], h = size[1];
                        const size_t P = (size_t)w * (size_t)h;
                        for (int splat = 0; splat < 2; ++splat) {
                            unsigned long long* film = (unsigned long long*)malloc(P * 32);
                            for (size_t p = 0; p < P; ++p) {
                                film[4 * p] = values[p % V];
                                film[4 * p + 1] = values[(p * 7 + 3) % V];
                                film[4 * p + 2] = values[(p / 3 + p) % V];
                                film[4 * p + 3] = splat ? weights[(p * 5 + 1) % W] : ((weights[p % W] & 0xffffffffull) | (p % 4 << 32));
                            }
                            const int levels = 1 + (w + bits) % 4;
                            ptss_glare_level lv[8];
                            size_t entries = 0;
                            EXPECT(ptss_glare_layout(w, h, levels, lv, &entries) == 0);
                            ptss_glare_entry* pyr = (ptss_glare_entry*)malloc(entries * sizeof(ptss_glare_entry));
                            ptss_glare_params glare = {(unsigned int)sizeof(ptss_glare_params), levels, splat ? PTSS_GLARE_MIX : PTSS_GLARE_ADD, 0.75f, 0.25f, 0u};
                            EXPECT(ptss_probe_glare_build(film, splat, w, h, &params, &glare, pyr) == 0);
                            ptss_history_entry* lin = (ptss_history_entry*)malloc(P * sizeof(ptss_history_entry));
                            uint32_t* px = (uint32_t*)malloc(P * sizeof(uint32_t));
                            ptss_history_entry* hist = (ptss_history_entry*)malloc(P * sizeof(ptss_history_entry));
                            ptss_meter_state* state = (ptss_meter_state*)calloc(1, sizeof(ptss_meter_state));
                            memset(px, 0, P * sizeof(uint32_t));
                            for (float exposure : exposures) {
                                state->exposure = exposure;
                                EXPECT(ptss_probe_resolve_toned(film, splat, 0, P, &params, &tone, table, state, 0, 0, nullptr, nullptr, lin, px, hist) == 0);
                                EXPECT(ptss_probe_resolve_toned(film, splat, 0, P, &params, &tone, table, state, w, h, &glare, pyr, lin, px, hist) == 0);
                                resolves += 2;
                                bool alpha = true;
                                for (size_t p = 0; p < P; ++p) alpha = alpha && (bits == 10 ? px[p] >> 30 == 3u : px[p] >> 24 == 255u);
                                EXPECT(alpha);
                            }
                            // ranges that end at the film's end and start at its start, one pixel, nothing; every combination of outputs
                            EXPECT(ptss_probe_resolve_toned(film, splat, P / 2, P - P / 2, &params, &tone, table, nullptr, w, h, &glare, pyr, lin, nullptr, nullptr) == 0);
                            EXPECT(ptss_probe_resolve_toned(film, splat, 0, P / 2, &params, &tone, table, nullptr, 0, 0, nullptr, nullptr, nullptr, px, nullptr) == 0);
                            EXPECT(ptss_probe_resolve_toned(film, splat, P - 1, 1, &params, &tone, table, nullptr, w, h, &glare, pyr, nullptr, nullptr, hist) == 0);
                            EXPECT(ptss_probe_resolve_toned(film, splat, P, 0, &params, &tone, table, nullptr, w, h, &glare, pyr, lin, px, hist) == 0);
                            EXPECT(ptss_probe_resolve_toned(film, splat, 0, P, &params, &tone, table, nullptr, w, h, &glare, pyr, nullptr, nullptr, nullptr) == 0);
                            EXPECT(ptss_probe_resolve_toned(film, splat, 0, P + 1, &params, &tone, table, nullptr, w, h, &glare, pyr, lin, px, hist) != 0);
                            EXPECT(ptss_probe_resolve_toned(film, splat, P, 1, &params, &tone, table, nullptr, w, h, &glare, pyr, lin, px, hist) != 0);
                            resolves += 5;
                            free(state);
                            free(hist);
                            free(px);
                            free(lin);
                            free(pyr);
                            free(film);
                        }
                    }
                    free(table);
                }
    // what is refused is refused before a buffer is touched: the buffers here are one byte long
    {
        char* tiny = (char*)malloc(1);
        ptss_tone_params bad = toneOf(PTSS_TONE_FILMIC, PTSS_TRANSFER_SRGB, 9, 0u);
        EXPECT(ptss_probe_tone_build(&bad, (float*)tiny) != 0);
        bad = toneOf(PTSS_TONE_REINHARD, PTSS_TRANSFER_SRGB, 8, 0u);
        bad.white = nan;
        EXPECT(ptss_probe_tone_build(&bad, (float*)tiny) != 0);
        EXPECT(ptss_probe_tone_value(&bad, (const float*)tiny, (float*)tiny, 1) != 0);
        bad = toneOf(PTSS_TONE_FILMIC, PTSS_TRANSFER_GAMMA22, 10, 2u);
        EXPECT(ptss_probe_resolve_toned(tiny, 0, 0, 16, &params, &bad, (const float*)tiny, nullptr, 4, 4, nullptr, nullptr, nullptr, (uint32_t*)tiny, nullptr) != 0);
        bad = toneOf(PTSS_TONE_FILMIC, PTSS_TRANSFER_GAMMA22, 10, 0u);
        bad.filmic[0] = bad.filmic[2] = 3e38f;
        EXPECT(ptss_probe_tone_build(&bad, (float*)tiny) != 0);
        const ptss_tone_params good = toneOf(PTSS_TONE_FILMIC, PTSS_TRANSFER_SRGB, 8, 0u);
        EXPECT(ptss_probe_resolve_toned(tiny, 2, 0, 16, &params, &good, (const float*)tiny, nullptr, 4, 4, nullptr, nullptr, nullptr, (uint32_t*)tiny, nullptr) != 0);
        EXPECT(ptss_probe_resolve_toned(tiny, 0, 0, 16, &params, &good, (const float*)tiny, nullptr, 4, 4, nullptr, (const ptss_glare_entry*)tiny, nullptr, (uint32_t*)tiny, nullptr) != 0);
        EXPECT(ptss_probe_tone_level((const float*)tiny, 9, (const float*)tiny, (uint32_t*)tiny, 1) != 0);
        free(tiny);
    }
    if (failures) return 1;
    printf("tone_sanitize ok: %zu builds, %zu resolves\n", builds, resolves);
    return 0;
}
