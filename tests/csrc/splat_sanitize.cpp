// splat_sanitize.cpp — a stand-alone host program over the filtered film's probes (ptss_probe_splat_paths, ptss_probe_resolve_splat:
// the host build of csrc/ptsplat.h), meant to be compiled with -fsanitize=address,undefined together with host/*.cpp
// and run on the CPU (tests/test_splat_cpu.py does). Every buffer is a heap block of exactly the size the call may touch, so a tap
// written outside the film or a row read past the batch is an error; the rows are the adversarial ones: positions on and around every
// film border, far outside, NaN and the infinities, radiance NaN, negative, huge and on the clamp, sums that start at 2^62, weights up
// to 2^39 - 1 in the resolve. Prints "splat_sanitize ok" and returns 0 when every call answered as expected.
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
            fprintf(stderr, "splat_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 3}, {5, 4}, {17, 16}, {40, 24}};
    const float radii[] = {0.5f, 1.0f, 1.5f, 2.0f};
    const float radiance[] = {nan, inf, -inf, -1.f, -0.f, 0.f, 1e-45f, 0.18f, 1.f, 40.f, 65536.f, 65537.f, 3e38f};
    ptss_linear_params params{(unsigned)sizeof(ptss_linear_params), 20, 65536.f, 0.7f, 0u};
    unsigned long long totalDropped = 0, totalClamped = 0, totalWeight = 0;
    for (const auto& size : sizes) {
        const int W = size[0], H = size[1];
        std::vector<float> xs, ys;
        for (int k = -3; k <= W + 3; ++k)
            for (float off : {0.f, 0.5f, -1e-6f, 1e-6f, 0.25f}) xs.push_back((float)k + off);
        for (int k = -3; k <= H + 3; ++k)
            for (float off : {0.f, 0.5f, -1e-6f, 1e-6f, 0.75f}) ys.push_back((float)k + off);
        for (float v : {nan, inf, -inf, 1e9f, -1e9f, 4194311.f, std::nextafter((float)W, inf), std::nextafter(0.f, -inf)}) {
            xs.push_back(v);
            ys.push_back(v);
        }
        const size_t n = xs.size() * ys.size();
        // exact-size heap blocks
        ptss_film_position* pos = (ptss_film_position*)malloc(n * sizeof(ptss_film_position));
        ptss_path_result* res = (ptss_path_result*)malloc(n * sizeof(ptss_path_result));
        size_t i = 0;
        for (float x : xs)
            for (float y : ys) {
                pos[i] = ptss_film_position{x, y};
                memset(&res[i], 0, sizeof(res[i]));
                res[i].radiance.x = radiance[i % 13];
                res[i].radiance.y = radiance[(i / 13) % 13];
                res[i].radiance.z = radiance[(i * 7 + 3) % 13];
                ++i;
            }
        const size_t P = (size_t)W * (size_t)H;
        for (int kind = 0; kind < 3; ++kind)
            for (float R : radii) {
                ptss_splat_filter f{(unsigned)sizeof(ptss_splat_filter), kind, R, kind == 2 ? 2.f : nan, 0u};
                ptss_splat_entry* film = (ptss_splat_entry*)malloc(P * sizeof(ptss_splat_entry));
                for (size_t p = 0; p < P; ++p) film[p] = ptss_splat_entry{1ull << 62, 1ull << 62, 0ull, 5ull << 16};
                unsigned long long dropped = ~0ull, clamped = ~0ull;
                EXPECT(ptss_probe_splat_paths(res, pos, nullptr, n, film, W, H, &f, &params, &dropped, &clamped) == 0);
                EXPECT(dropped > 0 && dropped < n && clamped > 0 && clamped <= n - dropped);
                totalDropped += dropped;
                totalClamped += clamped;
                // the homed form on every aligned window of the batch that fits the film: most samples are strays
                for (size_t first = 0; first < P; first += (P + 2) / 3) {
                    const size_t count = P - first < n ? P - first : n;
                    EXPECT(ptss_probe_splat_paths(res, pos, &first, count, film, W, H, &f, &params, &dropped, &clamped) == 0);
                    EXPECT(dropped <= count);
                }
                ptss_history_entry* lin = (ptss_history_entry*)malloc(P * sizeof(ptss_history_entry));
                ptss_history_entry* hist = (ptss_history_entry*)malloc(P * sizeof(ptss_history_entry));
                ptss_uchar4* px = (ptss_uchar4*)malloc(P * sizeof(ptss_uchar4));
                EXPECT(ptss_probe_resolve_splat(film, 0, P, &params, lin, px, hist) == 0);
                for (size_t p = 0; p < P; ++p) {
                    totalWeight += film[p].weight;
                    EXPECT(px[p].w == 255 && lin[p].weight == hist[p].weight && lin[p].weight >= 5.f);
                }
                EXPECT(ptss_probe_resolve_splat(film, P - 1, 1, &params, nullptr, px, nullptr) == 0);
                free(lin);
                free(hist);
                free(px);
                free(film);
            }
        free(pos);
        free(res);
    }
    // the resolve at the edges of its range: Wt = 0, 1, 2^39 - 1; S up to 2^63 - 1 (with S / Wt below 2^48)
    ptss_splat_entry edge[] = {{0, 0, 0, 0}, {123, 456, 789, 0}, {1ull << 47, 1, 0, 1}, {(1ull << 63) - 1, 1ull << 62, 12345, (1ull << 39) - 1},
                               {(1ull << 63) - 1, (1ull << 63) - 2, 1, 1ull << 16}, {1ull << 40, (1ull << 40) - 1, 3, 65535}};
    const size_t E = sizeof(edge) / sizeof(edge[0]);
    ptss_splat_entry* film = (ptss_splat_entry*)malloc(sizeof(edge));
    memcpy(film, edge, sizeof(edge));
    ptss_history_entry* lin = (ptss_history_entry*)malloc(E * sizeof(ptss_history_entry));
    for (int s : {0, 20, 32}) {
        ptss_linear_params p{(unsigned)sizeof(ptss_linear_params), s, s == 0 ? 1099511627776.f : s == 20 ? 1048576.f : 256.f, 1.f, 0u};
        EXPECT(ptss_probe_resolve_splat(film, 0, E, &p, lin, nullptr, nullptr) == 0);
        EXPECT(lin[0].weight == 0.f && lin[1].r == 0.f && lin[2].weight == 1.f / 65536.f && std::isfinite(lin[3].r) && std::isfinite(lin[4].g));
    }
    free(lin);
    free(film);
    EXPECT(totalDropped > 0 && totalClamped > 0 && totalWeight > 0);
    if (failures) return 1;
    printf("splat_sanitize ok: %llu dropped, %llu clamped\n", totalDropped, totalClamped);
    return 0;
}
