// linstats_sanitize.cpp — a stand-alone host program over the probes of the linear film's sampling plan
// (ptss_probe_accumulate_linear_stats, ptss_probe_plan_samples_linear, ptss_probe_linear_plan_weight: the host build of csrc/ptlinstats.h;
// DESIGN.md §3.33), meant to be compiled with -fsanitize=address,undefined together with host/*.cpp and run on the CPU
// (tests/test_linstats_cpu.py does). Every buffer is a heap block of exactly the size the call may touch — results n rows, index n words,
// film and moments filmPixels rows, cdf filmPixels words, info 32 bytes — so a pixel past the film or a shift, a conversion or a product
// that leaves its type is an error. The rows are the adversarial ones: NaN, infinities, negatives and clampMax in the samples, index
// entries beyond the film, moment words at every power of two, words that do not belong together, sample counts around the limits.
// Prints "linstats_sanitize ok" and returns 0 when every call answered as expected.
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
            fprintf(stderr, "linstats_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                        \
        }                                                                      \
    } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const unsigned long long top = ~0ull;
    unsigned long long samples = 0, plans = 0, weights = 0;

    // ---- the accumulate: three scales, with and without an index, with and without a film
    const struct { int scaleLog2; float clampMax; } scales[] = {{0, 1099511627776.f}, {20, 1048576.f}, {32, 256.f}, {20, 65536.f}};
    for (const auto& sc : scales) {
        const ptss_linear_params params{(unsigned)sizeof(ptss_linear_params), sc.scaleLog2, sc.clampMax, 1.f, 0u};
        const float unit = std::ldexp(1.f, -sc.scaleLog2);
        const float values[] = {nan, inf, -inf, -0.f, 0.f, -1.f, 1e-45f, 3e38f, sc.clampMax, std::nextafter(sc.clampMax, inf), std::nextafter(sc.clampMax, 0.f),
                                unit / 2, unit, 1.5f * unit, 0.18f, 0.5f, 1.f, 40.f};
        const size_t V = sizeof(values) / sizeof(values[0]), n = V * V, P = 37;
        ptss_path_result* res = (ptss_path_result*)malloc(n * sizeof(ptss_path_result));
        uint32_t* index = (uint32_t*)malloc(n * sizeof(uint32_t));
        for (size_t i = 0; i < n; ++i) {
            res[i] = ptss_path_result{{values[i % V], values[i / V], values[(i * 7 + 3) % V]}, 1};
            index[i] = i % 11 == 5 ? (uint32_t)(P + i) : i % 13 == 0 ? 0xffffffffu : (uint32_t)((i * 2654435761u) % P);
        }
        for (int withFilm = 0; withFilm < 2; ++withFilm) {
            ptss_linear_entry* film = withFilm ? (ptss_linear_entry*)calloc(P, sizeof(ptss_linear_entry)) : nullptr;
            ptss_linear_moment* mom = (ptss_linear_moment*)calloc(P, sizeof(ptss_linear_moment));
            for (size_t p = 0; p < P; p += 2) mom[p] = ptss_linear_moment{top - p, 1ull << 62, top, 5};   // words that wrap
            unsigned long long rejected = 99;
            EXPECT(ptss_probe_accumulate_linear_stats(res, index, 0, n, film, mom, P, &params, &rejected) == 0);
            unsigned long long kept = 0;
            for (size_t p = 0; p < P; ++p) kept += mom[p].samples - (p % 2 == 0 ? 5 : 0);
            EXPECT(kept + rejected == n && rejected > 0);
            samples += kept;
            // the identity map: exactly the last P pixels' worth of rays, from first pixels that just fit
            EXPECT(ptss_probe_accumulate_linear_stats(res, nullptr, 0, P, film, mom, P, &params, &rejected) == 0 && rejected == 0);
            EXPECT(ptss_probe_accumulate_linear_stats(res, nullptr, P - 1, 1, film, mom, P, &params, nullptr) == 0);
            EXPECT(ptss_probe_accumulate_linear_stats(res, nullptr, P, 0, film, mom, P, &params, nullptr) == 0);
            EXPECT(ptss_probe_accumulate_linear_stats(res, nullptr, P, 1, film, mom, P, &params, nullptr) != 0);
            EXPECT(ptss_probe_accumulate_linear_stats(res, nullptr, 1, P, film, mom, P, &params, nullptr) != 0);
            EXPECT(ptss_probe_accumulate_linear_stats(res, index, 0, n, film, nullptr, P, &params, nullptr) != 0);
            EXPECT(ptss_probe_accumulate_linear_stats(nullptr, index, 0, n, film, mom, P, &params, nullptr) != 0);
            if (film) EXPECT(film[0].samples > 0);
            free(film);
            free(mom);
        }
        free(res);
        free(index);
    }

    // ---- the weight and the plan: moment words at every power of two and their neighbours, crossed
    std::vector<unsigned long long> values = {0, 1, 2, 3, 7, 8, 9, 255, top, top - 1, (1ull << 63) - 1};
    for (int k = 2; k <= 63; ++k) {
        values.push_back(1ull << k);
        values.push_back((1ull << k) + 1);
        values.push_back((1ull << k) - 1);
    }
    const unsigned long long counts[] = {0, 1, 7, 8, 9, 63, 64, 1000, (1ull << 23) - 1, 1ull << 23, (1ull << 23) + 1, 1ull << 32, 1ull << 63, top};
    const size_t V = values.size(), W = sizeof(counts) / sizeof(counts[0]);
    const size_t P = V * W;
    ptss_linear_moment* mom = (ptss_linear_moment*)malloc(P * sizeof(ptss_linear_moment));
    for (size_t i = 0; i < V; ++i)
        for (size_t j = 0; j < W; ++j)
            mom[i * W + j] = ptss_linear_moment{values[i], values[(i * 7 + 3) % V], values[(i * 5 + j) % V], counts[j]};
    const struct { int scaleLog2; float clampMax; float floor; float threshold; uint32_t minS, maxS; } rules[] = {
        {20, 65536.f, 1.f / 64.f, 0.02f, 8u, 1u << 23}, {0, 1099511627776.f, 1.f, 0.f, 1u, 1u << 23}, {32, 256.f, 256.f, 3e38f, 8u, 8u},
        {20, 1048576.f, 1.f / 1048576.f, 0.f, 1u, 2u},  {0, 1099511627776.f, 1099511627776.f, 0.5f, 9u, 1000u}};
    for (const auto& r : rules) {
        const ptss_linear_params params{(unsigned)sizeof(ptss_linear_params), r.scaleLog2, r.clampMax, 1.f, 0u};
        const ptss_linear_plan_params plan{(unsigned)sizeof(ptss_linear_plan_params), r.minS, r.maxS, r.threshold, r.floor, {0u, 0u, 0u}};
        unsigned long long sum = 0;
        for (size_t p = 0; p < P; ++p) {
            const uint32_t w = ptss_probe_linear_plan_weight(&mom[p], &params, &plan);
            EXPECT(w <= (1u << 19));
            EXPECT((w == (1u << 19)) == (mom[p].samples < r.minS));
            sum += w;
            ++weights;
        }
        for (size_t n : {(size_t)1, (size_t)63, P, 3 * P + 1}) {
            unsigned long long* cdf = (unsigned long long*)malloc(P * sizeof(unsigned long long));
            uint32_t* index = (uint32_t*)malloc(n * sizeof(uint32_t));
            ptss_plan_info* info = (ptss_plan_info*)malloc(sizeof(ptss_plan_info));
            EXPECT(ptss_probe_plan_samples_linear(mom, P, &params, &plan, n, cdf, index, info) == 0);
            EXPECT(info->totalWeight == sum && cdf[P - 1] == sum && info->uniform == (sum == 0 ? 1u : 0u));
            for (size_t i = 0; i < n; ++i) EXPECT(index[i] < P && (i == 0 || index[i - 1] <= index[i]));
            EXPECT(ptss_probe_plan_samples_linear(mom, P, &params, &plan, n, cdf, index, nullptr) == 0);
            ++plans;
            free(cdf);
            free(index);
            free(info);
        }
        // one pixel, and the first and the last alone
        unsigned long long one = 0;
        uint32_t where = 9;
        EXPECT(ptss_probe_plan_samples_linear(mom + P - 1, 1, &params, &plan, 1, &one, &where, nullptr) == 0 && where == 0);
        EXPECT(ptss_probe_plan_samples_linear(mom, 1, &params, &plan, 1, &one, &where, nullptr) == 0 && where == 0);
        // refused: nothing is read
        ptss_linear_plan_params bad = plan;
        bad.floor = nan;
        EXPECT(ptss_probe_plan_samples_linear(mom, P, &params, &bad, 1, &one, &where, nullptr) != 0);
        bad = plan;
        bad.reserved[2] = 1u;
        EXPECT(ptss_probe_linear_plan_weight(mom, &params, &bad) == 0xffffffffu);
    }
    free(mom);
    EXPECT(samples > 0 && plans > 0 && weights > 0);
    if (failures) return 1;
    printf("linstats_sanitize ok: %llu samples kept, %llu weights, %llu plans\n", samples, weights, plans);
    return 0;
}
