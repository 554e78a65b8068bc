// meter_sanitize.cpp — a stand-alone host program over the meter's probes (ptss_probe_meter_bin, ptss_probe_meter_linear,
// ptss_probe_meter_splat, ptss_probe_meter_exposure: the host build of csrc/ptmeter.h), meant to be compiled with
// -fsanitize=address,undefined together with host/*.cpp and run on the CPU (tests/test_meter_cpu.py does). Every buffer is a heap block
// of exactly the size the call may touch — the histogram 329 words, the state 48 bytes, the film count entries — so a bin beyond the
// histogram or a pixel read past the range is an error; the rows are the adversarial ones: entries without samples, means at every power
// of two up to 2^40, sums and weights no call of the library leaves (2^64 - 1, weights of 2^39 - 1 and beyond), histograms that are empty,
// black, full in every bin, and states that are new, saturated and garbage. Prints "meter_sanitize ok" and returns 0 when every call
// answered as expected.
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
            fprintf(stderr, "meter_sanitize: line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

int main() {
    const unsigned long long top = ~0ull;
    std::vector<unsigned long long> values = {0, 1, 2, 3, 7, 8, 9, 255, 256, top, top - 1, 1ull << 63, (1ull << 63) - 1};
    for (int k = 0; k <= 62; ++k) {
        values.push_back(1ull << k);
        values.push_back((1ull << k) + 1);
    }
    const unsigned long long weights[] = {0, 1, 2, 3, 5, 65535, 65536, 65537, (1ull << 32) - 1, 1ull << 32, (1ull << 39) - 1, 1ull << 39, 1ull << 48, 1ull << 63, top};
    const size_t V = values.size(), W = sizeof(weights) / sizeof(weights[0]);
    const size_t P = V * W;
    ptss_linear_entry* lin = (ptss_linear_entry*)malloc(P * sizeof(ptss_linear_entry));
    ptss_splat_entry* spl = (ptss_splat_entry*)malloc(P * sizeof(ptss_splat_entry));
    size_t metered[2] = {0, 0};
    for (size_t i = 0; i < V; ++i)
        for (size_t j = 0; j < W; ++j) {
            const size_t p = i * W + j;
            lin[p] = ptss_linear_entry{values[i], values[(i * 7 + 3) % V], values[(i + j) % V], (uint32_t)weights[j], (uint32_t)(weights[j] >> 32)};
            spl[p] = ptss_splat_entry{values[i], values[(i * 5 + 1) % V], values[(i + 2 * j) % V], weights[j]};
            metered[0] += lin[p].samples != 0u;
            metered[1] += spl[p].weight != 0ull;
            int bin = 99999;
            unsigned long long Y = 0;
            EXPECT(ptss_probe_meter_bin((const unsigned long long*)&lin[p], 0, &bin, &Y) == 0);
            EXPECT(bin >= -1 && bin < PTSS_METER_BINS && (bin == -1) == (lin[p].samples == 0u) && (bin != 0 || Y == 0));
            EXPECT(ptss_probe_meter_bin((const unsigned long long*)&spl[p], 1, &bin, nullptr) == 0);
            EXPECT(bin >= -1 && bin < PTSS_METER_BINS && (bin == -1) == (spl[p].weight == 0ull));
        }
    // the whole film, sub-ranges that end at the film's end and start at its start, one pixel, nothing
    for (int splat = 0; splat < 2; ++splat) {
        uint32_t* hist = (uint32_t*)calloc(PTSS_METER_BINS, sizeof(uint32_t));
        auto meter = [&](size_t first, size_t count) {
            return splat ? ptss_probe_meter_splat(spl, first, count, hist) : ptss_probe_meter_linear(lin, first, count, hist);
        };
        EXPECT(meter(0, P) == 0);
        unsigned long long total = 0;
        for (int b = 0; b < PTSS_METER_BINS; ++b) total += hist[b];
        EXPECT(total == metered[splat]);
        EXPECT(meter(P - 1, 1) == 0 && meter(0, 1) == 0 && meter(P / 2, P - P / 2) == 0 && meter(P, 0) == 0 && meter(0, 0) == 0);
        EXPECT(meter(0, 1ull << 31) != 0 && meter(1ull << 31, 1) != 0);
        EXPECT(splat ? ptss_probe_meter_splat(nullptr, 0, 1, hist) != 0 : ptss_probe_meter_linear(nullptr, 0, 1, hist) != 0);
        free(hist);
    }
    free(lin);
    free(spl);

    // the exposure: histograms x parameters x states
    ptss_linear_params film{(unsigned)sizeof(ptss_linear_params), 20, 65536.f, 1.f, 0u};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    unsigned long long updates = 0;
    for (int kind = 0; kind < 6; ++kind) {
        uint32_t* hist = (uint32_t*)calloc(PTSS_METER_BINS, sizeof(uint32_t));
        if (kind == 1) hist[0] = 0xffffffffu;
        if (kind == 2) for (int b = 0; b < PTSS_METER_BINS; ++b) hist[b] = 0xffffffffu;
        if (kind == 3) hist[PTSS_METER_BINS - 1] = 1u;
        if (kind == 4) hist[1] = 1u;
        if (kind == 5) for (int b = 1; b < PTSS_METER_BINS; ++b) hist[b] = (uint32_t)(b * 2654435761u) >> (b % 29);
        for (int s : {0, 20, 32}) {
            film.scaleLog2 = s;
            film.clampMax = s == 0 ? 1099511627776.f : s == 20 ? 1048576.f : 256.f;
            const ptss_meter_params meters[] = {
                {(unsigned)sizeof(ptss_meter_params), 0.18f, 100u, 20u, 1.f, 1.f / 65536.f, 65536.f, 0u},
                {(unsigned)sizeof(ptss_meter_params), 1e-30f, 999u, 0u, 0.f, 0.f, 0.f, 0u},
                {(unsigned)sizeof(ptss_meter_params), 3e38f, 0u, 999u, 0.25f, 0.f, 3e38f, 0u},
                {(unsigned)sizeof(ptss_meter_params), 0.5f, 500u, 499u, 0.5f, 2.f, 2.f, 0u},
            };
            for (const ptss_meter_params& m : meters) {
                ptss_meter_state* state = (ptss_meter_state*)calloc(1, sizeof(ptss_meter_state));
                for (int round = 0; round < 3; ++round) {
                    EXPECT(ptss_probe_meter_exposure(hist, &film, &m, state) == 0);
                    ++updates;
                    EXPECT(state->updates == (uint32_t)(round + 1) && state->exposure >= m.minExposure && state->exposure <= m.maxExposure ? true
                                                                                                                                             : state->metered == 0);
                    EXPECT(state->black == hist[0] && (state->counted >= 1) == (state->metered >= 1));
                }
                // a saturated counter, and a state of garbage: garbage out, no fault
                state->updates = 0xffffffffu;
                EXPECT(ptss_probe_meter_exposure(hist, &film, &m, state) == 0 && state->updates == 0xffffffffu);
                memset(state, 0xff, sizeof(*state));
                EXPECT(ptss_probe_meter_exposure(hist, &film, &m, state) == 0);
                state->exposure = inf;
                state->meanLog2 = nan;
                EXPECT(ptss_probe_meter_exposure(hist, &film, &m, state) == 0);
                free(state);
            }
        }
        ptss_meter_params bad{(unsigned)sizeof(ptss_meter_params), nan, 100u, 20u, 1.f, 0.f, 1.f, 0u};
        ptss_meter_state st{};
        EXPECT(ptss_probe_meter_exposure(hist, &film, &bad, &st) != 0 && st.updates == 0u);
        free(hist);
    }
    EXPECT(updates > 0 && metered[0] > 0 && metered[1] > 0);
    if (failures) return 1;
    printf("meter_sanitize ok: %llu updates, %zu + %zu pixels metered\n", updates, metered[0], metered[1]);
    return 0;
}
