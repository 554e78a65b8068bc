// ptglare.h — glare for a linear or a filtered linear film (ptss_glare_build, ptss_resolve_linear_glare / ptss_resolve_splat_glare;
// DESIGN.md §3.32): what a pixel's integer mean holds above a threshold, a pyramid of rounded integer averages of it, and the resolve that
// adds the pyramid's sum to the mean (or mixes the two) in front of the tone map. PTM_HD over ptmath.h, ptlinear.h, ptsplat.h and
// ptmeter.h: the host build of this header (libptss_host.so, ptss_probe_glare_build / ptss_probe_resolve_glare) is the specification, the
// kernels of ptss_glare.hip evaluate the same operations, and the two agree byte for byte.
//
// Everything in front of the resolve's float steps is unsigned 64-bit integer work: sums of integers and shifts, the same in any order,
// so a pyramid is the same bytes for every launch shape, for every tile size and whether a level was built in LDS or in global memory.
//
//   source   b = m > t ? m - t : 0 per channel, m = ptmeter::linearMean / splatMean (0 where the pixel has no samples), t the threshold
//            in the film's fixed point. Taking the threshold off every channel by itself is a design choice (a luminance key is not built)
//   down     d_k(i, j) = (sum over the 4 x 4 texels 2i-1 .. 2i+2 x 2j-1 .. 2j+2 of level k - 1, weights (1, 3, 3, 1) per axis, + 32) >> 6,
//            coordinates clamped to the level; level 0 is the source, level k is (w_{k-1} + 1) / 2 wide
//   up       u_L = d_L, u_k = d_k + up(u_{k+1}); up at x = 2i takes 3 a[i] + a[i-1], at x = 2i + 1 takes 3 a[i] + a[i+1], indices clamped, the
//            two axes multiply, (sum + 8) >> 4
//   resolve  g = (up(u_1) + L / 2) / L, s = (uint32_t)(strength * 65536 + 0.5), m' = (m * k + g * s + 32768) >> 16 with k = 65536 (ADD) or
//            65536 - s (MIX); then ptlin::showMean from (float)m' * 2^-scaleLog2. A pixel without samples whose m' is 0 in all channels
//            is the plain resolve's empty row, so strength = 0 gives the plain resolve's bytes everywhere (m * 65536 is taken in 64 bits:
//            everywhere on a film whose means stay below 2^48; the library leaves none above 2^40)
//
// Bounds, on a film the library filled (m <= 2^40: ptmeter.h). b <= m <= 2^40. The sixteen weights of a down sum to 64, so the sum is at
// most 2^46 and d <= (2^46 + 32) >> 6 = 2^40. The four weights of an up sum to 16: up(a) <= max a, so u_L <= 2^40 and u_k <= d_k +
// max u_{k+1} <= (L - k + 1) * 2^40. g <= (L * 2^40 + L / 2) / L = 2^40. With k, s <= 65536: m * k + g * s + 32768 <= 2^57 + 32768 and
// m' <= 2^41 (ADD), 2^40 (MIX: k + s = 65536). Nothing comes near 2^64. A film the caller filled with anything else wraps like any
// unsigned integer, on both sides alike; no address depends on a value.
#ifndef PTSS_PTGLARE_H
#define PTSS_PTGLARE_H
#include "ptmath.h"
#include "ptlinear.h"
#include "ptsplat.h"
#include "ptmeter.h"

namespace ptglare {

using ptlin::u64;

constexpr int kMaxLevels = PTSS_GLARE_MAX_LEVELS;
constexpr int kMaxSide = ptspl::kMaxFilmSide;
// the shapes of ptss_glare.hip. A reduce workgroup owns kTile x kTile texels of level 1 and stages the (2 kTile + 2)^2 film pixels under
// them; once the levels from some level T on hold no more than kTailEntries texels together (24 B each in LDS: just under 64 KiB), one
// workgroup builds them all in one launch
constexpr int kTile = 16;
constexpr int kStage = 2 * kTile + 2;
constexpr int kTailEntries = 2730;
constexpr int kTailBlock = 1024;

PTM_HD int clampTo(int v, int last) { return v < 0 ? 0 : (v > last ? last : v); }
PTM_HD int halfOf(int n) { return (n + 1) / 2; }

// what the threshold takes off one channel of a mean
PTM_HD u64 above(u64 m, u64 t) { return m > t ? m - t : 0ull; }

// the source of the pyramid at one film entry (w: the samples of a linear entry, the weight of a filtered one)
PTM_HD void sourceOf(u64 r, u64 g, u64 b, u64 w, bool splat, u64 t, u64* out) {
    if (w == 0ull) {
        out[0] = out[1] = out[2] = 0ull;
        return;
    }
    out[0] = above(splat ? ptmeter::splatMean(r, w) : ptmeter::linearMean(r, w), t);
    out[1] = above(splat ? ptmeter::splatMean(g, w) : ptmeter::linearMean(g, w), t);
    out[2] = above(splat ? ptmeter::splatMean(b, w) : ptmeter::linearMean(b, w), t);
}

// the weight of tap 0 .. 3 along one axis of a down
PTM_HD u64 downWeight(int tap) { return (tap == 0 || tap == 3) ? 1ull : 3ull; }

// texel (i, j) of a level from the level below it, w x h texels read through fetch(x, y, v[3])
template <class Fetch>
PTM_HD void downTexel(int i, int j, int w, int h, Fetch&& fetch, u64* out) {
    u64 acc[3] = {0ull, 0ull, 0ull};
    for (int dy = 0; dy < 4; ++dy) {
        const int y = clampTo(2 * j - 1 + dy, h - 1);
        for (int dx = 0; dx < 4; ++dx) {
            const int x = clampTo(2 * i - 1 + dx, w - 1);
            u64 v[3];
            fetch(x, y, v);
            const u64 wt = downWeight(dx) * downWeight(dy);
            for (int c = 0; c < 3; ++c) acc[c] += wt * v[c];
        }
    }
    for (int c = 0; c < 3; ++c) out[c] = (acc[c] + 32ull) >> 6;
}

// up(a) at texel (x, y) of the finer level, a the coarser one of w x h texels read through fetch(i, j, v[3])
template <class Fetch>
PTM_HD void upTexel(int x, int y, int w, int h, Fetch&& fetch, u64* out) {
    const int i = clampTo(x >> 1, w - 1), j = clampTo(y >> 1, h - 1);   // (x >> 1 < w on a level of the pyramid: the clamp is for safety's sake)
    const int i2 = clampTo((x & 1) ? i + 1 : i - 1, w - 1), j2 = clampTo((y & 1) ? j + 1 : j - 1, h - 1);
    u64 a[3], bx[3], by[3], bxy[3];
    fetch(i, j, a);
    fetch(i2, j, bx);
    fetch(i, j2, by);
    fetch(i2, j2, bxy);
    for (int c = 0; c < 3; ++c) out[c] = (9ull * a[c] + 3ull * bx[c] + 3ull * by[c] + bxy[c] + 8ull) >> 4;
}

// what the kernels take of a ptss_glare_params and of the film's ptss_linear_params
struct Rule {
    u64 threshold;    // in the film's fixed point
    uint32_t keep;    // k: 65536 (ADD) or 65536 - s (MIX)
    uint32_t s;       // the strength, 65536 being 1
    int levels;
};

PTM_HD u64 glareOf(u64 upSum, int levels) { return (upSum + (u64)(levels / 2)) / (u64)levels; }
PTM_HD u64 mixed(u64 m, u64 g, const Rule& R) { return (m * (u64)R.keep + g * (u64)R.s + 32768ull) >> 16; }

// one film entry resolved with up(u_1) at its pixel: ptlin::resolve's outputs (ptspl::resolve's where splat)
PTM_HD void resolve(u64 r, u64 g, u64 b, u64 w, bool splat, const u64* upSum, const Rule& R, const ptlin::Scale& sc, const float* T,
                    float* linear, uint32_t* px, float* hist) {
    const u64 sum[3] = {r, g, b};
    u64 shown[3];
    for (int c = 0; c < 3; ++c) {
        const u64 m = w == 0ull ? 0ull : (splat ? ptmeter::splatMean(sum[c], w) : ptmeter::linearMean(sum[c], w));
        shown[c] = mixed(m, glareOf(upSum[c], R.levels), R);
    }
    if (w == 0ull && (shown[0] | shown[1] | shown[2]) == 0ull) {
        ptlin::resolve(0ull, 0ull, 0ull, 0u, sc, T, linear, px, hist);   // the N = 0 rows
        return;
    }
    uint32_t word = 255u << 24;
    for (int c = 0; c < 3; ++c) ptlin::showMean((float)shown[c] * sc.down, c, sc, T, linear, &word, hist);
    linear[3] = hist[3] = splat ? (float)w * (1.f / ptspl::kOne) : (float)(uint32_t)w;
    *px = word;
}

// what the glare calls refuse about their parameters (PTSS_EINVAL), or nullptr. film: the film's parameters, already checked
inline const char* paramsError(const ptss_glare_params* p, const ptss_linear_params& film) {
    if (!p) return "glare params is null";
    if (p->structSize != sizeof(ptss_glare_params)) return "glare->structSize is not sizeof(ptss_glare_params)";
    if (p->levels < 1 || p->levels > kMaxLevels) return "levels must be in [1, 8]";
    if (p->mode != PTSS_GLARE_ADD && p->mode != PTSS_GLARE_MIX) return "unknown glare mode";
    if (!(p->strength >= 0.f && p->strength <= 1.f)) return "strength must be in [0, 1]";
    if (!(p->threshold >= 0.f) || !(p->threshold < ptm::inf())) return "threshold must be finite and not negative";
    if (!(p->threshold * ptlin::pow2(film.scaleLog2) <= ptlin::kMaxScaled)) return "threshold * 2^scaleLog2 must not exceed 2^40";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// what they refuse about the film's sides (PTSS_ERANGE), or nullptr
inline const char* sidesError(int width, int height) {
    if (width < 1 || height < 1 || width > kMaxSide || height > kMaxSide) return "width and height must be in [1, 2^22]";
    if ((unsigned long long)width * (unsigned long long)height >= (1ull << 31)) return "width * height must be below 2^31";
    return nullptr;
}

inline Rule ruleOf(const ptss_glare_params& p, const ptss_linear_params& film) {
    uint32_t flag = 0u;
    Rule R;
    R.threshold = ptlin::toFixed(p.threshold, p.threshold, ptlin::pow2(film.scaleLog2), &flag);   // rounded as a sample is, not clamped
    R.s = (uint32_t)(p.strength * 65536.f + 0.5f);
    R.keep = p.mode == PTSS_GLARE_MIX ? 65536u - R.s : 65536u;
    R.levels = p.levels;
    return R;
}

// the levels of a pyramid over a width x height film, one behind the other (ptss_glare_layout). The sides were checked by the caller
inline size_t layoutOf(int width, int height, int levels, ptss_glare_level* out) {
    unsigned long long first = 0ull;
    int w = width, h = height;
    for (int k = 0; k < levels; ++k) {
        w = halfOf(w);
        h = halfOf(h);
        out[k] = ptss_glare_level{w, h, first};
        first += (unsigned long long)w * (unsigned long long)h;
    }
    return (size_t)first;
}

// the level (1 .. levels) the tail kernel starts from: the first one from which on all levels hold at most kTailEntries texels together;
// `levels` itself when only the last level fits or none does (nothing is left for a tail to do: u_L = d_L)
inline int tailLevel(const ptss_glare_level* lv, int levels) {
    unsigned long long held = 0ull;
    int T = levels;
    for (int k = levels; k >= 1; --k) {
        held += (unsigned long long)lv[k - 1].width * (unsigned long long)lv[k - 1].height;
        if (held > (unsigned long long)kTailEntries) break;
        T = k;
    }
    return T;
}

}  // namespace ptglare
#endif
