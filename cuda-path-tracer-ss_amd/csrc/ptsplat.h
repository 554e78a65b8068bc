// ptsplat.h — the filtered linear film of a path query (ptss_splat_paths / ptss_splat_paths_homed / ptss_resolve_splat):
// a sample's linear radiance, ptlinear.h's 64-bit fixed point, spread over the pixels around its position on the film by a box, a tent or
// a Gaussian whose weights are integers, and the resolve of a pixel's sums by its summed weight. PTM_HD over ptmath.h, ptquant.h and
// ptlinear.h: the host build of this header (libptss_host.so, ptss_probe_splat_paths / ptss_probe_resolve_splat) is the specification, the
// kernels of ptss_splat.hip evaluate the same operations in the same order, and the two agree byte for byte.
//
// A sample at (X, Y) and pixel column i: d = X - ((float)i + 0.5f) (exact operands: the film is at most 2^22 wide), f = profile(d) in float32,
// wq = (uint32_t)(f * 65536.f + 0.5f) in [0, 65536]; rows alike. A tap's weight is W = (wqx * wqy + 32768) >> 16, its contribution per
// channel (q * W + 32768) >> 16 with q = ptlin::toFixed(..) <= 2^40 (the product stays below 2^57), and W itself goes to the entry's weight.
// Everything added is an integer, so a film is the same bytes for every order of the samples and for every kernel that adds them.
#ifndef PTSS_PTSPLAT_H
#define PTSS_PTSPLAT_H
#include "ptlinear.h"

namespace ptspl {

using ptlin::u64;

constexpr float kMinRadius = 0.5f, kMaxRadius = 2.f;
constexpr int kMaxFilmSide = 1 << 22;   // (float)i + 0.5f is exact below it
constexpr float kOne = 65536.f;         // a weight of 1

// a ptss_splat_filter with its host-evaluated constants
struct Filter {
    int kind;
    float radius;
    float invR;    // 1 / radius (the tent)
    float alpha;   // the Gaussian
    float c;       // exp(-alpha R^2) (the Gaussian)
    int reach;     // taps are looked for in columns floor(X) - reach .. floor(X) + reach: 1 while R < 1.5, else 2
    int halo;      // K = floor(R + 0.5): the homes around a pixel whose closed square can reach it
};

// what the splat calls refuse about their filter, or nullptr
inline const char* filterError(const ptss_splat_filter* f) {
    if (!f) return "filter is null";
    if (f->structSize != sizeof(ptss_splat_filter)) return "filter->structSize is not sizeof(ptss_splat_filter)";
    if (f->kind != PTSS_SPLAT_BOX && f->kind != PTSS_SPLAT_TENT && f->kind != PTSS_SPLAT_GAUSSIAN) return "unknown splat filter kind";
    if (!(f->radius >= kMinRadius && f->radius <= kMaxRadius)) return "radius must be in [0.5, 2]";
    if (f->kind == PTSS_SPLAT_GAUSSIAN && (!(f->alpha > 0.f) || !(f->alpha < ptm::inf()))) return "alpha must be finite and positive";
    if (f->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

inline Filter filterOf(const ptss_splat_filter& f) {
    Filter F;
    F.kind = f.kind;
    F.radius = f.radius;
    F.invR = 1.0f / f.radius;
    F.alpha = f.kind == PTSS_SPLAT_GAUSSIAN ? f.alpha : 0.f;
    F.c = f.kind == PTSS_SPLAT_GAUSSIAN ? ptm::exp(-(f.alpha * (f.radius * f.radius))) : 0.f;
    F.reach = f.radius < 1.5f ? 1 : 2;
    F.halo = (int)(f.radius + 0.5f);
    return F;
}

// the per-axis profile at offset d from a pixel's centre; NaN gives 0
PTM_HD float profile(const Filter& F, float d) {
    if (F.kind == PTSS_SPLAT_BOX) return (d >= -F.radius && d < F.radius) ? 1.f : 0.f;
    if (F.kind == PTSS_SPLAT_TENT) return ptm::max(0.f, 1.f - ptm::abs(d) * F.invR);
    if (!(ptm::abs(d) < F.radius)) return 0.f;
    return ptm::max(0.f, ptm::exp(-(F.alpha * (d * d))) - F.c);
}

// the integer weight of pixel column (row) i for a sample at X (Y) along that axis
PTM_HD uint32_t axisWeight(const Filter& F, float X, int i) {
    const float d = X - ((float)i + 0.5f);
    return (uint32_t)(profile(F, d) * kOne + 0.5f);
}

// (wqx * wqy = 2^32 when both are 65536: the product is taken in 64 bits)
PTM_HD uint32_t tapWeight(uint32_t wqx, uint32_t wqy) { return (uint32_t)(((u64)wqx * (u64)wqy + 32768ull) >> 16); }
PTM_HD u64 contribution(u64 q, uint32_t W) { return (q * (u64)W + 32768ull) >> 16; }

// a coordinate the scatter form drops: not finite, or outside [-R, extent + R]
PTM_HD bool outside(float X, float radius, int extent) { return !(X >= -radius && X <= (float)extent + radius); }

// a sample that is not in its home's closed square (the homed form drops it); NaN is a stray
PTM_HD bool stray(float X, float Y, int hx, int hy) {
    return !(X >= (float)hx && X <= (float)(hx + 1) && Y >= (float)hy && Y <= (float)(hy + 1));
}

// the first column (row) to look for taps in: floor(X) - reach. X is finite and inside [-R, extent + R]
PTM_HD int firstTap(const Filter& F, float X) { return (int)__builtin_floorf(X) - F.reach; }

// the mean of a channel: floor((S * 2^16 + Wt / 2) / Wt) without the 80-bit product, as a float, times 2^-scaleLog2. The split is exact
// for Wt < 2^39 (rem << 16 stays below 2^55) and S / Wt < 2^48; a film the splat calls filled has S / Wt <= 2^24 + 1, every contribution
// being at most 2^24 W + 1/2
PTM_HD float meanOf(u64 sum, u64 Wt, float down) {
    const u64 a = sum / Wt, rem = sum % Wt;
    const u64 m = (a << 16) + ((rem << 16) + Wt / 2ull) / Wt;
    return (float)m * down;
}

// one film entry resolved, with ptlin::resolve's outputs; the weight written is (float)Wt * 2^-16
PTM_HD void resolve(u64 r, u64 g, u64 b, u64 Wt, const ptlin::Scale& sc, const float* T, float* linear, uint32_t* px, float* hist) {
    if (Wt == 0ull) {
        ptlin::resolve(0ull, 0ull, 0ull, 0u, sc, T, linear, px, hist);   // the N = 0 rows
        return;
    }
    const u64 sum[3] = {r, g, b};
    uint32_t word = 255u << 24;
    for (int c = 0; c < 3; ++c) ptlin::showMean(meanOf(sum[c], Wt, sc.down), c, sc, T, linear, &word, hist);
    linear[3] = hist[3] = (float)Wt * (1.f / kOne);
    *px = word;
}

}  // namespace ptspl
#endif
