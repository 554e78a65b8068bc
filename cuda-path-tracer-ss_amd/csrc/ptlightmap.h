// ptlightmap.h — reading a baked light map back (ptss_lookup_lightmap): from a ptss_ray_hit and the block tables of
// ptss_surface_atlas_blocks to an ordinary linear film row, written once for the gfx950 kernels (ptss_lightmap.hip) and for the host
// probe (host_capi.cpp ptss_probe_lookup_lightmap; tests/test_lightmap_cpu.py). The floats are float32 built from ptmath.h operations in
// the order written here, compiled without contraction on both sides; everything behind the place is integer work. The host build of
// this header is the specification of the device's rows. Per hit, in this order; the first verdict that applies is the hit's:
//
//  1. BLOCK    kind outside 0..2, or a w1, w2 or normal component that is not finite (a miss included): REJECTED.
//              kind 0: NO BLOCK. A triangle hit takes row k = primitive - firstTriangle of the triangle table when 0 <= k <
//              numTriangleBlocks, a sphere hit row primitive - firstSphere of the sphere table alike; no such row, or a row with
//              width == 0: NO BLOCK. The row is never trusted: x < 0, y < 0, width < 0, height < 0, height == 0, x + width >
//              atlasWidth, y + height > atlasHeight, width > 8192 or height > 4096: REJECTED, and no address is formed from it.
//              With a flag that needs the material (either one) and materialIdx outside the image's materials: REJECTED.
//  2. PLACE    triangle: fu = w1 * (float)width - kThird, fv = w2 * (float)height - kThird (one product and one difference each;
//                        kThird = 1.0f / 3.0f): the atlas' point (3 i + 1) / (3 s) lands on i.
//              sphere:   lon = atan2(n.x, -n.z), lat = atan2(n.y, sqrt(fma(n.z, n.z, n.x * n.x))) of the hit's normal n (ptlinrp.h's
//                        atan2 and project's expressions), a = div(lon, 2 pi) + 0.5, b = div(lat, pi) + 0.5,
//                        fu = a * (float)width - 0.5, fv = b * (float)height - 0.5.
//              Each is then held into [-1, side]: fu = min(max(fu, -1), (float)width) (w1 is any finite number; beyond these bounds
//              both taps of the axis are the block's edge texel, so nothing changes but the conversion below stays defined).
//              i0 = (int)floor(fu), fx = fu - floor(fu), qx = (int)(fx * 256 + 0.5f) in 0 .. 256; j0, qy alike.
//              PTSS_LIGHTMAP_NEAREST: q = q >= 128 ? 256 : 0 on both axes.
//              Tap t = 0 .. 3 is texel (i0 + (t & 1), j0 + (t >> 1)) with the INTEGER weight (t & 1 ? qx : 256 - qx) * (t >> 1 ? qy :
//              256 - qy); the four add up to 65,536. Columns clamp into [0, width - 1] on a triangle block and wrap modulo width on a
//              sphere block; rows clamp into [0, height - 1]. No tap leaves its block: the gutter between blocks is never read.
//  3. COUNT    a tap counts iff its weight is above 0 and its texel's samples are above 0. None: EMPTY.
//  4. MEAN     m_k = the film's own integer mean per channel, (sum + N / 2) / N (ptldn::meanOf; N == 1: the sum itself, no division).
//              W = the sum of the counted weights, S = the sum of w_k m_k (below 2^80: two words), m' = floor((S + W / 2) / W), exact.
//              A channel in which the counted taps agree keeps that integer (W m + W / 2 < W (m + 1)).
//  5. SHADE    PTSS_LIGHTMAP_MODULATE: q_c = clamp((int)(diffuseColor_c * 65536 + 0.5f), 0, 65536) of the hit's material (not a number,
//              or below 0: 0), m' = (m' q_c + 32768) >> 16 through a two-word product. PTSS_LIGHTMAP_EMISSION: m' += ptlin::toFixed(
//              emmitance_c, clampMax, 2^scaleLog2), saturating at 2^64 - 1.
//  6. ROW      FILTERED: {m'_r, m'_g, m'_b, samples = 1, clamped = 0}; every other verdict: all zero.
//
// ptss_lookup_lightmap_chain has a step 6 of its own after SHADE, in front of the row, for the light a chain of mirrors
// and glass lets through (ptss_intersect_chain's throughput, one ptss_chain_result per hit, never trusted):
//  6. TINT     per channel t_c = modulateWeight(throughput_c), step 5's conversion: clamp((int)(throughput_c * 65536 + 0.5f), 0, 65536),
//              0 for a throughput that is not a number or below 0 — and 65,536 for every throughput ABOVE 1: the tint is clamped at 1 —;
//              m' = (m' t_c + 32768) >> 16 through the same two-word product. A throughput of exactly 1 keeps m' (m' 2^16 + 2^15 >> 16).
//              The verdicts and counts are those of the plain lookup.
#pragma once
#include "ptlinrp.h"

namespace ptlm {
using namespace ptv;
using ptlin::u64;
using ptls::U128;

constexpr int kFiltered = 0, kEmpty = 1, kNoBlock = 2, kRejected = 3;   // the verdicts, in the order of dev_info's four counts
constexpr int kMaxBlockWidth = 8192, kMaxBlockHeight = 4096;
constexpr float kThird = 1.0f / 3.0f;
constexpr uint32_t kKnownFlags = PTSS_LIGHTMAP_MODULATE | PTSS_LIGHTMAP_EMISSION;

// what ptss_lookup_lightmap and ptss_probe_lookup_lightmap refuse with EINVAL about their parameters, or nullptr
inline const char* paramsError(const ptss_lightmap_params* p) {
    if (!p) return "lightmap params is null";
    if (p->structSize != (unsigned int)sizeof(ptss_lightmap_params))
        return "params->structSize is not sizeof(ptss_lightmap_params): start from ptss_default_lightmap_params";
    if (p->filter != PTSS_LIGHTMAP_NEAREST && p->filter != PTSS_LIGHTMAP_BILINEAR) return "unknown lightmap filter";
    if (p->flags & ~kKnownFlags) return "unknown lightmap flag";
    if (p->reserved != 0u) return "reserved must be 0";
    return nullptr;
}

// ... and with ERANGE
inline const char* rangeError(const ptss_lightmap_params* p) {
    if (p->atlasWidth < 1 || p->atlasHeight < 1) return "atlasWidth and atlasHeight must be positive";
    if ((unsigned long long)p->atlasWidth * (unsigned long long)p->atlasHeight >= (1ull << 31)) return "atlasWidth * atlasHeight must be below 2^31";
    if (p->firstTriangle < 0 || p->numTriangleBlocks < 0 || p->firstSphere < 0 || p->numSphereBlocks < 0)
        return "firsts and counts of the block tables must not be negative";
    return nullptr;
}

struct Rule {   // the constants of a call
    int atlasWidth, atlasHeight, filter;
    uint32_t flags;
    int firstTriangle, numTriangleBlocks, firstSphere, numSphereBlocks;
    int numMaterials;
    float clampMax, up;   // the film's ptlin::Scale
};

inline Rule ruleOf(const ptss_lightmap_params& p, const ptss_linear_params& film, int numMaterials) {
    return Rule{p.atlasWidth, p.atlasHeight, p.filter, p.flags, p.firstTriangle, p.numTriangleBlocks, p.firstSphere, p.numSphereBlocks,
                numMaterials, film.clampMax, ptlin::pow2(film.scaleLog2)};
}

struct Hit {   // rows 1 and 2 of a ptss_ray_hit
    vec3 normal;
    int materialIdx, kind, primitive;
    float w1, w2;
};

struct Block {   // a ptss_surface_block
    int x, y, width, height;
};

struct Texel {   // a ptss_linear_entry without its clamped count
    u64 r, g, b;
    uint32_t samples;
};

struct Place {   // steps 1 and 2 of a hit
    int status;   // kFiltered: go on; else the verdict
    bool sphere;
    Block block;
    int i0, j0;
    uint32_t qx, qy;
};

// step 1, before the table: kRejected, kNoBlock, or kFiltered with the table (*sphere) and the row to read; row < 0: no such row
PTM_HD int tableRow(const Hit& h, const Rule& R, bool* sphere, int* row) {
    *sphere = false;
    *row = -1;
    if (h.kind < PTSS_HIT_MISS || h.kind > PTSS_HIT_TRIANGLE) return kRejected;
    if (!(ptrp::finite(h.w1) && ptrp::finite(h.w2) && ptrp::finite(h.normal.x) && ptrp::finite(h.normal.y) && ptrp::finite(h.normal.z)))
        return kRejected;
    if (h.kind == PTSS_HIT_MISS) return kNoBlock;
    *sphere = h.kind == PTSS_HIT_SPHERE;
    const long long k = (long long)h.primitive - (long long)(*sphere ? R.firstSphere : R.firstTriangle);
    if (k < 0 || k >= (long long)(*sphere ? R.numSphereBlocks : R.numTriangleBlocks)) return kNoBlock;
    *row = (int)k;
    return kFiltered;
}

// step 1, the row read: kNoBlock, kRejected or kFiltered
PTM_HD int blockVerdict(const Block& b, const Hit& h, const Rule& R) {
    if (b.width == 0) return kNoBlock;
    if (b.x < 0 || b.y < 0 || b.width < 0 || b.height <= 0 || b.width > kMaxBlockWidth || b.height > kMaxBlockHeight) return kRejected;
    if (b.x > R.atlasWidth - b.width || b.y > R.atlasHeight - b.height) return kRejected;   // (no sum that could wrap)
    if (R.flags != 0u && (h.materialIdx < 0 || h.materialIdx >= R.numMaterials)) return kRejected;
    return kFiltered;
}

// one axis of step 2: f held into [-1, side], split into floor and the weight of the upper tap in 1/256
PTM_HD void splitAxis(float f, int side, int filter, int* lo, uint32_t* q) {
    f = ptm::min(ptm::max(f, -1.0f), (float)side);
    const float fl = __builtin_floorf(f);
    *lo = (int)fl;
    uint32_t w = (uint32_t)(int)((f - fl) * 256.0f + 0.5f);
    if (filter == PTSS_LIGHTMAP_NEAREST) w = w >= 128u ? 256u : 0u;
    *q = w;
}

// step 2 of a hit whose block passed blockVerdict
PTM_HD Place placeOf(const Hit& h, bool sphere, const Block& b, int filter) {
    float fu, fv;
    if (sphere) {
        const vec3 n = h.normal;
        const float lon = ptlrp::atan2(n.x, -n.z);
        const float lat = ptlrp::atan2(n.y, ptm::sqrt(ptm::fma(n.z, n.z, n.x * n.x)));
        fu = (ptm::div(lon, ptcam::kTwoPi) + 0.5f) * (float)b.width - 0.5f;
        fv = (ptm::div(lat, ptm::kPi) + 0.5f) * (float)b.height - 0.5f;
    } else {
        fu = h.w1 * (float)b.width - kThird;
        fv = h.w2 * (float)b.height - kThird;
    }
    Place p;
    p.status = kFiltered;
    p.sphere = sphere;
    p.block = b;
    splitAxis(fu, b.width, filter, &p.i0, &p.qx);
    splitAxis(fv, b.height, filter, &p.j0, &p.qy);
    return p;
}

// tap t = 0 .. 3 of a place: its weight, and its texel's number in the map when the weight is above 0
PTM_HD uint32_t tapOf(const Place& p, int t, int atlasWidth, uint32_t* texel) {
    const int di = t & 1, dj = t >> 1;
    const uint32_t w = (di ? p.qx : 256u - p.qx) * (dj ? p.qy : 256u - p.qy);
    int col = p.i0 + di, row = p.j0 + dj;   // in [-1, side + 1]
    if (p.sphere) {
        if (col < 0) col += p.block.width;
        if (col >= p.block.width) col -= p.block.width;
    }
    col = col < 0 ? 0 : (col > p.block.width - 1 ? p.block.width - 1 : col);   // (a sphere block of one column)
    row = row < 0 ? 0 : (row > p.block.height - 1 ? p.block.height - 1 : row);
    *texel = (uint32_t)(p.block.y + row) * (uint32_t)atlasWidth + (uint32_t)(p.block.x + col);   // inside the map: blockVerdict
    return w;
}

// step 4's mean of one channel of a texel with N >= 1 samples
PTM_HD u64 meanOf(u64 sum, uint32_t N) { return N == 1u ? sum : ptldn::meanOf(sum, (u64)N, false); }

struct Sums {   // W and S per channel
    U128 s[3];
    uint32_t W;
};

PTM_HD Sums noSums() { return Sums{{U128{0ull, 0ull}, U128{0ull, 0ull}, U128{0ull, 0ull}}, 0u}; }

PTM_HD U128 add128(U128 a, U128 b) {
    const u64 lo = a.lo + b.lo;
    return U128{lo, a.hi + b.hi + (lo < a.lo ? 1ull : 0ull)};
}

// steps 3 and 4 of one tap: nothing when it does not count
PTM_HD void addTap(Sums& S, uint32_t w, const Texel& e) {
    if (w == 0u || e.samples == 0u) return;
    S.s[0] = add128(S.s[0], ptls::mul64(meanOf(e.r, e.samples), (u64)w));
    S.s[1] = add128(S.s[1], ptls::mul64(meanOf(e.g, e.samples), (u64)w));
    S.s[2] = add128(S.s[2], ptls::mul64(meanOf(e.b, e.samples), (u64)w));
    S.W += w;
}

// floor((s + W / 2) / W) for W in [1, 65536] and s <= W (2^64 - 1): the quotient fits one word. W = 65536 is a shift; otherwise long
// division in 16-bit digits — the remainder stays below W <= 65535, so remainder * 2^16 + digit fits 32 bits and every division is a
// 32-bit one (gfx950 has no 64-bit division)
PTM_HD u64 divRound(U128 s, uint32_t W) {
    s = add128(s, U128{(u64)(W / 2u), 0ull});
    if (W == 65536u) return (s.lo >> 16) | (s.hi << 48);
    uint32_t rem = (uint32_t)s.hi % W;   // s.hi < W: its quotient digit is 0
    u64 q = 0ull;
    for (int k = 3; k >= 0; --k) {
        const uint32_t cur = (rem << 16) | (uint32_t)((s.lo >> (16 * k)) & 0xffffull);
        q = (q << 16) | (u64)(cur / W);
        rem = cur % W;
    }
    return q;
}

PTM_HD uint32_t modulateWeight(float c) {
    const float t = c * 65536.0f + 0.5f;
    if (!(t > 0.0f)) return 0u;   // not a number, the negatives
    return t >= 65536.0f ? 65536u : (uint32_t)(int)t;
}

// step 5 of one channel; diffuse, emission: the material's (read only with the flag)
PTM_HD u64 shade(u64 m, uint32_t flags, float diffuse, float emission, const Rule& R) {
    if (flags & PTSS_LIGHTMAP_MODULATE) {
        const U128 p = add128(ptls::mul64(m, (u64)modulateWeight(diffuse)), U128{32768ull, 0ull});
        m = (p.lo >> 16) | (p.hi << 48);
    }
    if (flags & PTSS_LIGHTMAP_EMISSION) {
        uint32_t flag = 0u;
        const u64 e = ptlin::toFixed(emission, R.clampMax, R.up, &flag);
        m = m + e < m ? ~0ull : m + e;
    }
    return m;
}

// step 6 of one channel (ptss_lookup_lightmap_chain only)
PTM_HD u64 tint(u64 m, float throughput) {
    const U128 p = add128(ptls::mul64(m, (u64)modulateWeight(throughput)), U128{32768ull, 0ull});
    return (p.lo >> 16) | (p.hi << 48);
}

// A whole hit, one tap after the other (the host probe; the kernel's one-lane form). blockTri(k) / blockSph(k) -> the Block of a table
// row inside its table; at(texel) -> the Texel of a texel inside the map; material(idx, row) -> xyz of row `row` of material idx inside
// the image (0: diffuseColor, 3: emmitance). out[0 .. 3): the row's r, g, b (zero unless kFiltered). Returns the verdict.
template <class BlockTri, class BlockSph, class At, class Material>
PTM_HD int lookup(const Hit& h, const Rule& R, BlockTri blockTri, BlockSph blockSph, At at, Material material, u64* out) {
    out[0] = out[1] = out[2] = 0ull;
    bool sphere;
    int row;
    int verdict = tableRow(h, R, &sphere, &row);
    if (verdict != kFiltered) return verdict;
    const Block b = sphere ? blockSph(row) : blockTri(row);
    verdict = blockVerdict(b, h, R);
    if (verdict != kFiltered) return verdict;
    const Place p = placeOf(h, sphere, b, R.filter);
    Sums S = noSums();
    for (int t = 0; t < 4; ++t) {
        uint32_t texel;
        const uint32_t w = tapOf(p, t, R.atlasWidth, &texel);
        if (w != 0u) addTap(S, w, at(texel));
    }
    if (S.W == 0u) return kEmpty;
    vec3 diffuse = v3(0, 0, 0), emission = v3(0, 0, 0);
    if (R.flags & PTSS_LIGHTMAP_MODULATE) diffuse = material(h.materialIdx, 0);
    if (R.flags & PTSS_LIGHTMAP_EMISSION) emission = material(h.materialIdx, 3);
    out[0] = shade(divRound(S.s[0], S.W), R.flags, diffuse.x, emission.x, R);
    out[1] = shade(divRound(S.s[1], S.W), R.flags, diffuse.y, emission.y, R);
    out[2] = shade(divRound(S.s[2], S.W), R.flags, diffuse.z, emission.z, R);
    return kFiltered;
}

}  // namespace ptlm
