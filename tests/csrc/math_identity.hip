// math_identity.hip — the shared math of csrc/ptmath.h on the device against the SAME functions in the g++ build of libptss_host.so
// (the build the oracle's results and every host probe come from), bit for bit, on the GPU it runs on. Nothing is compared on the
// device: one trivial kernel per operation writes f(pattern) into a buffer; the host copies it back, evaluates the same patterns
// through ptss_probe_math / ptss_probe_quantize / ptss_probe_vector (never through hipcc's host pass over the header, which would
// be a third compilation) on at most 16 threads and compares 32-bit words. A NaN equals a NaN of any payload.
//
//   sin cos tan atan log exp        every one of the 2^32 float32 patterns
//   pow_gamma                       pow(x, kGamma), every pattern of x
//   quantize                        ptq::quantize_literal, every pattern (the device literal form is what checkQuantize of
//                                   math_exhaustive.hip holds the table form against)
//   pow_grid                        pow(x, y) for all pairs of a grid: every biased exponent x both signs x 16 mantissas, +-0, +-inf,
//                                   NaNs, denormals, 1 and its neighbours; y has 1 / (e + 1) of the presets' Phong exponents besides
//   dot cross div_scalar madd_scalar madd_vector rotate quat_mul normalize_vec3 normalize_quat length
//                                   the pinned fma chains of the vector layer (csrc/ptvecops.h says which operands go where) on
//                                   components from the recipe of guards_device.hip
//
// Every pattern runs in two orders, because ptm::div and ptm::rcp (inside tan and atan, normalize, length, vec3 / float) leave their
// fast path per WAVE: what a lane computes depends on what the other 63 hold.
//   sorted     pattern(i) = i: a wave holds 64 neighbours and takes the fast path or the escape as a whole.
//   scattered  pattern(i) = i * 2654435761 mod 2^32 (odd multiplier: a bijection): a wave holds 64 unrelated exponents and signs and
//              takes the per-lane select.
// The host values do not depend on the order and are computed once per chunk of 2^26 consecutive patterns. A wave of the scattered
// order holds patterns of every chunk, so the scattered kernel runs all 2^32 threads for every chunk — each thread in its own wave,
// with its own 63 neighbours — and keeps the results whose pattern lies in the chunk (64 times the device work, still well under a
// second per operation; the alternative is a 16 GiB buffer).
//
// Controls — columns that MUST count mismatches, or the comparison proves nothing: exp through the hardware exp2, sincos with the
// third Cody-Waite step left out, dot without the fma chain.
//
// One line per operation and order: "<op> <order> checked=N mismatch=M first=0x.. device=0x.. host=0x.." (first: the smallest
// mismatching pattern, or case index for the grid and the vectors), and "<op> control_<name> checked=N mismatch=M".
// Any HIP error ends the program at once with status 2; mismatches give status 1.
// usage: ptss_identitycheck [op [sorted|scattered|both]]        (no argument: every operation, both orders)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "ptmath.h"
#include "ptquant.h"
#include "ptss_host.h"
#include "ptvecops.h"

namespace {

constexpr uint32_t kScatter = 2654435761u;
constexpr uint32_t kChunk = 1u << 26;
constexpr size_t kHostBlock = 1u << 14;   // patterns a host thread hands to a probe at a time

#define HIP_OK(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) {                                                                                       \
            printf("hip error %d (%s) at %s\n", (int)e_, hipGetErrorString(e_), #expr);                               \
            fflush(stdout);                                                                                           \
            exit(2);                                                                                                  \
        }                                                                                                             \
    } while (0)

// ---- device side ---------------------------------------------------------------------------------------------------------------------
enum Unary { kSin = 0, kCos, kTan, kAtan, kLog, kExp, kPowGamma, kQuantize, kExpHardware, kSinTwoStep, kCosTwoStep };

// ptm::sincos as written in ptmath.h, with the third Cody-Waite step left out (a control: it must differ somewhere)
__device__ void sincosTwoStep(float x, float& s, float& c) {
    if (!(ptm::abs(x) <= 1.0e4f)) {
        s = ptm::qnan();
        c = ptm::qnan();
        return;
    }
    float fn = __builtin_rintf(x * 0.6366197466850281f);
    int n = (int)fn;
    float r = ptm::fma(fn, -1.5707963705062866f, x);
    r = ptm::fma(fn, 4.371138828673793e-08f, r);
    float z = r * r;
    float sp = ptm::fma(ptm::fma(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    sp = ptm::fma(sp * z, r, r);
    float cp = ptm::fma(ptm::fma(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    cp = ptm::fma(cp * z, z, ptm::fma(-0.5f, z, 1.0f));
    float ss = (n & 1) ? cp : sp;
    float cc = (n & 1) ? sp : cp;
    s = (n & 2) ? -ss : ss;
    c = ((n + 1) & 2) ? -cc : cc;
}

template <int kF>
__device__ __forceinline__ uint32_t evalUnary(uint32_t pattern) {
    const float x = ptm::u2f(pattern);
    float s = 0.0f, c = 0.0f;
    if constexpr (kF == kSin) { ptm::sincos(x, s, c); return ptm::f2u(s); }
    if constexpr (kF == kCos) { ptm::sincos(x, s, c); return ptm::f2u(c); }
    if constexpr (kF == kTan) return ptm::f2u(ptm::tan(x));
    if constexpr (kF == kAtan) return ptm::f2u(ptm::atan(x));
    if constexpr (kF == kLog) return ptm::f2u(ptm::log(x));
    if constexpr (kF == kExp) return ptm::f2u(ptm::exp(x));
    if constexpr (kF == kPowGamma) return ptm::f2u(ptm::pow(x, ptm::kGamma));
    if constexpr (kF == kQuantize) return ptq::quantize_literal(x);
    if constexpr (kF == kExpHardware) return ptm::f2u(__builtin_amdgcn_exp2f(x * 1.4426950f));
    if constexpr (kF == kSinTwoStep) { sincosTwoStep(x, s, c); return ptm::f2u(s); }
    if constexpr (kF == kCosTwoStep) { sincosTwoStep(x, s, c); return ptm::f2u(c); }
    return 0u;
}

// thread i of the chunk: pattern first + i
template <int kF>
__global__ void sortedKernel(uint32_t first, uint32_t n, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = evalUnary<kF>(first + i);
}
// thread t of ALL 2^32: pattern t * kScatter, evaluated by every lane; kept where it lies in [first, first + n). The grid is
// (2^23, 2) blocks of 256 — one dimension may not span 2^32 threads — and blockIdx.y is bit 31 of t.
template <int kF>
__global__ void scatteredKernel(uint32_t first, uint32_t n, uint32_t* out) {
    const uint32_t t = (blockIdx.y << 31) | (blockIdx.x * blockDim.x + threadIdx.x);
    const uint32_t pattern = t * kScatter;
    const uint32_t result = evalUnary<kF>(pattern);
    const uint32_t k = pattern - first;
    if (k < n) out[k] = result;
}

// pair k of the grid: x = gx[k / ny], y = gy[k % ny]. sorted: thread t takes pair t. scattered: pair t * kScatter mod pairs.
__global__ void powGridKernel(const float* gx, const float* gy, uint32_t ny, uint32_t pairs, int scattered, uint32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= pairs) return;
    const uint32_t k = scattered ? (uint32_t)(((unsigned long long)t * kScatter) % pairs) : t;
    out[k] = ptm::f2u(ptm::pow(gx[k / ny], gy[k % ny]));
}

// case t: kIn floats in, kOut words out (the host laid the cases out in the order under test)
__global__ void vectorKernel(int op, const float* in, uint32_t cases, uint32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cases) return;
    float a[ptvecops::kIn], r[ptvecops::kOut];
    for (int k = 0; k < ptvecops::kIn; ++k) a[k] = in[(size_t)t * ptvecops::kIn + k];
    ptvecops::apply(op, a, r);
    for (int k = 0; k < ptvecops::kOut; ++k) out[(size_t)t * ptvecops::kOut + k] = ptm::f2u(r[k]);
}
// control: dot as a sum of three products, each rounded, without the fma chain
__global__ void plainDotKernel(const float* in, uint32_t cases, uint32_t* out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cases) return;
    const float* a = in + (size_t)t * ptvecops::kIn;
    out[(size_t)t * ptvecops::kOut] = ptm::f2u(a[0] * a[3] + a[1] * a[4] + a[2] * a[5]);
    for (int k = 1; k < ptvecops::kOut; ++k) out[(size_t)t * ptvecops::kOut + k] = 0u;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
float u2f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
uint32_t f2u(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
bool isNan(uint32_t w) { return (w & 0x7fffffffu) > 0x7f800000u; }
bool sameWord(uint32_t a, uint32_t b, bool floats) { return a == b || (floats && isNan(a) && isNan(b)); }

unsigned threadCount() { return std::max(1u, std::min(16u, std::thread::hardware_concurrency())); }

// f(begin, end) over [0, total) in contiguous slices, one per thread
void parallelFor(size_t total, const std::function<void(size_t, size_t)>& f) {
    const unsigned threads = threadCount();
    std::vector<std::thread> pool;
    for (unsigned k = 0; k < threads; ++k) {
        const size_t begin = total * k / threads, end = total * (k + 1) / threads;
        if (begin < end) pool.emplace_back(f, begin, end);
    }
    for (std::thread& t : pool) t.join();
}

struct Column {
    unsigned long long checked = 0, mismatch = 0;
    unsigned long long first = ~0ull;
    uint32_t device = 0, host = 0;
    void add(unsigned long long index, uint32_t dev, uint32_t hst) {
        ++mismatch;
        if (index < first) { first = index; device = dev; host = hst; }
    }
    void merge(const Column& o) {
        checked += o.checked;
        mismatch += o.mismatch;
        if (o.first < first) { first = o.first; device = o.device; host = o.host; }
    }
    void print(const char* op, const char* name) const {
        if (strncmp(name, "control_", 8) == 0) printf("%s %s checked=%llu mismatch=%llu\n", op, name, checked, mismatch);
        else printf("%s %s checked=%llu mismatch=%llu first=0x%08llx device=0x%08x host=0x%08x\n", op, name, checked, mismatch,
                    mismatch ? first : 0ull, device, host);
        fflush(stdout);
    }
};

void probeFailed(const char* what) {
    printf("%s refused its arguments\n", what);
    fflush(stdout);
    exit(2);
}

using Launch = void (*)(uint32_t first, uint32_t n, uint32_t* out);
template <int kF> void launchSorted(uint32_t first, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(sortedKernel<kF>, dim3(n / 256u), dim3(256), 0, 0, first, n, out);
}
template <int kF> void launchScattered(uint32_t first, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(scatteredKernel<kF>, dim3(1u << 23, 2), dim3(256), 0, 0, first, n, out);
}

struct UnaryOp {
    const char* name;
    int probeOp;           // of ptss_probe_math; -1: ptss_probe_quantize
    bool gamma;            // y = kGamma
    Launch sorted, scattered;
    const char* controlName;
    Launch control;        // sorted order, held against the same host values
};
const UnaryOp kUnary[] = {
    {"sin", 0, false, launchSorted<kSin>, launchScattered<kSin>, "control_two_step_reduction", launchSorted<kSinTwoStep>},
    {"cos", 1, false, launchSorted<kCos>, launchScattered<kCos>, "control_two_step_reduction", launchSorted<kCosTwoStep>},
    {"tan", 2, false, launchSorted<kTan>, launchScattered<kTan>, nullptr, nullptr},
    {"atan", 3, false, launchSorted<kAtan>, launchScattered<kAtan>, nullptr, nullptr},
    {"log", 4, false, launchSorted<kLog>, launchScattered<kLog>, nullptr, nullptr},
    {"exp", 5, false, launchSorted<kExp>, launchScattered<kExp>, "control_hardware_exp2", launchSorted<kExpHardware>},
    {"pow_gamma", 6, true, launchSorted<kPowGamma>, launchScattered<kPowGamma>, nullptr, nullptr},
    {"quantize", -1, false, launchSorted<kQuantize>, launchScattered<kQuantize>, nullptr, nullptr},
};

struct Orders { bool sorted, scattered; };

bool runUnary(const UnaryOp& op, Orders orders) {   // true: a mismatch
    const auto t0 = std::chrono::steady_clock::now();
    const bool floats = op.probeOp >= 0;
    uint32_t *dSorted = nullptr, *dScattered = nullptr, *dControl = nullptr;      // device
    uint32_t *hSorted = nullptr, *hScattered = nullptr, *hControl = nullptr;      // pinned host copies
    const size_t bytes = (size_t)kChunk * sizeof(uint32_t);
    if (orders.sorted) { HIP_OK(hipMalloc(&dSorted, bytes)); HIP_OK(hipHostMalloc(&hSorted, bytes)); }
    if (orders.scattered) { HIP_OK(hipMalloc(&dScattered, bytes)); HIP_OK(hipHostMalloc(&hScattered, bytes)); }
    if (op.control) { HIP_OK(hipMalloc(&dControl, bytes)); HIP_OK(hipHostMalloc(&hControl, bytes)); }
    Column sorted, scattered, control;
    std::mutex merge;
    double deviceSeconds = 0;
    for (uint32_t chunk = 0; chunk < (1ull << 32) / kChunk; ++chunk) {
        const uint32_t first = chunk * kChunk;
        const auto d0 = std::chrono::steady_clock::now();
        if (orders.sorted) { op.sorted(first, kChunk, dSorted); HIP_OK(hipGetLastError()); }
        if (orders.scattered) {
            HIP_OK(hipMemset(dScattered, 0xa5, bytes));   // (a pattern no thread wrote would show as a mismatch)
            op.scattered(first, kChunk, dScattered);
            HIP_OK(hipGetLastError());
        }
        if (op.control) { op.control(first, kChunk, dControl); HIP_OK(hipGetLastError()); }
        HIP_OK(hipDeviceSynchronize());
        deviceSeconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count();
        if (orders.sorted) HIP_OK(hipMemcpy(hSorted, dSorted, bytes, hipMemcpyDeviceToHost));
        if (orders.scattered) HIP_OK(hipMemcpy(hScattered, dScattered, bytes, hipMemcpyDeviceToHost));
        if (op.control) HIP_OK(hipMemcpy(hControl, dControl, bytes, hipMemcpyDeviceToHost));
        parallelFor(kChunk, [&](size_t begin, size_t end) {
            std::vector<float> x(kHostBlock), y(op.gamma ? kHostBlock : 0, ptm::kGamma), hf(kHostBlock);
            std::vector<unsigned int> hq(floats ? 0 : kHostBlock);
            Column s, c, k;
            for (size_t b = begin; b < end; b += kHostBlock) {
                const size_t m = std::min(kHostBlock, end - b);
                for (size_t i = 0; i < m; ++i) x[i] = u2f(first + (uint32_t)(b + i));
                if (floats) {
                    if (ptss_probe_math(op.probeOp, x.data(), op.gamma ? y.data() : nullptr, hf.data(), m) != 0) probeFailed("ptss_probe_math");
                } else if (ptss_probe_quantize(x.data(), hq.data(), m) != 0) {
                    probeFailed("ptss_probe_quantize");
                }
                for (size_t i = 0; i < m; ++i) {
                    const uint32_t pattern = first + (uint32_t)(b + i), h = floats ? f2u(hf[i]) : (uint32_t)hq[i];
                    if (hSorted && !sameWord(hSorted[b + i], h, floats)) s.add(pattern, hSorted[b + i], h);
                    if (hScattered && !sameWord(hScattered[b + i], h, floats)) c.add(pattern, hScattered[b + i], h);
                    if (hControl && !sameWord(hControl[b + i], h, floats)) k.add(pattern, hControl[b + i], h);
                }
                if (hSorted) s.checked += m;
                if (hScattered) c.checked += m;
                if (hControl) k.checked += m;
            }
            std::lock_guard<std::mutex> lock(merge);
            sorted.merge(s);
            scattered.merge(c);
            control.merge(k);
        });
        if ((chunk & 15u) == 15u) fprintf(stderr, "%s: %u / 64 chunks\n", op.name, chunk + 1u);   // progress
    }
    if (orders.sorted) sorted.print(op.name, "sorted");
    if (orders.scattered) scattered.print(op.name, "scattered");
    if (op.control) control.print(op.name, op.controlName);
    for (uint32_t* p : {dSorted, dScattered, dControl}) if (p) HIP_OK(hipFree(p));
    for (uint32_t* p : {hSorted, hScattered, hControl}) if (p) HIP_OK(hipHostFree(p));
    printf("%s seconds=%.1f device_seconds=%.1f host_threads=%u\n", op.name,
           std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), deviceSeconds, threadCount());
    return sorted.mismatch || scattered.mismatch;
}

// ---- pow(x, y) on a grid --------------------------------------------------------------------------------------------------------------
std::vector<float> powGrid(bool withPhong) {
    std::vector<uint32_t> mant = {0u, 0x7fffffu, 1u, 0x400000u, 0x7ffffeu, 2u, 0x000800u, 0x200000u};   // zero, all ones, one bit, ...
    uint32_t s = 0x2468aceu;
    while (mant.size() < 16) { s = s * 1664525u + 1013904223u; mant.push_back((s >> 9) & 0x7fffffu); }   // ... random
    std::vector<float> g;
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t e = 0; e < 256; ++e)
            for (uint32_t m : mant) g.push_back(u2f((sign << 31) | (e << 23) | m));
    const uint32_t specials[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u,   // +-0, +-inf, NaNs
                                 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00400000u,                               // denormals
                                 0x3f7fffffu, 0x3f800000u, 0x3f800001u, 0xbf7fffffu, 0xbf800000u, 0xbf800001u};                 // +-1 and neighbours
    for (uint32_t b : specials) g.push_back(u2f(b));
    if (withPhong)   // host/Scene.cpp's presets: Phong exponents 250 and 300, and infinity for the mirror-like lobes
        for (float e : {250.0f, 300.0f, u2f(0x7f800000u)}) g.push_back(1.0f / (e + 1.0f));
    return g;
}

bool runPowGrid(Orders orders) {
    const auto t0 = std::chrono::steady_clock::now();
    const std::vector<float> gx = powGrid(false), gy = powGrid(true);
    const uint32_t nx = (uint32_t)gx.size(), ny = (uint32_t)gy.size();
    const unsigned long long pairs64 = (unsigned long long)nx * ny;
    uint32_t a = kScatter, b = (uint32_t)pairs64;
    while (b) { const uint32_t r = a % b; a = b; b = r; }
    if (pairs64 >= (1ull << 28) || a != 1u) { printf("pow_grid: %llu pairs: too many, or not coprime to the multiplier\n", pairs64); exit(2); }
    const uint32_t pairs = (uint32_t)pairs64;
    printf("pow_grid grid x=%u y=%u pairs=%u\n", nx, ny, pairs);
    float *dx = nullptr, *dy = nullptr;
    uint32_t* dOut = nullptr;
    HIP_OK(hipMalloc(&dx, nx * sizeof(float)));
    HIP_OK(hipMalloc(&dy, ny * sizeof(float)));
    HIP_OK(hipMalloc(&dOut, (size_t)pairs * sizeof(uint32_t)));
    HIP_OK(hipMemcpy(dx, gx.data(), nx * sizeof(float), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dy, gy.data(), ny * sizeof(float), hipMemcpyHostToDevice));
    std::vector<uint32_t> device[2];
    for (int scattered = 0; scattered < 2; ++scattered) {
        if (!(scattered ? orders.scattered : orders.sorted)) continue;
        HIP_OK(hipMemset(dOut, 0xa5, (size_t)pairs * sizeof(uint32_t)));
        hipLaunchKernelGGL(powGridKernel, dim3((pairs + 255u) / 256u), dim3(256), 0, 0, dx, dy, ny, pairs, scattered, dOut);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        device[scattered].resize(pairs);
        HIP_OK(hipMemcpy(device[scattered].data(), dOut, (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    HIP_OK(hipFree(dx));
    HIP_OK(hipFree(dy));
    HIP_OK(hipFree(dOut));
    Column column[2];
    std::mutex merge;
    parallelFor(pairs, [&](size_t begin, size_t end) {
        std::vector<float> x(kHostBlock), y(kHostBlock), h(kHostBlock);
        Column mine[2];
        for (size_t blk = begin; blk < end; blk += kHostBlock) {
            const size_t m = std::min(kHostBlock, end - blk);
            for (size_t i = 0; i < m; ++i) { x[i] = gx[(blk + i) / ny]; y[i] = gy[(blk + i) % ny]; }
            if (ptss_probe_math(6, x.data(), y.data(), h.data(), m) != 0) probeFailed("ptss_probe_math");
            for (int o = 0; o < 2; ++o) {
                if (device[o].empty()) continue;
                for (size_t i = 0; i < m; ++i)
                    if (!sameWord(device[o][blk + i], f2u(h[i]), true)) mine[o].add(blk + i, device[o][blk + i], f2u(h[i]));
                mine[o].checked += m;
            }
        }
        std::lock_guard<std::mutex> lock(merge);
        column[0].merge(mine[0]);
        column[1].merge(mine[1]);
    });
    if (orders.sorted) column[0].print("pow_grid", "sorted");
    if (orders.scattered) column[1].print("pow_grid", "scattered");
    printf("pow_grid seconds=%.1f host_threads=%u\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), threadCount());
    return column[0].mismatch || column[1].mismatch;
}

// ---- the vector layer -----------------------------------------------------------------------------------------------------------------
const char* kVectorNames[ptvecops::kOps] = {"dot", "cross", "div_scalar", "madd_scalar", "madd_vector", "rotate", "quat_mul", "normalize_vec3",
                                            "normalize_quat", "length"};
constexpr uint32_t kVectorReps = 64;

// the component list of guards_device.hip: every exponent x both signs x 64 mantissas (+-0, denormals, infinities and NaNs among
// them) and the values within two ulps of the ends of the fast ranges of sqrt, rcp and div
std::vector<float> components() {
    std::vector<uint32_t> mant = {0u, 1u, 0x7fffffu, 0x7ffffeu, 0x400000u};
    uint32_t s = 0x1234567u;
    while (mant.size() < 64) { s = s * 1664525u + 1013904223u; mant.push_back((s >> 9) & 0x7fffffu); }
    std::vector<float> v;
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t e = 0; e < 256; ++e)
            for (uint32_t m : mant) v.push_back(u2f((sign << 31) | (e << 23) | m));
    const float ends[] = {ptm::kSqrtLo, ptm::kSqrtHi, ptm::kRcpLo, ptm::kRcpHi, ptm::kDivLo, ptm::kDivHi};
    for (float e : ends)
        for (int d = -2; d <= 2; ++d)
            for (uint32_t sign = 0; sign < 2; ++sign) v.push_back(u2f((f2u(e) + (uint32_t)d) | (sign << 31)));
    return v;
}

uint32_t pickIndex(uint32_t n, uint32_t i, uint32_t salt) {   // guards_device.hip's pick()
    uint32_t h = (i + 1u) * 2654435761u ^ (salt * 0x9e3779b9u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    return h % n;
}

// case t = (operand i, repetition rep) as guards_device.hip combines them. sorted: the other components are the operand's neighbours
// in the list (same or adjacent exponent), so a wave is of one kind; scattered: every component from anywhere in the list.
std::vector<float> vectorCases(const std::vector<float>& v, bool scattered) {
    const uint32_t n = (uint32_t)v.size();
    std::vector<float> in((size_t)n * kVectorReps * ptvecops::kIn);
    for (uint32_t t = 0; t < n * kVectorReps; ++t) {
        uint32_t i = t / kVectorReps;
        const uint32_t rep = t % kVectorReps;
        if (scattered) i = (uint32_t)(((unsigned long long)i * 40503ull + 12345ull * rep) % n);
        float* c = &in[(size_t)t * ptvecops::kIn];
        c[0] = v[i];
        for (uint32_t k = 1; k < (uint32_t)ptvecops::kIn; ++k) c[k] = scattered ? v[pickIndex(n, t, k)] : v[(i + k + (2u * k - 1u) * rep) % n];
    }
    return in;
}

bool runVector(int op, Orders orders) {
    const std::vector<float> v = components();
    const uint32_t cases = (uint32_t)v.size() * kVectorReps;
    float* dIn = nullptr;
    uint32_t* dOut = nullptr;
    HIP_OK(hipMalloc(&dIn, (size_t)cases * ptvecops::kIn * sizeof(float)));
    HIP_OK(hipMalloc(&dOut, (size_t)cases * ptvecops::kOut * sizeof(uint32_t)));
    bool bad = false;
    Column control;
    for (int scattered = 0; scattered < 2; ++scattered) {
        if (!(scattered ? orders.scattered : orders.sorted)) continue;
        const std::vector<float> in = vectorCases(v, scattered != 0);
        HIP_OK(hipMemcpy(dIn, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
        std::vector<uint32_t> device((size_t)cases * ptvecops::kOut), plain;
        hipLaunchKernelGGL(vectorKernel, dim3((cases + 255u) / 256u), dim3(256), 0, 0, op, dIn, cases, dOut);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(device.data(), dOut, device.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (op == 0) {
            plain.resize(device.size());
            hipLaunchKernelGGL(plainDotKernel, dim3((cases + 255u) / 256u), dim3(256), 0, 0, dIn, cases, dOut);
            HIP_OK(hipGetLastError());
            HIP_OK(hipDeviceSynchronize());
            HIP_OK(hipMemcpy(plain.data(), dOut, plain.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        std::vector<float> host((size_t)cases * ptvecops::kOut);
        parallelFor(cases, [&](size_t begin, size_t end) {
            if (ptss_probe_vector(op, &in[begin * ptvecops::kIn], &host[begin * ptvecops::kOut], end - begin) != 0) probeFailed("ptss_probe_vector");
        });
        Column column;
        for (uint32_t t = 0; t < cases; ++t) {
            for (int k = 0; k < ptvecops::kOut; ++k) {
                const size_t w = (size_t)t * ptvecops::kOut + k;
                if (!sameWord(device[w], f2u(host[w]), true)) { column.add(t, device[w], f2u(host[w])); break; }
            }
            if (op == 0 && !sameWord(plain[(size_t)t * ptvecops::kOut], f2u(host[(size_t)t * ptvecops::kOut]), true)) control.add(t, 0u, 0u);
        }
        column.checked = cases;
        if (op == 0) control.checked += cases;
        column.print(kVectorNames[op], scattered ? "scattered" : "sorted");
        bad = bad || column.mismatch != 0;
    }
    if (op == 0) control.print(kVectorNames[op], "control_without_fma_chain");
    HIP_OK(hipFree(dIn));
    HIP_OK(hipFree(dOut));
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    const char* only = argc > 1 ? argv[1] : nullptr;
    Orders orders{true, true};
    if (argc > 2) {
        if (strcmp(argv[2], "sorted") == 0) orders.scattered = false;
        else if (strcmp(argv[2], "scattered") == 0) orders.sorted = false;
        else if (strcmp(argv[2], "both") != 0) { printf("usage: ptss_identitycheck [op [sorted|scattered|both]]\n"); return 2; }
    }
    int deviceCount = 0;
    HIP_OK(hipGetDeviceCount(&deviceCount));
    if (deviceCount < 1) { printf("no device\n"); return 2; }
    bool ran = false, bad = false;
    for (const UnaryOp& op : kUnary)
        if (!only || strcmp(only, op.name) == 0) { bad = runUnary(op, orders) || bad; ran = true; }
    if (!only || strcmp(only, "pow_grid") == 0) { bad = runPowGrid(orders) || bad; ran = true; }
    for (int op = 0; op < ptvecops::kOps; ++op)
        if (!only || strcmp(only, kVectorNames[op]) == 0) { bad = runVector(op, orders) || bad; ran = true; }
    if (!ran) { printf("unknown operation %s\n", only); return 2; }
    return bad ? 1 : 0;
}
