// math_accuracy.cpp — the worst case of every ptm:: transcendental (csrc/ptmath.h) against float64 libm, by exhaustion over every
// finite float32 pattern of the function's domain. A tool, not a test: tests/test_ptmath.py adds the patterns it reports to its
// samples and cites the figures kept under profiles/math_accuracy/.
//
// Error unit (the definition of tests/test_ptmath.py's ulp_err): |got - ref| / spacing(|RN32(ref)|), ref = the float64 libm value
// of the float32 argument, spacing(a) = the distance from a to the next float32 above it. Ties go to the smaller bit pattern, so the
// output does not depend on the number of threads.
//
// build (the flags are CPU_FLAGS of cuda-path-tracer-ss_amd/build.py, plus OpenMP):
//   g++ -O2 -std=c++17 -mfma -mavx2 -ffp-contract=off -fno-fast-math -fopenmp -I include -I cuda-path-tracer-ss_amd/csrc
//       tools/math_accuracy.cpp -o math_accuracy
// run:  ./math_accuracy > profiles/math_accuracy/worst_cases.txt      (minutes; every core)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ptmath.h"

namespace {

struct Worst {
    unsigned long long count = 0;
    double ulp = -1.0;
    uint32_t pattern = 0;
    void take(double e, uint32_t p) {
        ++count;
        if (!(e == e)) e = INFINITY;   // a NaN where libm has a number must not pass unseen
        if (e > ulp || (e == ulp && p < pattern)) {
            ulp = e;
            pattern = p;
        }
    }
    void merge(const Worst& o) {
        count += o.count;
        if (o.ulp > ulp || (o.ulp == ulp && o.pattern < pattern)) {
            ulp = o.ulp;
            pattern = o.pattern;
        }
    }
};

double ulpError(float got, double ref) {
    const float a = fabsf((float)ref);
    const double spacing = (double)nextafterf(a, INFINITY) - (double)a;
    return fabs((double)got - ref) / spacing;
}

enum Row { kSin2Pi, kSin1e4, kCos2Pi, kCos1e4, kTan2Pi, kTan1e4, kAtan, kLog, kExp, kRows };
const char* kFunction[kRows] = {"sin", "sin", "cos", "cos", "tan", "tan", "atan", "log", "exp"};
const char* kDomain[kRows] = {"|x|<=2pi", "|x|<=1e4", "|x|<=2pi", "|x|<=1e4", "|x|<=2pi", "|x|<=1e4", "finite", "0<x<inf", "-87.3<=x<=88.7"};

void measure(uint32_t p, Worst* w) {
    const float x = ptm::u2f(p);
    if (!(ptm::abs(x) < ptm::inf())) return;   // finite patterns only
    const double xd = (double)x;
    if (ptm::abs(x) <= 1.0e4f) {
        float s, c;
        ptm::sincos(x, s, c);
        const float t = ptm::tan(x);
        const double es = ulpError(s, sin(xd)), ec = ulpError(c, cos(xd)), et = ulpError(t, tan(xd));
        w[kSin1e4].take(es, p);
        w[kCos1e4].take(ec, p);
        w[kTan1e4].take(et, p);
        if (fabs(xd) <= 2.0 * M_PI) {
            w[kSin2Pi].take(es, p);
            w[kCos2Pi].take(ec, p);
            w[kTan2Pi].take(et, p);
        }
    }
    w[kAtan].take(ulpError(ptm::atan(x), atan(xd)), p);
    if (x > 0.0f) w[kLog].take(ulpError(ptm::log(x), log(xd)), p);
    if (x >= -87.3f && x <= 88.7f) w[kExp].take(ulpError(ptm::exp(x), exp(xd)), p);
}

}  // namespace

int main() {
    Worst total[kRows];
#pragma omp parallel
    {
        Worst mine[kRows];
#pragma omp for schedule(dynamic, 1)
        for (long long block = 0; block < 4096; ++block)   // 2^20 patterns per block
            for (uint32_t k = 0; k < (1u << 20); ++k) measure(((uint32_t)block << 20) | k, mine);
#pragma omp critical
        for (int r = 0; r < kRows; ++r) total[r].merge(mine[r]);
    }
    printf("%-8s %-16s %12s %10s %12s\n", "function", "domain", "count", "worst_ulp", "at_pattern");
    for (int r = 0; r < kRows; ++r)
        printf("%-8s %-16s %12llu %10.3f   0x%08x\n", kFunction[r], kDomain[r], total[r].count, total[r].ulp, total[r].pattern);
    return 0;
}
