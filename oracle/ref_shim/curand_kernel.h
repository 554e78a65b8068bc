// curand_kernel.h — this repository's own stand-in for cuRAND's device API (TEST INFRASTRUCTURE): curandState, curand_init,
// curand, curand_uniform for the XORWOW generator, from its published description: Marsaglia's xorwow with the Weyl increment
// 362437, cuRAND's seed scramble, and `sequence` skipping sequence * 2^67 draws of the xorshift part. Written apart from
// oracle/oracle.cpp's statement of the same generator; tests/test_reference_functions.py holds the two streams against each other
// (and tests/test_xorwow.py holds the oracle's against rocRAND's tables).
#pragma once
#include <cstdint>
#include <vector>

struct curandStateXORWOW {
    unsigned int d;
    unsigned int v[5];
};
typedef curandStateXORWOW curandState;

inline unsigned int curand(curandState* s) {
    const unsigned int t = s->v[0] ^ (s->v[0] >> 2);
    s->v[0] = s->v[1];
    s->v[1] = s->v[2];
    s->v[2] = s->v[3];
    s->v[3] = s->v[4];
    s->v[4] = (s->v[4] ^ (s->v[4] << 4)) ^ (t ^ (t << 1));
    s->d += 362437u;
    return s->v[4] + s->d;
}

// (0, 1]: x * 2^-32 + 2^-33
inline float curand_uniform(curandState* s) { return (float)curand(s) * 2.3283064365386963e-10f + (2.3283064365386963e-10f / 2.0f); }

namespace ref_xorwow {
// the xorshift step is linear over GF(2) on the 160 bits of v[]: a jump is a power of its matrix, kept as 160 rows of 160 bits
struct Matrix {
    uint32_t row[160][5];   // row[i] = image of unit vector i
};
inline void apply(const Matrix& m, unsigned int v[5]) {
    uint32_t out[5] = {0, 0, 0, 0, 0};
    for (int word = 0; word < 5; ++word)
        for (int bit = 0; bit < 32; ++bit)
            if (v[word] & (1u << bit))
                for (int k = 0; k < 5; ++k) out[k] ^= m.row[32 * word + bit][k];
    for (int k = 0; k < 5; ++k) v[k] = out[k];
}
inline void square(Matrix& m) {
    Matrix* next = new Matrix(m);
    for (int i = 0; i < 160; ++i) apply(m, next->row[i]);
    m = *next;
    delete next;
}
// jumps()[k] advances by 2^(67 + k) draws
inline const std::vector<Matrix>& jumps() {
    static const std::vector<Matrix> table = [] {
        std::vector<Matrix> t;
        Matrix m;
        for (int i = 0; i < 160; ++i) {
            curandState unit = {0, {0, 0, 0, 0, 0}};
            unit.v[i / 32] = 1u << (i % 32);
            (void)curand(&unit);
            for (int k = 0; k < 5; ++k) m.row[i][k] = unit.v[k];
        }
        for (int s = 0; s < 67; ++s) square(m);
        for (int k = 0; k < 64; ++k) {
            t.push_back(m);
            square(m);
        }
        return t;
    }();
    return table;
}
}  // namespace ref_xorwow

inline void curand_init(unsigned long long seed, unsigned long long sequence, unsigned long long offset, curandState* s) {
    const unsigned int lo = (unsigned int)seed ^ 0xaad26b49u;
    const unsigned int hi = (unsigned int)(seed >> 32) ^ 0xf7dcefddu;
    const unsigned int a = lo * 1099087573u;
    const unsigned int b = hi * 2591861531u;
    s->v[0] = 123456789u + a;
    s->v[1] = 362436069u ^ a;
    s->v[2] = 521288629u + b;
    s->v[3] = 88675123u ^ b;
    s->v[4] = 5783321u + a;
    s->d = 6615241u + b + a;
    const std::vector<ref_xorwow::Matrix>& j = ref_xorwow::jumps();
    for (int k = 0; k < 64; ++k)
        if ((sequence >> k) & 1ull) ref_xorwow::apply(j[k], s->v);
    for (unsigned long long i = 0; i < offset; ++i) (void)curand(s);   // the reference passes 0
}
