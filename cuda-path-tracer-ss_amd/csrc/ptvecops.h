// ptvecops.h — the vector layer of ptmath.h by number: ONE statement of which ptv:: function an operation code calls and where its
// operands and results lie, shared by the host probe (ptss_probe_vector, host/host_capi.cpp) and the device side of the identity check
// (tests/csrc/math_identity.hip). Both compile this very switch, so a difference between their results is a difference between the
// two compilations of the functions themselves. Tests only; no kernel of the product includes it.
//
// One case reads kIn floats and writes kOut floats (results the operation does not have are written as +0):
//   op                 in                                         out
//   0 dot              a = in[0..2], b = in[3..5]                 dot(a, b)
//   1 cross            a = in[0..2], b = in[3..5]                 cross(a, b)
//   2 div_scalar       a = in[0..2], s = in[3]                    a / s
//   3 madd_scalar      v = in[0..2], s = in[3], o = in[4..6]      madd(v, s, o)
//   4 madd_vector      a = in[0..2], b = in[3..5], o = in[6..8]   madd(a, b, o)
//   5 rotate           q = in[0..3] (x, y, z, w), v = in[4..6]    rotate(q, v)
//   6 quat_mul         p = in[0..3], q = in[4..7]                 mul(p, q) as x, y, z, w
//   7 normalize_vec3   v = in[0..2]                               normalize(v)
//   8 normalize_quat   q = in[0..3]                               normalize(q) as x, y, z, w
//   9 length           v = in[0..2]                               length(v)
#ifndef PTSS_PTVECOPS_H
#define PTSS_PTVECOPS_H
#include "ptmath.h"

namespace ptvecops {

constexpr int kIn = 12, kOut = 4, kOps = 10;

PTM_HD void apply(int op, const float* in, float* out) {
    using namespace ptv;
    const vec3 a = v3(in[0], in[1], in[2]), b = v3(in[3], in[4], in[5]);
    const quat p = quat{in[0], in[1], in[2], in[3]};
    vec3 r = v3(0.0f);
    float w = 0.0f;
    switch (op) {
        case 0: r.x = dot(a, b); break;
        case 1: r = cross(a, b); break;
        case 2: r = a / in[3]; break;
        case 3: r = madd(a, in[3], v3(in[4], in[5], in[6])); break;
        case 4: r = madd(a, b, v3(in[6], in[7], in[8])); break;
        case 5: r = rotate(p, v3(in[4], in[5], in[6])); break;
        case 6: {
            const quat m = mul(p, quat{in[4], in[5], in[6], in[7]});
            r = v3(m.x, m.y, m.z);
            w = m.w;
            break;
        }
        case 7: r = normalize(a); break;
        case 8: {
            const quat m = normalize(p);
            r = v3(m.x, m.y, m.z);
            w = m.w;
            break;
        }
        default: r.x = length(a); break;
    }
    out[0] = r.x;
    out[1] = r.y;
    out[2] = r.z;
    out[3] = w;
}

}  // namespace ptvecops
#endif
