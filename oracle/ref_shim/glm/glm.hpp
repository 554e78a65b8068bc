// glm/glm.hpp — this repository's own stand-in for the part of glm 0.9.5 that the reference includes (TEST INFRASTRUCTURE).
//
// It lets the reference's own headers and sources compile with g++ into oracle/_ref/libref_probe.so (oracle/build.py build_ref).
// Written from glm's documented definitions (the GLSL specification's for the common functions), in plain float arithmetic: one
// rounding per operation, sums left to right, no fma. THIS FILE IS OURS: it is the one thing between the tests and the literal
// reference, so what the tests pin is "the reference's text over this glm", not "the reference over glm 0.9.5's binaries".
//
// Holds only what the reference uses: vec3 (.x/.r ...), vec4, quat, mat3, mat4, dot, cross, length, clamp, min, max, normalize,
// quat * vec3, quat * quat, quat(euler), translate, scale, rotate (degrees), inverse, transpose, mat4 * vec4, mediump_float.
#pragma once
#include <cmath>

namespace glm {

typedef float mediump_float;

struct vec4;

struct vec3 {
    union { float x, r; };
    union { float y, g; };
    union { float z, b; };
    vec3() {}
    explicit vec3(float s) : x(s), y(s), z(s) {}
    template <class A, class B, class C>
    vec3(A a, B b_, C c) : x((float)a), y((float)b_), z((float)c) {}
    explicit vec3(const vec4& v);
    float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    const float& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
    vec3& operator+=(const vec3& o) { x += o.x; y += o.y; z += o.z; return *this; }
    vec3& operator-=(const vec3& o) { x -= o.x; y -= o.y; z -= o.z; return *this; }
    vec3& operator*=(const vec3& o) { x *= o.x; y *= o.y; z *= o.z; return *this; }
    vec3& operator*=(float s) { x *= s; y *= s; z *= s; return *this; }
};

inline vec3 operator+(const vec3& a, const vec3& b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3& a, const vec3& b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3& a, const vec3& b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(const vec3& a, const vec3& b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator*(const vec3& a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator*(float s, const vec3& a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(const vec3& a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator-(const vec3& a) { return vec3(-a.x, -a.y, -a.z); }

struct vec4 {
    union { float x, r; };
    union { float y, g; };
    union { float z, b; };
    union { float w, a; };
    vec4() {}
    template <class A, class B, class C, class D>
    vec4(A a_, B b_, C c, D d) : x((float)a_), y((float)b_), z((float)c), w((float)d) {}
    float& operator[](int i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    const float& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
};
inline vec3::vec3(const vec4& v) : x(v.x), y(v.y), z(v.z) {}

inline vec4 operator+(const vec4& a, const vec4& b) { return vec4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
inline vec4 operator*(const vec4& a, float s) { return vec4(a.x * s, a.y * s, a.z * s, a.w * s); }

// ---- common and geometric functions (GLSL 4.x §8.3, §8.5) -----------------------------------------
template <class T> inline T min(T x, T y) { return y < x ? y : x; }   // "y if y < x, otherwise x"
template <class T> inline T max(T x, T y) { return x < y ? y : x; }   // "y if x < y, otherwise x"
template <class T> inline T clamp(T x, T lo, T hi) { return glm::min(glm::max(x, lo), hi); }
inline vec3 clamp(const vec3& v, float lo, float hi) { return vec3(clamp(v.x, lo, hi), clamp(v.y, lo, hi), clamp(v.z, lo, hi)); }

inline float dot(const vec3& a, const vec3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline vec3 cross(const vec3& a, const vec3& b) {
    return vec3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y);
}
inline float length(const vec3& v) { return std::sqrt(dot(v, v)); }
inline float inversesqrt(float x) { return 1.0f / std::sqrt(x); }
inline vec3 normalize(const vec3& v) { return v * inversesqrt(dot(v, v)); }
inline float radians(float degrees) { return degrees * 0.01745329251994329576923690768489f; }

// ---- quaternion: constructed (w, x, y, z), stored x, y, z, w; the default is the identity ------------
struct quat {
    float x, y, z, w;
    quat() : x(0), y(0), z(0), w(1) {}
    quat(float w_, float x_, float y_, float z_) : x(x_), y(y_), z(z_), w(w_) {}
    explicit quat(const vec3& euler) {   // pitch (x), yaw (y), roll (z), in radians
        const vec3 c(std::cos(euler.x * 0.5f), std::cos(euler.y * 0.5f), std::cos(euler.z * 0.5f));
        const vec3 s(std::sin(euler.x * 0.5f), std::sin(euler.y * 0.5f), std::sin(euler.z * 0.5f));
        w = c.x * c.y * c.z + s.x * s.y * s.z;
        x = s.x * c.y * c.z - c.x * s.y * s.z;
        y = c.x * s.y * c.z + s.x * c.y * s.z;
        z = c.x * c.y * s.z - s.x * s.y * c.z;
    }
};
inline float dot(const quat& a, const quat& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
inline float length(const quat& q) { return std::sqrt(dot(q, q)); }
inline quat normalize(const quat& q) {
    const float len = length(q);
    if (len <= 0.0f) return quat(1, 0, 0, 0);
    const float oneOverLen = 1.0f / len;
    return quat(q.w * oneOverLen, q.x * oneOverLen, q.y * oneOverLen, q.z * oneOverLen);
}
inline quat operator*(const quat& p, const quat& q) {   // Hamilton product
    return quat(p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z,
                p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
                p.w * q.y + p.y * q.w + p.z * q.x - p.x * q.z,
                p.w * q.z + p.z * q.w + p.x * q.y - p.y * q.x);
}
inline vec3 operator*(const quat& q, const vec3& v) {   // v + 2w (u x v) + 2 (u x (u x v)), u = (q.x, q.y, q.z)
    const vec3 u(q.x, q.y, q.z);
    vec3 uv = cross(u, v);
    vec3 uuv = cross(u, uv);
    uv *= (2.0f * q.w);
    uuv *= 2.0f;
    return v + uv + uuv;
}

// ---- matrices: column-major, m[c] is column c ---------------------------------------------------------
struct mat4 {
    vec4 col[4];
    mat4() : mat4(1.0f) {}
    explicit mat4(float d) {
        for (int c = 0; c < 4; ++c) col[c] = vec4(c == 0 ? d : 0.0f, c == 1 ? d : 0.0f, c == 2 ? d : 0.0f, c == 3 ? d : 0.0f);
    }
    vec4& operator[](int c) { return col[c]; }
    const vec4& operator[](int c) const { return col[c]; }
};
struct mat3 {
    vec3 col[3];
    vec3& operator[](int c) { return col[c]; }
    const vec3& operator[](int c) const { return col[c]; }
};

inline vec4 operator*(const mat4& m, const vec4& v) {
    return vec4(m[0][0] * v.x + m[1][0] * v.y + m[2][0] * v.z + m[3][0] * v.w,
                m[0][1] * v.x + m[1][1] * v.y + m[2][1] * v.z + m[3][1] * v.w,
                m[0][2] * v.x + m[1][2] * v.y + m[2][2] * v.z + m[3][2] * v.w,
                m[0][3] * v.x + m[1][3] * v.y + m[2][3] * v.z + m[3][3] * v.w);
}
inline mat4 operator*(const mat4& a, const mat4& b) {
    mat4 r(0.0f);
    for (int c = 0; c < 4; ++c) r[c] = a[0] * b[c][0] + a[1] * b[c][1] + a[2] * b[c][2] + a[3] * b[c][3];
    return r;
}
inline mat4 transpose(const mat4& m) {
    mat4 r(0.0f);
    for (int c = 0; c < 4; ++c)
        for (int k = 0; k < 4; ++k) r[c][k] = m[k][c];
    return r;
}
// inverse = adjugate / determinant (cofactors from the 2x2 minors of the lower two rows)
inline mat4 inverse(const mat4& m) {
    const float a00 = m[0][0], a01 = m[0][1], a02 = m[0][2], a03 = m[0][3];
    const float a10 = m[1][0], a11 = m[1][1], a12 = m[1][2], a13 = m[1][3];
    const float a20 = m[2][0], a21 = m[2][1], a22 = m[2][2], a23 = m[2][3];
    const float a30 = m[3][0], a31 = m[3][1], a32 = m[3][2], a33 = m[3][3];
    const float b00 = a00 * a11 - a01 * a10, b01 = a00 * a12 - a02 * a10, b02 = a00 * a13 - a03 * a10;
    const float b03 = a01 * a12 - a02 * a11, b04 = a01 * a13 - a03 * a11, b05 = a02 * a13 - a03 * a12;
    const float b06 = a20 * a31 - a21 * a30, b07 = a20 * a32 - a22 * a30, b08 = a20 * a33 - a23 * a30;
    const float b09 = a21 * a32 - a22 * a31, b10 = a21 * a33 - a23 * a31, b11 = a22 * a33 - a23 * a32;
    const float det = b00 * b11 - b01 * b10 + b02 * b09 + b03 * b08 - b04 * b07 + b05 * b06;
    const float inv = 1.0f / det;
    mat4 r(0.0f);
    r[0] = vec4((a11 * b11 - a12 * b10 + a13 * b09) * inv, (a02 * b10 - a01 * b11 - a03 * b09) * inv,
                (a31 * b05 - a32 * b04 + a33 * b03) * inv, (a22 * b04 - a21 * b05 - a23 * b03) * inv);
    r[1] = vec4((a12 * b08 - a10 * b11 - a13 * b07) * inv, (a00 * b11 - a02 * b08 + a03 * b07) * inv,
                (a32 * b02 - a30 * b05 - a33 * b01) * inv, (a20 * b05 - a22 * b02 + a23 * b01) * inv);
    r[2] = vec4((a10 * b10 - a11 * b08 + a13 * b06) * inv, (a01 * b08 - a00 * b10 - a03 * b06) * inv,
                (a30 * b04 - a31 * b02 + a33 * b00) * inv, (a21 * b02 - a20 * b04 - a23 * b00) * inv);
    r[3] = vec4((a11 * b07 - a10 * b09 - a12 * b06) * inv, (a00 * b09 - a01 * b07 + a02 * b06) * inv,
                (a31 * b01 - a30 * b03 - a32 * b00) * inv, (a20 * b03 - a21 * b01 + a22 * b00) * inv);
    return r;
}

// ---- gtx/transform: the one-argument forms act on the identity --------------------------------------
inline mat4 translate(const vec3& v) {
    const mat4 m(1.0f);
    mat4 r(m);
    r[3] = m[0] * v.x + m[1] * v.y + m[2] * v.z + m[3];
    return r;
}
inline mat4 scale(const vec3& v) {
    const mat4 m(1.0f);
    mat4 r(0.0f);
    r[0] = m[0] * v.x;
    r[1] = m[1] * v.y;
    r[2] = m[2] * v.z;
    r[3] = m[3];
    return r;
}
// the angle is in DEGREES: glm 0.9.5 without GLM_FORCE_RADIANS, which the reference does not define
inline mat4 rotate(float angle, const vec3& v) {
    const float a = radians(angle);
    const float c = std::cos(a), s = std::sin(a);
    const vec3 axis = normalize(v);
    const vec3 temp = (1.0f - c) * axis;
    mat4 rot(0.0f);
    rot[0][0] = c + temp[0] * axis[0];
    rot[0][1] = 0 + temp[0] * axis[1] + s * axis[2];
    rot[0][2] = 0 + temp[0] * axis[2] - s * axis[1];
    rot[1][0] = 0 + temp[1] * axis[0] - s * axis[2];
    rot[1][1] = c + temp[1] * axis[1];
    rot[1][2] = 0 + temp[1] * axis[2] + s * axis[0];
    rot[2][0] = 0 + temp[2] * axis[0] + s * axis[1];
    rot[2][1] = 0 + temp[2] * axis[1] - s * axis[0];
    rot[2][2] = c + temp[2] * axis[2];
    const mat4 m(1.0f);
    mat4 r(0.0f);
    r[0] = m[0] * rot[0][0] + m[1] * rot[0][1] + m[2] * rot[0][2];
    r[1] = m[0] * rot[1][0] + m[1] * rot[1][1] + m[2] * rot[1][2];
    r[2] = m[0] * rot[2][0] + m[1] * rot[2][1] + m[2] * rot[2][2];
    r[3] = m[3];
    return r;
}

}  // namespace glm
