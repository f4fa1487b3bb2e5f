// rt_pose.h — a mesh's triangles under a node matrix (host and device, no HIP).
//
// rt_scene_pose_meshes (include/rt_hw.h) recomputes the records of a mesh from its object-space
// vertices and a 4 x 4 matrix M, exactly as the loader makes them when the glTF node carries M; the
// loader's triangle loop (rt_host.cpp load_gltf) calls this same text, so tests/test_loader.py pins
// it against the reference's own dumps.  M and NT are matrix4<double> in column storage
// (src/utils/matrix.h:8-43): element (row i, column j) is m[4 * j + i].
//   positions  multiply(M, (q, 1)) (matrix.h:66-72): four float accumulators from 0, every add done
//              in double and rounded to float; v0 = M q0, U = M q1 - v0 (a - b is a + (-b)),
//              V.x = (M q2).x - v0.x; V.y and V.z are the differences of once-rounded dots of q2 and q0
//              (dot_once: the four products added in double, rounded to float once) — the shipped
//              reference binary's SLP-vectorized loop (see rt_host.cpp m4_mul_vector_gcc's note)
//   normals    normal(multiplyVector(NT, n)) with x and y once-rounded, z rounded per add, w = 0
//   geometric  n = cross(U, V); area = 0.5f * length(n); normal(n) (primitive.cpp:77-84)
//   NT         inverse(transpose(M)), the cofactor inverse of matrix.h:88-217: each cofactor is six
//              signed triple products added left to right, det = m0 c0 + m1 c4 + m2 c8 + m3 c12,
//              every cofactor times 1.0 / det.  Host only, once per mesh; det == 0 has no NT.
// Every product and every add is one fp64 or fp32 operation: no fused multiply-add anywhere (what
// rt_refit.h says about fast-math flags holds here too; the device listing is checked once,
// DESIGN.md §5.25).  tri_tan and the texture coordinates do not depend on M: tangents stay in
// object space and the shading pass carries them with the mesh's NT (rt_path.h), which is why
// mesh_nt must follow a pose.
#pragma once
#include <cstdint>

#include "rt_libm.h"
#include "rt_vec.h"

namespace rtps {

constexpr int kRestWords = 18;      // a rest record: q0, q1, q2, n0, n1, n2 (object space)
constexpr int kRestDevWords = 20;   // on the device: padded to five 16-byte quads

// One component of multiply(mat, vector4f): rounded to float after every add.
RT_HD float dot_per_add(const double *m, int i, float x, float y, float z, float w) {
    float r = 0.f;
    r = (float)((double)r + m[i] * (double)x);
    r = (float)((double)r + m[4 + i] * (double)y);
    r = (float)((double)r + m[8 + i] * (double)z);
    r = (float)((double)r + m[12 + i] * (double)w);
    return r;
}

// The same component with the four products added in double and rounded once.
RT_HD float dot_once(const double *m, int i, float x, float y, float z, float w) {
    return (float)(m[i] * (double)x + m[4 + i] * (double)y + m[8 + i] * (double)z + m[12 + i] * (double)w);
}

RT_HD rtv::V3 mul_point(const double *m, rtv::V3 p) {
    return {dot_per_add(m, 0, p.x, p.y, p.z, 1.f), dot_per_add(m, 1, p.x, p.y, p.z, 1.f), dot_per_add(m, 2, p.x, p.y, p.z, 1.f)};
}

// multiplyVector as the reference binary computes it in the triangle loop: x, y once-rounded.
RT_HD rtv::V3 mul_vector_gcc(const double *m, rtv::V3 p) {
    return {dot_once(m, 0, p.x, p.y, p.z, 0.f), dot_once(m, 1, p.x, p.y, p.z, 0.f), dot_per_add(m, 2, p.x, p.y, p.z, 0.f)};
}

// v0, U, V of the triangle q0 q1 q2 under M.
RT_HD void positions(const double *M, rtv::V3 q0, rtv::V3 q1, rtv::V3 q2, rtv::V3 &v0, rtv::V3 &U, rtv::V3 &V) {
    v0 = mul_point(M, q0);
    const rtv::V3 p1 = mul_point(M, q1);
    const float x2 = dot_per_add(M, 0, q2.x, q2.y, q2.z, 1.f);
    const float y0 = dot_once(M, 1, q0.x, q0.y, q0.z, 1.f), z0 = dot_once(M, 2, q0.x, q0.y, q0.z, 1.f);
    const float y2 = dot_once(M, 1, q2.x, q2.y, q2.z, 1.f), z2 = dot_once(M, 2, q2.x, q2.y, q2.z, 1.f);
    U = rtv::sub(p1, v0);
    V = rtv::V3{x2 - v0.x, y2 - y0, z2 - z0};
}

RT_HD rtv::V3 shading_normal(const double *NT, rtv::V3 n) { return rtv::normal(mul_vector_gcc(NT, n)); }

// Primitive::get_geometric_normal (primitive.cpp:77-84).
RT_HD rtv::V3 geometric_normal(rtv::V3 U, rtv::V3 V, float &area) {
    const rtv::V3 n = rtv::cross(U, V);
    area = 0.5f * rtv::length(n);
    return rtv::normal(n);
}

// A whole record: rest (18 words) under M and NT into tri (12 words: v0, U, V, geometric normal)
// and the first nine words of tri_attr (the three shading normals).
RT_HD void pose_record(const double *M, const double *NT, const float *rest, float *tri, float *attr9) {
    rtv::V3 v0, U, V;
    positions(M, {rest[0], rest[1], rest[2]}, {rest[3], rest[4], rest[5]}, {rest[6], rest[7], rest[8]}, v0, U, V);
    float area;
    const rtv::V3 g = geometric_normal(U, V, area);
    tri[0] = v0.x, tri[1] = v0.y, tri[2] = v0.z;
    tri[3] = U.x, tri[4] = U.y, tri[5] = U.z;
    tri[6] = V.x, tri[7] = V.y, tri[8] = V.z;
    tri[9] = g.x, tri[10] = g.y, tri[11] = g.z;
    for (int v = 0; v < 3; ++v) {
        const rtv::V3 n = shading_normal(NT, {rest[9 + 3 * v], rest[10 + 3 * v], rest[11 + 3 * v]});
        attr9[3 * v] = n.x, attr9[3 * v + 1] = n.y, attr9[3 * v + 2] = n.z;
    }
}

// ---------------------------------------------------------------- host only: the normal transform
inline void transpose(const double *m, double *out) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = m[4 * j + i];
}

// Cofactor inverse (matrix.h:88-217).  The table lists (sign, a, b, c) for
// inv[k] = sum sign * m[a]*m[b]*m[c], summed left to right.  False (out untouched) where det == 0.
inline bool inverse(const double *m, double *out) {
    static const int8_t T[16][6][4] = {
        {{+1, 5, 10, 15}, {-1, 5, 11, 14}, {-1, 9, 6, 15}, {+1, 9, 7, 14}, {+1, 13, 6, 11}, {-1, 13, 7, 10}},
        {{-1, 1, 10, 15}, {+1, 1, 11, 14}, {+1, 9, 2, 15}, {-1, 9, 3, 14}, {-1, 13, 2, 11}, {+1, 13, 3, 10}},
        {{+1, 1, 6, 15}, {-1, 1, 7, 14}, {-1, 5, 2, 15}, {+1, 5, 3, 14}, {+1, 13, 2, 7}, {-1, 13, 3, 6}},
        {{-1, 1, 6, 11}, {+1, 1, 7, 10}, {+1, 5, 2, 11}, {-1, 5, 3, 10}, {-1, 9, 2, 7}, {+1, 9, 3, 6}},
        {{-1, 4, 10, 15}, {+1, 4, 11, 14}, {+1, 8, 6, 15}, {-1, 8, 7, 14}, {-1, 12, 6, 11}, {+1, 12, 7, 10}},
        {{+1, 0, 10, 15}, {-1, 0, 11, 14}, {-1, 8, 2, 15}, {+1, 8, 3, 14}, {+1, 12, 2, 11}, {-1, 12, 3, 10}},
        {{-1, 0, 6, 15}, {+1, 0, 7, 14}, {+1, 4, 2, 15}, {-1, 4, 3, 14}, {-1, 12, 2, 7}, {+1, 12, 3, 6}},
        {{+1, 0, 6, 11}, {-1, 0, 7, 10}, {-1, 4, 2, 11}, {+1, 4, 3, 10}, {+1, 8, 2, 7}, {-1, 8, 3, 6}},
        {{+1, 4, 9, 15}, {-1, 4, 11, 13}, {-1, 8, 5, 15}, {+1, 8, 7, 13}, {+1, 12, 5, 11}, {-1, 12, 7, 9}},
        {{-1, 0, 9, 15}, {+1, 0, 11, 13}, {+1, 8, 1, 15}, {-1, 8, 3, 13}, {-1, 12, 1, 11}, {+1, 12, 3, 9}},
        {{+1, 0, 5, 15}, {-1, 0, 7, 13}, {-1, 4, 1, 15}, {+1, 4, 3, 13}, {+1, 12, 1, 7}, {-1, 12, 3, 5}},
        {{-1, 0, 5, 11}, {+1, 0, 7, 9}, {+1, 4, 1, 11}, {-1, 4, 3, 9}, {-1, 8, 1, 7}, {+1, 8, 3, 5}},
        {{-1, 4, 9, 14}, {+1, 4, 10, 13}, {+1, 8, 5, 14}, {-1, 8, 6, 13}, {-1, 12, 5, 10}, {+1, 12, 6, 9}},
        {{+1, 0, 9, 14}, {-1, 0, 10, 13}, {-1, 8, 1, 14}, {+1, 8, 2, 13}, {+1, 12, 1, 10}, {-1, 12, 2, 9}},
        {{-1, 0, 5, 14}, {+1, 0, 6, 13}, {+1, 4, 1, 14}, {-1, 4, 2, 13}, {-1, 12, 1, 6}, {+1, 12, 2, 5}},
        {{+1, 0, 5, 10}, {-1, 0, 6, 9}, {-1, 4, 1, 10}, {+1, 4, 2, 9}, {+1, 8, 1, 6}, {-1, 8, 2, 5}},
    };
    double res[16];
    for (int k = 0; k < 16; ++k) {
        const int8_t(*t)[4] = T[k];
        double acc = (t[0][0] < 0 ? -m[t[0][1]] : m[t[0][1]]) * m[t[0][2]] * m[t[0][3]];
        for (int q = 1; q < 6; ++q) {
            double p = m[t[q][1]] * m[t[q][2]] * m[t[q][3]];
            acc = t[q][0] < 0 ? acc - p : acc + p;
        }
        res[k] = acc;
    }
    double det = m[0] * res[0] + m[1] * res[4] + m[2] * res[8] + m[3] * res[12];
    if (det == 0) return false;
    det = 1.0 / det;
    for (int i = 0; i < 16; ++i) out[i] = res[i] * det;
    return true;
}

// NT = inverse(transpose(M)); false where the determinant, as inverse computes it, is zero.
inline bool normal_transform(const double *M, double *NT) {
    double t[16];
    transpose(M, t);
    return inverse(t, NT);
}

}  // namespace rtps
