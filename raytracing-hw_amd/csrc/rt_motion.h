// rt_motion.h — per-pixel motion records: where the surface point a pixel sees now was at the
// previous push of a history (host and device, no HIP).
//
// rt_motion / rt_motion_device (include/rt_hw.h has the rule in full) carry the hit position P and
// the shading normal N of a first-hit record from the triangle as it stands (tri) to the same
// triangle as it stood (tri_prev): P is expressed in the triangle's own frame (v0, U, V) by a Gram
// solve, and the change of that frame is applied to it.  For a rigid motion of the triangle that is
// the moved point and the rotated normal up to rounding; for a deforming triangle the position is
// the point of equal barycentric coordinates and the normal an approximation.  Neither is
// renormalised.  The per-pixel text lives here and is shared by the device kernel
// (rt_motion_device.h), the host function (rt_host.cpp rt_motion) and, through a numpy
// restatement, the CPU tests.  Only f32 +, -, *, /, comparisons and selects, in the order written;
// no float is ever converted to an int.  Every translation unit that includes this is built with
// -ffp-contract=off, and the device build with correctly rounded division.
//
// The carry is written as a displacement, P + ((dv0 + u dU) + v dV), not as v0' + u U' + v V':
// P = o + d t lies a rounding off its triangle's plane, and the displacement form keeps that
// residue instead of exchanging it for the solve's error, so the error of the carried point scales
// with the motion and not with the coordinates (a translation whose offset is exact in f32 is
// carried exactly: dU = dV = 0).
//
// (The namespace is rt_moments.h's too; the names here are disjoint from its.)
#pragma once
#include <cstdint>

#include "rt_denoise.h"
#include "rt_vec.h"

namespace rtmo {

using rtdn::Q;

constexpr int kMotionQuads = 2;   // (P_prev, state), (N_prev, 0): RT_MOTION_WORDS / 4, pixel-major
constexpr int32_t kStatic = 0;    // the record is the pixel's own P and N
constexpr int32_t kCarried = 1;
constexpr int32_t kLost = 2;      // no history may be taken for this pixel

// det / (a c) is the squared sine of the angle between U and V, and the rounding of a c - b b is a
// few 2^-24 of a c: below 2^-20 (a sliver of less than 0.06 degrees) the solve is noise, not a
// position, and the pixel is lost like one on a degenerate triangle.
constexpr float kMinSin2 = 9.5367431640625e-07f;   // 2^-20

struct Motion {
    Q p, n;
};

RT_HD float dot3(const rtv::V3 &a, const rtv::V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_HD rtv::V3 diff3(const rtv::V3 &a, const rtv::V3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
RT_HD bool finite3(const rtv::V3 &a) { return rtdn::finite(a.x) && rtdn::finite(a.y) && rtdn::finite(a.z); }
// a + ((d0 + s * d1) + t * d2) per component
RT_HD rtv::V3 displaced(const rtv::V3 &a, const rtv::V3 &d0, float s, const rtv::V3 &d1, float t, const rtv::V3 &d2) {
    return {a.x + ((d0.x + s * d1.x) + t * d2.x), a.y + ((d0.y + s * d1.y) + t * d2.y), a.z + ((d0.z + s * d1.z) + t * d2.z)};
}

RT_HD Motion motion_of(const rtv::V3 &P, const rtv::V3 &N, int32_t state) {
    return Motion{Q{P.x, P.y, P.z, rtm::u2f((uint32_t)state)}, Q{N.x, N.y, N.z, 0.f}};
}
RT_HD Motion motion_lost() { return motion_of(rtv::V3{0.f, 0.f, 0.f}, rtv::V3{0.f, 0.f, 0.f}, kLost); }

// The record of a pixel whose first-hit record has quads g0 = (N, t), g1 = (albedo, triangle id)
// and g3 = (P, 0).  tri, tri_prev: the triangle arrays as quads (three per triangle; words 0..8 of
// a record are read); an id outside [0, n_tris) is tested, never indexed.
RT_HD Motion carry_pixel(const Q &g0, const Q &g1, const Q &g3, const Q *tri, const Q *tri_prev, uint32_t n_tris) {
    const rtv::V3 P{g3.x, g3.y, g3.z}, N{g0.x, g0.y, g0.z};
    const int32_t id = (int32_t)rtm::f2u(g1.w);
    if (id < 0 || (uint32_t)id >= n_tris) return motion_of(P, N, kStatic);   // a miss: its own (zero) words
    const Q a0 = tri[3 * (long long)id], a1 = tri[3 * (long long)id + 1], a2 = tri[3 * (long long)id + 2];
    const Q b0 = tri_prev[3 * (long long)id], b1 = tri_prev[3 * (long long)id + 1], b2 = tri_prev[3 * (long long)id + 2];
    const bool same = rtm::f2u(a0.x) == rtm::f2u(b0.x) && rtm::f2u(a0.y) == rtm::f2u(b0.y) && rtm::f2u(a0.z) == rtm::f2u(b0.z) &&
                      rtm::f2u(a0.w) == rtm::f2u(b0.w) && rtm::f2u(a1.x) == rtm::f2u(b1.x) && rtm::f2u(a1.y) == rtm::f2u(b1.y) &&
                      rtm::f2u(a1.z) == rtm::f2u(b1.z) && rtm::f2u(a1.w) == rtm::f2u(b1.w) && rtm::f2u(a2.x) == rtm::f2u(b2.x);
    if (same) return motion_of(P, N, kStatic);
    const rtv::V3 v0{a0.x, a0.y, a0.z}, U{a0.w, a1.x, a1.y}, V{a1.z, a1.w, a2.x};
    const rtv::V3 v0p{b0.x, b0.y, b0.z}, Up{b0.w, b1.x, b1.y}, Vp{b1.z, b1.w, b2.x};
    const rtv::V3 e = diff3(P, v0);
    const float a = dot3(U, U), b = dot3(U, V), c = dot3(V, V);
    const float det = a * c - b * b;
    if (!(det > (a * c) * kMinSin2) || !rtdn::finite(det)) return motion_lost();
    const float d = dot3(U, e), f = dot3(V, e);
    const float u = (c * d - b * f) / det, v = (a * f - b * d) / det;
    const rtv::V3 dv0 = diff3(v0p, v0), dU = diff3(Up, U), dV = diff3(Vp, V);
    const rtv::V3 Pp = displaced(P, dv0, u, dU, v, dV);
    // the normal: N = al U + be V + ga W with W = cross(U, V), the same three numbers on (U', V', W')
    const rtv::V3 Wn = rtv::cross(U, V), Wp = rtv::cross(Up, Vp);
    const float dn = dot3(U, N), fn = dot3(V, N);
    const float al = (c * dn - b * fn) / det, be = (a * fn - b * dn) / det;
    const float ga = dot3(Wn, N) / dot3(Wn, Wn);
    const rtv::V3 dW = diff3(Wp, Wn);
    const rtv::V3 Np{N.x + ((al * dU.x + be * dV.x) + ga * dW.x), N.y + ((al * dU.y + be * dV.y) + ga * dW.y),
                     N.z + ((al * dU.z + be * dV.z) + ga * dW.z)};
    if (!finite3(Pp) || !finite3(Np)) return motion_lost();
    return motion_of(Pp, Np, kCarried);
}

}  // namespace rtmo
