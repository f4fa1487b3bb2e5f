// rt_denoise.h — the edge-avoiding a-trous filter of a low-sample frame (host and device, no HIP).
//
// rt_denoise / rt_denoise_device (include/rt_hw.h has the rules in full) filter a whole frame of
// sums, guided by its first-hit records (rt_gbuffer.h).  The per-pixel text of the three steps
// (prepare, one level, resolve) lives here and is shared by the device kernels
// (rt_denoise_device.h) and the host function (rt_host.cpp rt_denoise), the way rt_select.h and
// rt_fast_units.h are shared.  Only f32 +, -, *, /, comparisons and selects, in the order written;
// the falloffs are rational, 1 / (1 + x), so there is no exp to differ between libraries.  Every
// translation unit that includes this is built with -ffp-contract=off, and the device build with
// correctly rounded division, so host, device and a numpy restatement agree bit for bit.
#pragma once
#include <cstdint>

#include "rt_libm.h"

namespace rtdn {

constexpr int kMaxIterations = 6;
constexpr int kMaxNormalPowerLog2 = 16;
// Defaults.  5 levels (a 125-pixel footprint) and a normal exponent of 2^6 are the usual choices
// for this filter; the two sigmas are picked, not tuned: no measurement stands behind them.
constexpr int kDefaultIterations = 5;
constexpr int kDefaultNormalPowerLog2 = 6;
constexpr float kDefaultSigmaColor = 2.f;     // in units of demodulated radiance, at level 0
constexpr float kDefaultSigmaPlane = 0.02f;   // as a fraction of the centre's hit distance
constexpr float kAlbedoFloor = 1e-3f;

// What a pixel is to the filter (word w of its packed colour, as int bits).
constexpr uint32_t kPass = 0;    // miss, or a hit whose mean (or demodulated mean) is not finite: its own
                                 // mean passes through, and it contributes to no other pixel
constexpr uint32_t kValid = 1;   // hit, n > 0, finite: filtered, contributes
constexpr uint32_t kFill = 2;    // hit, n == 0: filled from its neighbours (colour term 1), contributes
                                 // from the level after the one that filled it

// 16 bytes, read and written whole.
struct alignas(16) Q {
    float x, y, z, w;
};

struct Params {
    int iterations;
    float sigma_color, sigma_plane;
    int normal_power_log2;
};

RT_HD bool finite(float v) { return (rtm::f2u(v) & 0x7f800000u) != 0x7f800000u; }

// rt_denoise_params to the values the filter runs with: 0 fine, 1 = RT_ERR_ARG.  iterations 0 is a
// value of its own (no filtering), so only a negative one takes the default.
inline int resolve_params(int iterations, float sigma_color, float sigma_plane, int normal_power_log2, Params &out) {
    if (iterations > kMaxIterations || normal_power_log2 > kMaxNormalPowerLog2) return 1;
    if (!finite(sigma_color) || !finite(sigma_plane)) return 1;
    out.iterations = iterations < 0 ? kDefaultIterations : iterations;
    out.sigma_color = sigma_color > 0.f ? sigma_color : kDefaultSigmaColor;
    out.sigma_plane = sigma_plane > 0.f ? sigma_plane : kDefaultSigmaPlane;
    out.normal_power_log2 = normal_power_log2 > 0 ? normal_power_log2 : kDefaultNormalPowerLog2;
    return 0;
}

// The reciprocal a sum is multiplied by, as the frame finish does (rt_select.h count_normalizer).
RT_HD float mean_normalizer(int n) { return n > 0 ? 1.f / (float)n : 0.f; }

RT_HD float floor_albedo(float a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }

// Prepare: the pixel's mean, its kind and its demodulated colour L = (m - E) / a'.
// S: the pixel's three sums; n: its sample count; g: its first-hit record (4 x Q).
// a: (L.xyz, kind); nt: (N.xyz, t); pp: (P.xyz, 0).
RT_HD void prepare_pixel(const float *S, int n, const Q *g, Q &a, Q &nt, Q &pp) {
    const float rn = mean_normalizer(n);
    const bool hit = (int32_t)rtm::f2u(g[1].w) >= 0;
    const float al[3] = {g[1].x, g[1].y, g[1].z}, E[3] = {g[2].x, g[2].y, g[2].z};
    float L[3];
    bool fin = true;
    for (int c = 0; c < 3; ++c) {
        const float m = S[c] * rn;
        L[c] = (m - E[c]) / floor_albedo(al[c]);
        fin = fin && finite(m) && finite(L[c]);
    }
    const uint32_t kind = !hit ? kPass : (n <= 0 ? kFill : (fin ? kValid : kPass));
    const bool keep = kind == kValid;
    a = Q{keep ? L[0] : 0.f, keep ? L[1] : 0.f, keep ? L[2] : 0.f, rtm::u2f(kind)};
    nt = g[0];
    pp = g[3];
}

// The constants of level k (stride 2^k): the colour sigma halves per level, (sigma_color 2^-k)^2.
struct Level {
    int stride;
    float sigma_plane;
    float color_den;
    int normal_power_log2;
};
inline Level level_of(const Params &p, int k) {
    const float sck = p.sigma_color * (1.f / (float)(1 << k));
    return Level{1 << k, p.sigma_plane, sck * sck, p.normal_power_log2};
}

// The B3-spline weight by |offset|: 3/8, 1/4, 1/16 (their products are exact).
RT_HD float spline(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// What the centre contributes to a tap's normal and plane terms.
struct Geo {
    Q np, pp;
    float plane_den;
    int normal_power_log2;
};
template <class Src>
RT_HD Geo geo_of(const Src &src, int x, int y, float sigma_plane, int normal_power_log2) {
    const Q np = src.nt(x, y);
    return Geo{np, src.pp(x, y), sigma_plane * np.w, normal_power_log2};
}
RT_HD float normal_term(const Geo &c, const Q &nq) {
    float nd = (c.np.x * nq.x + c.np.y * nq.y) + c.np.z * nq.z;
    nd = nd > 0.f ? nd : 0.f;
    for (int i = 0; i < c.normal_power_log2; ++i) nd = nd * nd;
    return nd;
}
// The tap's signed distance from the centre's tangent plane (rt_temporal.h tests it against plane_den).
RT_HD float plane_dist(const Geo &c, const Q &pq) {
    const float ex = pq.x - c.pp.x, ey = pq.y - c.pp.y, ez = pq.z - c.pp.z;
    return (c.np.x * ex + c.np.y * ey) + c.np.z * ez;
}
RT_HD float plane_term(const Geo &c, const Q &pq) {
    const float pr = plane_dist(c, pq) / c.plane_den;
    return 1.f / (1.f + pr * pr);
}
// The colour term of tap q at a centre c of kind `kind`: 1 for a centre that is being filled.
RT_HD float color_term(uint32_t kind, const Q &c, const Q &q, float color_den) {
    float wc = 1.f;
    if (kind == kValid) {
        const float lx = q.x - c.x, ly = q.y - c.y, lz = q.z - c.z;
        const float d2 = (lx * lx + ly * ly) + lz * lz;
        wc = 1.f / (1.f + d2 / color_den);
    }
    return wc;
}
// A tap's weight: the spline weight h and the three terms, multiplied in this order.
RT_HD float tap_weight(float h, float nd, float wp, float wc) {
    float w = h * nd;
    w = w * wp;
    w = w * wc;
    return w;
}

// One level at centre (x, y) of a W x H frame.  src.a / src.nt / src.pp(qx, qy) read the three
// packed words of a tap (global memory, LDS or a host array: the same text runs over each).
// (rt_denoise_guided.h's level is a loop of its own over the same weight functions: one loop for
// both, with a flag for the variance, made this mode's five levels 4% slower)
template <class Src>
RT_HD Q level_pixel(const Src &src, int x, int y, int W, int H, const Level &lv) {
    const Q c = src.a(x, y);
    const uint32_t kind = rtm::f2u(c.w);
    if (kind == kPass) return c;
    const Geo gc = geo_of(src, x, y, lv.sigma_plane, lv.normal_power_log2);
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * lv.stride, qy = y + dy * lv.stride;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const Q q = src.a(qx, qy);
            if (rtm::f2u(q.w) != kValid) continue;
            const Q nq = src.nt(qx, qy), pq = src.pp(qx, qy);
            const float h = spline(dx) * spline(dy);
            const float w = tap_weight(h, normal_term(gc, nq), plane_term(gc, pq), color_term(kind, c, q, lv.color_den));
            if (!(w > 0.f)) continue;   // (zero and NaN weights: perpendicular faces, a centre at t = 0)
            sw = sw + w;
            sx = sx + w * q.x;
            sy = sy + w * q.y;
            sz = sz + w * q.z;
        }
    if (!(sw > 0.f)) return Q{0.f, 0.f, 0.f, c.w};
    const Q r{sx / sw, sy / sw, sz / sw, rtm::u2f(kValid)};   // (a filled pixel is valid from here on)
    if (!(finite(r.x) && finite(r.y) && finite(r.z))) return c;   // (an overflow: the centre keeps its value)
    return r;
}

// Resolve: m' = L' a' + E for a filtered pixel, the pixel's own mean for one that passes through.
RT_HD void resolve_pixel(const float *S, int n, const Q *g, const Q &a, float *out) {
    if (rtm::f2u(a.w) == kPass) {
        const float rn = mean_normalizer(n);
        for (int c = 0; c < 3; ++c) out[c] = S[c] * rn;
        return;
    }
    out[0] = a.x * floor_albedo(g[1].x) + g[2].x;
    out[1] = a.y * floor_albedo(g[1].y) + g[2].y;
    out[2] = a.z * floor_albedo(g[1].z) + g[2].z;
}

// A tap source over three row-major arrays (the host function; the device's plain-load path).
struct PlainSrc {
    const Q *A, *NT, *PP;
    int W;
    RT_HD Q a(int x, int y) const { return A[(long long)y * W + x]; }
    RT_HD Q nt(int x, int y) const { return NT[(long long)y * W + x]; }
    RT_HD Q pp(int x, int y) const { return PP[(long long)y * W + x]; }
};

}  // namespace rtdn
