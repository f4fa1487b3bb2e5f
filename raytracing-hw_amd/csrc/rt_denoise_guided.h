// rt_denoise_guided.h — the variance-guided mode of the frame denoiser (host and device, no HIP).
//
// rt_denoise_guided / rt_denoise_guided_device (include/rt_hw.h has the rules in full) are the
// a-trous filter of rt_denoise.h with three changes, after SVGF (Schied et al. 2017): surfaces whose
// radiance is not albedo-modulated pass through, a firefly clamp runs before the filter, and the
// colour falloff is measured in standard deviations of a per-pixel variance that is filtered along
// with the colour.  The per-pixel text of the clamp, the variance estimate and the guided level
// lives here, shared by the device kernels (rt_denoise_device.h) and the host function (rt_host.cpp
// rt_denoise_guided); prepare, the terms and the product of a tap's weight, and resolve are
// rt_denoise.h's.  The same arithmetic rules hold: f32 +, -, *, /, comparisons and selects in the
// order written, no contraction, correctly rounded division.
#pragma once
#include "rt_denoise.h"

namespace rtdg {

using rtdn::Geo;
using rtdn::Q;
using rtdn::finite;
using rtdn::geo_of;
using rtdn::kFill;
using rtdn::kPass;
using rtdn::kValid;
using rtdn::normal_term;
using rtdn::plane_term;

// Defaults.  sigma_var 2 and firefly 8, with the 5 x 5 clamp window and the 7 x 7 variance window,
// come from a coarse sweep on three small fixtures (sigma_var in {1, 2, 4}, firefly in {off, 2, 4,
// 8, 16}); they were not tuned on the headline frame.
constexpr float kDefaultSigmaVar = 2.f;
constexpr float kDefaultFirefly = 8.f;
constexpr float kColorDenFloor = 1e-8f;
constexpr int kClampReach = 2;      // 5 x 5
constexpr int kVarianceReach = 3;   // 7 x 7

struct Params {
    int iterations;
    float sigma_var, sigma_plane;
    int normal_power_log2;
    float firefly;   // < 0: no clamp
};

// rt_denoise_guided_params to the values the filter runs with: 0 fine, 1 = RT_ERR_ARG.
inline int resolve_params(int iterations, float sigma_var, float sigma_plane, int normal_power_log2, float firefly, Params &out) {
    if (iterations > rtdn::kMaxIterations || normal_power_log2 > rtdn::kMaxNormalPowerLog2) return 1;
    if (!finite(sigma_var) || !finite(sigma_plane) || !finite(firefly)) return 1;
    out.iterations = iterations < 0 ? rtdn::kDefaultIterations : iterations;
    out.sigma_var = sigma_var > 0.f ? sigma_var : kDefaultSigmaVar;
    out.sigma_plane = sigma_plane > 0.f ? sigma_plane : rtdn::kDefaultSigmaPlane;
    out.normal_power_log2 = normal_power_log2 > 0 ? normal_power_log2 : rtdn::kDefaultNormalPowerLog2;
    out.firefly = firefly == 0.f ? kDefaultFirefly : firefly;
    return 0;
}

// Prepare: rt_denoise's, and a hit whose albedo is at the floor in every channel passes through
// (an emitter or a black surface: its radiance is not albedo times irradiance, so its demodulated
// value, m / 1e-3, would flood its coplanar neighbours).
RT_HD void prepare_pixel(const float *S, int n, const Q *g, Q &a, Q &nt, Q &pp) {
    rtdn::prepare_pixel(S, n, g, a, nt, pp);
    const bool hit = (int32_t)rtm::f2u(g[1].w) >= 0;
    if (hit && !(g[1].x > rtdn::kAlbedoFloor) && !(g[1].y > rtdn::kAlbedoFloor) && !(g[1].z > rtdn::kAlbedoFloor))
        a = Q{0.f, 0.f, 0.f, rtm::u2f(kPass)};
}

RT_HD float lum(const Q &L) { return (0.2126f * L.x + 0.7152f * L.y) + 0.0722f * L.z; }

// The firefly clamp at (x, y): the pixel's (L, kind) with L scaled down to `firefly` times the
// geometry-weighted mean luminance of its 5 x 5 neighbours (centre skipped).
template <class Src>
RT_HD Q clamp_pixel(const Src &src, int x, int y, int W, int H, const Params &p) {
    const Q c = src.a(x, y);
    if (rtm::f2u(c.w) != kValid) return c;
    const Geo gc = geo_of(src, x, y, p.sigma_plane, p.normal_power_log2);
    float sg = 0.f, sl = 0.f;
    for (int dy = -kClampReach; dy <= kClampReach; ++dy)
        for (int dx = -kClampReach; dx <= kClampReach; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const Q q = src.a(qx, qy);
            if (rtm::f2u(q.w) != kValid) continue;
            const float g = normal_term(gc, src.nt(qx, qy)) * plane_term(gc, src.pp(qx, qy));
            if (!(g > 0.f)) continue;
            sg = sg + g;
            sl = sl + g * lum(q);
        }
    if (!(sg > 0.f)) return c;
    const float mean = sl / sg;
    const float cap = p.firefly * (mean > 0.f ? mean : 0.f);
    const float lc = lum(c);
    if (!(lc > cap)) return c;
    const float scale = cap / lc;
    return Q{c.x * scale, c.y * scale, c.z * scale, c.w};
}

// The caller's variance of a pixel of kind `kind`.
RT_HD float given_variance(uint32_t kind, float v) { return kind == kValid && finite(v) && v > 0.f ? v : 0.f; }

// The spatial variance estimate at (x, y): the geometry-weighted variance of L over the 7 x 7
// window (centre included), summed over the channels.
template <class Src>
RT_HD float variance_pixel(const Src &src, int x, int y, int W, int H, const Params &p) {
    if (rtm::f2u(src.a(x, y).w) != kValid) return 0.f;
    const Geo gc = geo_of(src, x, y, p.sigma_plane, p.normal_power_log2);
    float sg = 0.f, s1[3] = {0.f, 0.f, 0.f}, s2[3] = {0.f, 0.f, 0.f};
    int used = 0;
    for (int dy = -kVarianceReach; dy <= kVarianceReach; ++dy)
        for (int dx = -kVarianceReach; dx <= kVarianceReach; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const Q q = src.a(qx, qy);
            if (rtm::f2u(q.w) != kValid) continue;
            const float g = normal_term(gc, src.nt(qx, qy)) * plane_term(gc, src.pp(qx, qy));
            if (!(g > 0.f)) continue;
            sg = sg + g;
            s1[0] = s1[0] + g * q.x;
            s1[1] = s1[1] + g * q.y;
            s1[2] = s1[2] + g * q.z;
            s2[0] = s2[0] + g * (q.x * q.x);
            s2[1] = s2[1] + g * (q.y * q.y);
            s2[2] = s2[2] + g * (q.z * q.z);
            ++used;
        }
    if (used < 2) return 0.f;
    float var[3];
    for (int c = 0; c < 3; ++c) {
        const float mu = s1[c] / sg;
        const float v = s2[c] / sg - mu * mu;
        var[c] = v > 0.f ? v : 0.f;
    }
    const float V = (var[0] + var[1]) + var[2];
    return finite(V) ? V : 0.f;
}

// The constants of level k (stride 2^k).  The colour falloff does not halve per level: the
// variance it is measured against shrinks as the levels average.
struct Level {
    int stride;
    float sigma_plane;
    float sigma_var2;
    int normal_power_log2;
};
inline Level level_of(const Params &p, int k) { return Level{1 << k, p.sigma_plane, p.sigma_var * p.sigma_var, p.normal_power_log2}; }

// The variance prefilter's weight by |offset|: 1/2, 1/4.
RT_HD float tent(int d) { return d == 0 ? 0.5f : 0.25f; }

struct Pixel {
    Q a;
    float v;
};

// One guided level at centre (x, y).  src.a / nt / pp as rt_denoise's, src.v the variance.
template <class Src>
RT_HD Pixel level_pixel(const Src &src, int x, int y, int W, int H, const Level &lv) {
    const Q c = src.a(x, y);
    const float vc = src.v(x, y);
    const uint32_t kind = rtm::f2u(c.w);
    if (kind == kPass) return Pixel{c, vc};
    float gw = 0.f, gv = 0.f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            if (rtm::f2u(src.a(qx, qy).w) != kValid) continue;
            const float cw = tent(dx) * tent(dy);
            gw = gw + cw;
            gv = gv + cw * src.v(qx, qy);
        }
    const float vbar = gw > 0.f ? gv / gw : 0.f;
    const float color_den = lv.sigma_var2 * vbar + kColorDenFloor;
    const Geo gc = geo_of(src, x, y, lv.sigma_plane, lv.normal_power_log2);
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, sv = 0.f;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * lv.stride, qy = y + dy * lv.stride;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const Q q = src.a(qx, qy);
            if (rtm::f2u(q.w) != kValid) continue;
            const float h = rtdn::spline(dx) * rtdn::spline(dy);
            const float nd = normal_term(gc, src.nt(qx, qy));
            const float wp = plane_term(gc, src.pp(qx, qy));
            const float w = rtdn::tap_weight(h, nd, wp, rtdn::color_term(kind, c, q, color_den));
            if (!(w > 0.f)) continue;
            sw = sw + w;
            sx = sx + w * q.x;
            sy = sy + w * q.y;
            sz = sz + w * q.z;
            sv = sv + (w * w) * src.v(qx, qy);
        }
    if (!(sw > 0.f)) return Pixel{Q{0.f, 0.f, 0.f, c.w}, 0.f};
    const Q r{sx / sw, sy / sw, sz / sw, rtm::u2f(kValid)};
    if (!(finite(r.x) && finite(r.y) && finite(r.z))) return Pixel{c, vc};
    const float nv = sv / (sw * sw);
    return Pixel{r, finite(nv) ? nv : vc};
}

// out_variance: V of a pixel that is valid after the last level, else 0.
RT_HD float resolve_variance(const Q &a, float v) { return rtm::f2u(a.w) == kValid ? v : 0.f; }

// A tap source over row-major arrays (the host function; the device's plain-load path).
struct PlainSrc {
    const Q *A, *NT, *PP;
    const float *V;
    int W;
    RT_HD Q a(int x, int y) const { return A[(long long)y * W + x]; }
    RT_HD Q nt(int x, int y) const { return NT[(long long)y * W + x]; }
    RT_HD Q pp(int x, int y) const { return PP[(long long)y * W + x]; }
    RT_HD float v(int x, int y) const { return V[(long long)y * W + x]; }
};

}  // namespace rtdg
