// rt_temporal.h — the reprojected temporal history of a preview frame (host and device, no HIP).
//
// rt_temporal / rt_temporal_device (include/rt_hw.h has the rule in full) blend a frame's
// demodulated radiance with the previous frame's result at the pixel where the same surface point
// was seen: the temporal half of SVGF (Schied et al. 2017), in front of the spatial filters of
// rt_denoise.h and rt_denoise_guided.h.  The per-pixel text lives here and is shared by the device
// kernel (rt_temporal_device.h) and the host function (rt_host.cpp rt_temporal), the way
// rt_denoise.h is.  Only f32 +, -, *, /, comparisons and selects, in the order written; every
// translation unit that includes this is built with -ffp-contract=off, and the device build with
// correctly rounded division, so host, device and a numpy restatement agree bit for bit.
//
// The thresholds are picked, not measured: alpha = 0.2 and the moments' 0.2 are SVGF's, the plane
// fraction 0.02 is rt_denoise's, 0.9 for the normals is a guess; the plane test is hard (a tap is in
// or out) and the footprint is the bilinear one alone, without SVGF's 3 x 3 fallback.
// Known limits: a freshly disoccluded pixel reports a variance of 0 (one frame measures none), and
// the blend weighs frames, not sample counts (a frame of 1 sample counts as one of 16).
#pragma once
#include <cstdint>

#include "rt_denoise.h"

namespace rttm {

using rtdn::Q;

constexpr int kHistoryQuads = 3;   // (L, N), (M1, 0), (M2, 0): RT_HISTORY_WORDS / 4, plane-major
constexpr float kDefaultAlpha = 0.2f;
constexpr float kDefaultAlphaMoments = 0.2f;
constexpr float kDefaultSigmaPlane = 0.02f;   // as a fraction of the centre's hit distance
constexpr float kDefaultNormalMin = 0.9f;
constexpr int kDefaultMaxHistory = 65536;
constexpr int kMaxMaxHistory = 1 << 20;

struct Params {
    float alpha, alpha_moments, sigma_plane, normal_min;
    float max_history;   // (exact: at most 2^20)
};

// rt_temporal_params to the values the step runs with: 0 fine, 1 = RT_ERR_ARG.
inline int resolve_params(float alpha, float alpha_moments, float sigma_plane, float normal_min, int max_history, Params &out) {
    if (!rtdn::finite(alpha) || !rtdn::finite(alpha_moments) || !rtdn::finite(sigma_plane) || !rtdn::finite(normal_min)) return 1;
    if (alpha > 1.f || alpha_moments > 1.f || max_history > kMaxMaxHistory) return 1;
    out.alpha = alpha > 0.f ? alpha : kDefaultAlpha;
    out.alpha_moments = alpha_moments > 0.f ? alpha_moments : kDefaultAlphaMoments;
    out.sigma_plane = sigma_plane > 0.f ? sigma_plane : kDefaultSigmaPlane;
    out.normal_min = normal_min > 0.f ? normal_min : kDefaultNormalMin;
    out.max_history = (float)(max_history > 0 ? max_history : kDefaultMaxHistory);
    return 0;
}

// The previous frame's camera (rt_camera's words).
struct Camera {
    float pos[3], axes[9], tan[2];
};

// What a pixel writes: its history record and its two outputs.
struct Pixel {
    Q h[kHistoryQuads];
    float mean[3];
    float variance;
};

// The previous frame as a tap source: hist(plane, x, y) reads a history quad, g(k, x, y) quad k of
// a first-hit record (only 0, 2 and 3 are read).
struct PlainSrc {
    const Q *H, *G;
    int W;
    long long n;
    RT_HD Q hist(int plane, int x, int y) const { return H[plane * n + (long long)y * W + x]; }
    RT_HD Q g(int k, int x, int y) const { return G[4 * ((long long)y * W + x) + k]; }
};

// floor of f for f in (-1, 2^31): the truncation, less 1 where that lies above f.
RT_HD int floor_of(float f, float &frac) {
    int i = (int)f;
    if ((float)i > f) i = i - 1;
    frac = f - (float)i;
    return i;
}

RT_HD float max_of(float a, float b) { return a > b ? a : b; }

// The look-up: the previous frame's history at the point the pixel sees, over the bilinear taps
// that show the same surface.  nt, pp: the centre, (N, t) and (P, 0): the pixel's own, or its motion
// record's carried normal and position with the pixel's t (temporal_pixel); mesh: its mesh id.
// hq: (Lh, Nh), (M1h, 0), (M2h, 0).  False: no history.
template <class Src>
RT_HD bool lookup(const Src &prev, const Camera &cam, const Q &nt, const Q &pp, int32_t mesh, int W, int H, const Params &tp,
                  Q *hq) {
    const float vx = pp.x - cam.pos[0], vy = pp.y - cam.pos[1], vz = pp.z - cam.pos[2];
    const float *R = cam.axes, *U = cam.axes + 3, *F = cam.axes + 6;
    const float z = (vx * F[0] + vy * F[1]) + vz * F[2];
    if (!(z > 0.f)) return false;
    const float cx = ((vx * R[0] + vy * R[1]) + vz * R[2]) / z;
    const float cy = ((vx * U[0] + vy * U[1]) + vz * U[2]) / z;
    const float fx = ((cx / cam.tan[0] + 1.f) * 0.5f) * (float)W - 0.5f;
    const float fy = ((1.f - cy / cam.tan[1]) * 0.5f) * (float)H - 0.5f;
    if (!(fx > -1.f && fx < (float)W && fy > -1.f && fy < (float)H)) return false;   // (a NaN fails: before any conversion)
    float wx, wy;
    const int x0 = floor_of(fx, wx), y0 = floor_of(fy, wy);
    const rtdn::Geo gc{nt, pp, tp.sigma_plane * nt.w, 0};
    float sb = 0.f, s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[3] = {0.f, 0.f, 0.f}, s2[3] = {0.f, 0.f, 0.f};
    for (int dy = 0; dy <= 1; ++dy)
        for (int dx = 0; dx <= 1; ++dx) {
            const int qx = x0 + dx, qy = y0 + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float b = (dx ? wx : 1.f - wx) * (dy ? wy : 1.f - wy);
            if (!(b > 0.f)) continue;
            const Q h0 = prev.hist(0, qx, qy);
            if (!(h0.w > 0.f)) continue;
            const int32_t mq = (int32_t)rtm::f2u(prev.g(2, qx, qy).w);
            if (mq < 0 || mq != mesh) continue;
            const Q nq = prev.g(0, qx, qy);
            const float nd = (nt.x * nq.x + nt.y * nq.y) + nt.z * nq.z;
            if (!(nd >= tp.normal_min)) continue;
            const float pd = rtdn::plane_dist(gc, prev.g(3, qx, qy));
            if (!((pd < 0.f ? -pd : pd) <= gc.plane_den)) continue;
            const Q h1 = prev.hist(1, qx, qy), h2 = prev.hist(2, qx, qy);
            sb = sb + b;
            s0[0] = s0[0] + b * h0.x, s0[1] = s0[1] + b * h0.y, s0[2] = s0[2] + b * h0.z, s0[3] = s0[3] + b * h0.w;
            s1[0] = s1[0] + b * h1.x, s1[1] = s1[1] + b * h1.y, s1[2] = s1[2] + b * h1.z;
            s2[0] = s2[0] + b * h2.x, s2[1] = s2[1] + b * h2.y, s2[2] = s2[2] + b * h2.z;
        }
    if (!(sb > 0.f)) return false;
    hq[0] = Q{s0[0] / sb, s0[1] / sb, s0[2] / sb, s0[3] / sb};
    hq[1] = Q{s1[0] / sb, s1[1] / sb, s1[2] / sb, 0.f};
    hq[2] = Q{s2[0] / sb, s2[1] / sb, s2[2] / sb, 0.f};
    return rtdn::finite(hq[0].x) && rtdn::finite(hq[0].y) && rtdn::finite(hq[0].z) && rtdn::finite(hq[0].w) &&
           rtdn::finite(hq[1].x) && rtdn::finite(hq[1].y) && rtdn::finite(hq[1].z) && rtdn::finite(hq[2].x) &&
           rtdn::finite(hq[2].y) && rtdn::finite(hq[2].z);
}

// The whole step at pixel (x, y) of a W x H frame.  S: its three sums; n: its sample count; g: its
// first-hit record (4 x Q); has_prev: a previous frame exists (prev and cam are read only then).
// mo: the pixel's motion record (rt_motion.h: (P_prev, state), (N_prev, 0)) or null.  Null and
// state 0: the look-up from the pixel's own (N, t) and P; state 1: from ((N_prev, t), P_prev), which
// are then the projected point and the centre of the normal and plane tests; any other state: no
// history.
template <class Src>
RT_HD Pixel temporal_pixel(const Src &prev, bool has_prev, const Camera &cam, const float *S, int n, const Q *g, int W, int H,
                           const Params &tp, const Q *mo = nullptr) {
    Pixel r;
    r.h[0] = r.h[1] = r.h[2] = Q{0.f, 0.f, 0.f, 0.f};
    r.variance = 0.f;
    Q a, nt, pp;
    rtdn::prepare_pixel(S, n, g, a, nt, pp);
    const uint32_t kind = rtm::f2u(a.w);
    if (kind == rtdn::kPass) {   // its own mean, no history
        rtdn::resolve_pixel(S, n, g, a, r.mean);
        return r;
    }
    Q hq[kHistoryQuads];
    // (one call for both centres: the pixels of a wave that carry and those that do not look up together)
    Q cn = nt, cp = pp;
    bool look = has_prev;
    if (mo) {
        const uint32_t state = rtm::f2u(mo[0].w);
        if (state == 1u)
            cn = Q{mo[1].x, mo[1].y, mo[1].z, nt.w}, cp = Q{mo[0].x, mo[0].y, mo[0].z, 0.f};
        else if (state != 0u)
            look = false;
    }
    const bool have = look && lookup(prev, cam, cn, cp, (int32_t)rtm::f2u(g[2].w), W, H, tp, hq);
    const float L[3] = {a.x, a.y, a.z};
    float N1 = 0.f, L1[3] = {0.f, 0.f, 0.f}, M1[3] = {0.f, 0.f, 0.f}, M2[3] = {0.f, 0.f, 0.f};
    bool done = false;
    if (kind == rtdn::kValid) {
        if (have) {
            const float up = hq[0].w + 1.f;
            N1 = up < tp.max_history ? up : tp.max_history;
            const float rN = 1.f / N1, al = max_of(tp.alpha, rN), am = max_of(tp.alpha_moments, rN);
            const float Lh[3] = {hq[0].x, hq[0].y, hq[0].z}, M1h[3] = {hq[1].x, hq[1].y, hq[1].z},
                        M2h[3] = {hq[2].x, hq[2].y, hq[2].z};
            done = true;
            for (int c = 0; c < 3; ++c) {
                L1[c] = Lh[c] + al * (L[c] - Lh[c]);
                M1[c] = M1h[c] + am * (L[c] - M1h[c]);
                M2[c] = M2h[c] + am * (L[c] * L[c] - M2h[c]);
                done = done && rtdn::finite(L1[c]) && rtdn::finite(M1[c]) && rtdn::finite(M2[c]);
            }
        }
        if (!done) {   // no history, or one that overflowed
            N1 = 1.f;
            for (int c = 0; c < 3; ++c) L1[c] = M1[c] = L[c], M2[c] = L[c] * L[c];
        }
    } else if (have) {   // fill: the history as it is, no frame added
        N1 = hq[0].w;
        L1[0] = hq[0].x, L1[1] = hq[0].y, L1[2] = hq[0].z;
        M1[0] = hq[1].x, M1[1] = hq[1].y, M1[2] = hq[1].z;
        M2[0] = hq[2].x, M2[1] = hq[2].y, M2[2] = hq[2].z;
    }
    // (a fill pixel without history: zero words, N' = 0, and the resolve gives E)
    r.h[0] = Q{L1[0], L1[1], L1[2], N1};
    r.h[1] = Q{M1[0], M1[1], M1[2], 0.f};
    r.h[2] = Q{M2[0], M2[1], M2[2], 0.f};
    rtdn::resolve_pixel(S, n, g, Q{L1[0], L1[1], L1[2], a.w}, r.mean);
    if (N1 >= 2.f) {
        const float al = max_of(tp.alpha, 1.f / N1);
        float v[3];
        for (int c = 0; c < 3; ++c) {
            v[c] = M2[c] - M1[c] * M1[c];
            v[c] = v[c] > 0.f ? v[c] : 0.f;
        }
        const float V = ((v[0] + v[1]) + v[2]) * al;
        r.variance = rtdn::finite(V) ? V : 0.f;
    }
    return r;
}

}  // namespace rttm
