// far_dist_host.cpp — TEST ONLY: the traversal's root-free cull (rt_wavefront.h far_gt,
// kFarMax2, box_dist2 frames) compiled for the host, against sqrtf and against rt_path.h's
// closest_hit, which keeps the sqrt form op for op.  Built by tests/test_far_dist.py with
// RT_FAR_DIST2=1 and =0.
#include <cfloat>
#include <cmath>
#include "mega_emu.h"

// far_gt(x, acc) against sqrtf(x) > acc: every exponent of acc from denormal to 2^30 with
// 2^16 mantissas each (far_case_acc, clamped to 1e9f), x at the 9 floats around
// (float)(acc * acc) and the 5 around the exact boundary (far_case_x); then the special
// values.  Returns the mismatches.
extern "C" long long fd_far_gt_check() {
    long long bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (int e = 0; e < rtd::kFarCaseExps; ++e)
        for (uint32_t n = 0; n < (1u << 16); ++n) {
            const float acc = rtd::far_case_acc((uint32_t)e, n);
            for (int v = 0; v < rtd::kFarCaseXs; ++v) {
                const float x = rtd::far_case_x(acc, v);
                bad += rtd::far_gt(x, acc) != (sqrtf(x) > acc);
            }
        }
    const float accs[6] = {0.f, -0.f, 1e-45f, FLT_MIN, 1.f, 1e9f};
    const float xs[9] = {0.f, 1e-45f, FLT_MIN, 1.f, 4.f, 9.f, 1e18f, __builtin_inff(), __builtin_nanf("")};
    for (float acc : accs)
        for (float x : xs) bad += rtd::far_gt(x, acc) != (sqrtf(x) > acc);
    return bad;
}

// The generator itself: the cases must straddle the boundary (both answers occur among the
// x of one acc) or the check above proves nothing.  Returns the acc (of 2^12 per exponent)
// whose 14 x give one answer only, outside the exponents where acc * acc leaves the floats.
extern "C" long long fd_case_spread() {
    long long flat = 0;
    for (int e = 64; e < rtd::kFarCaseExps; ++e)   // (below 2^-63 acc * acc is denormal or 0)
        for (uint32_t n = 0; n < (1u << 12); ++n) {
            const float acc = rtd::far_case_acc((uint32_t)e, n);
            int yes = 0;
            for (int v = 0; v < rtd::kFarCaseXs; ++v) yes += sqrtf(rtd::far_case_x(acc, v)) > acc;
            flat += yes == 0 || yes == rtd::kFarCaseXs;
        }
    return flat;
}

// x > kFarMax2 against sqrtf(x) > 1e9f: every float within 64 ulps of the constant, 0, inf, NaN.
extern "C" long long fd_const_check() {
    long long bad = 0;
    for (int d = -64; d <= 64; ++d) {
        const float x = rtd::far_case_step(rtd::kFarMax2, d);
        bad += (x > rtd::kFarMax2) != (sqrtf(x) > 1e9f);
    }
    for (float x : {0.f, __builtin_inff(), __builtin_nanf("")}) bad += (x > rtd::kFarMax2) != (sqrtf(x) > 1e9f);
    // the constant is the last float with the root at or below 1e9f
    bad += !(sqrtf(rtd::kFarMax2) <= 1e9f) || !(sqrtf(rtd::far_case_step(rtd::kFarMax2, 1)) > 1e9f);
    return bad;
}

extern "C" int fd_far_dist2() { return rtd::kFarDist2 ? 1 : 0; }

namespace {
// A plain array stack that also counts the culls decided at equality: a far frame that
// survives is followed at once by the best frame holding the near subtree's best (trav_pop),
// so the pair (entry distance or its square, best) is seen here.
struct WatchStack {
    uint2 *p;
    float last_far = -1.f;
    long long equal = 0;
    void put(int i, uint2 v) {
        if (v.x == rtd::kFrameAcc && last_far >= 0.f) {
            const float acc = __uint_as_float(v.y);
            equal += rtd::kFarDist2 ? last_far == acc * acc : last_far == acc;
        }
        last_far = -1.f;
        p[i] = v;
    }
    uint2 get(int i) {
        const uint2 v = p[i];
        last_far = v.x == rtd::kFrameAcc ? -1.f : __uint_as_float(v.y);
        return v;
    }
};
}  // namespace

// n rays through trav_step (the frames of this build) and through closest_hit.  out_i per
// ray: primitive, AABB tests, triangle tests of trav_step; out_t: its t.  Returns the rays
// on which the two differ (primitive, t bits, either count); *equal_culls: the far children
// entered with their entry distance equal to the near subtree's best.
extern "C" long long fd_trace(const rt_scene_view *v, long long n, const float *org, const float *dir, int32_t *out_i,
                              float *out_t, long long *equal_culls) {
    const rtd::DevScene sc = emu::make(v);
    const rtd::NodeRec root = rtd::load_node(sc.node, 0);
    const rtd::GlobalNodes nodes{sc.node};
    long long bad = 0, equal = 0;
    for (long long i = 0; i < n; ++i) {
        const rtd::Ray r = rtd::make_ray(rtv::V3{org[3 * i], org[3 * i + 1], org[3 * i + 2]},
                                         rtv::V3{dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]});
        rtd::Counters ca{0, 0, 0, 0, 0, 0, 0}, cb{0, 0, 0, 0, 0, 0, 0};
        rtd::Hit want{1e9f, 0.f, 0.f, -1};
        rtd::closest_hit<true>(sc, r, want, ca);
        float e;
        const uint32_t bits = rtd::box_hit<false>(root.mn, root.mx, r, e) ? 0u : 8u;
        uint2 frames[rtd::kStack];
        WatchStack S{frames};
        rtd::TravState T;
        if (rtd::trav_start<true>(bits, root.a, root.b, T, cb))
            while (!rtd::trav_step<true>(sc, r, T, S, nodes, cb)) {
            }
        equal += S.equal;
        out_i[3 * i] = T.best.prim;
        out_i[3 * i + 1] = (int32_t)cb.aabb;
        out_i[3 * i + 2] = (int32_t)cb.tri;
        out_t[i] = T.best.t;
        const bool hit = T.best.prim >= 0;
        bad += T.best.prim != want.prim || (hit && std::memcmp(&T.best.t, &want.t, 4) != 0) || ca.aabb != cb.aabb ||
               ca.tri != cb.tri;
    }
    *equal_culls = equal;
    return bad;
}
