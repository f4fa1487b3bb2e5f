// kernel_host.cpp — TEST ONLY: compiles the GPU kernel source (raytracing-hw_amd/csrc/rt_path.h)
// for the host so tests can check its arithmetic against the goldens without a GPU.  Not
// part of the product: librt_hw_amd.so has no CPU render path.  The emulation of the
// lane-resident kernel's wave loop is mega_emu.h's; the kh_render_mega* entry points here run
// it with the harness's default options (kh_options, written by the kh_set_* setters).
#include "mega_emu.h"

using namespace emu;

// render_pixel (rt_path.h): the reference's recursion order, closest_hit by explicit stack.
extern "C" void kh_render(const rt_scene_view *v, int spp, int64_t p0, int64_t p1, float *out, uint64_t *cnt) {
    rtd::DevScene s = make(v);
    uint64_t c[6] = {0, 0, 0, 0, 0, 0};
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : c[:6])
    for (int64_t p = p0; p < p1; ++p) {
        rtd::Counters k{0, 0, 0, 0, 0, 0, 0};
        rtv::V3 r = rtd::render_pixel<true>(s, (int)(p % v->width), (int)(p / v->width), spp, k);
        out[3 * (p - p0)] = r.x;
        out[3 * (p - p0) + 1] = r.y;
        out[3 * (p - p0) + 2] = r.z;
        c[0] += k.rays; c[1] += k.aabb; c[2] += k.tri; c[3] += k.lq; c[4] += k.laabb; c[5] += k.ltri;
    }
    std::memcpy(cnt, c, sizeof c);
}

// Emulates the wavefront path (wf_init / wf_extend / wf_shade in rt_device.hip) on the host:
// the same rt_wavefront.h slot functions and queue records, driven by a host queue.
extern "C" int kh_render_wf(const rt_scene_view *v, int spp, int rank, int world, int row_block, float *out,
                            uint64_t *cnt_out, int64_t *iterations) {
    const rtd::DevScene sc = make(v);
    const Shard sh = shard_of(v, rank, world, row_block);
    const long long n = sh.n;
    const rtd::ShardGeom g = sh.g;
    const int D = v->ray_depth;
    std::vector<float4> stv((size_t)2 * n), ab((size_t)2 * n * D);
    std::vector<float> cv((size_t)n * D);
    rtd::WfState st{};
    st.n = n;
    st.D = D;
    st.st = stv.data();
    st.rec_ab = ab.data();
    st.rec_c = cv.data();
    std::vector<float4> q((size_t)rtd::kQRec * n), q2((size_t)rtd::kQRec * n), hits((size_t)n);
    unsigned cnt_q = 0;
    for (long long i = 0; i < n; ++i) rtd::store_qray(sc, q.data(), cnt_q++, (int)i, rtd::wf_init_slot(sc, g, st, i));
    rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
    uint2 stk[rtd::kStack];
    int64_t it = 0;
    while (cnt_q > 0) {
        if (++it > (int64_t)spp * D + 16) return -1;
        for (unsigned p = 0; p < cnt_q; ++p) {   // extend
            rtd::Hit h;
            rtd::closest_hit_wf<true>(sc, q.data(), p, h, stk, cnt);
            rtd::store_hit(hits.data(), p, h);
        }
        unsigned cnt_q2 = 0;
        for (unsigned p = 0; p < cnt_q; ++p) {   // shade
            int slot;
            rtd::Ray r = rtd::load_qray(q.data(), p, slot);
            const rtd::Hit h = rtd::load_hit(hits.data(), p);
            if (rtd::wf_shade_slot<true>(sc, g, st, spp, slot, r, h, out, cnt)) rtd::store_qray(sc, q2.data(), cnt_q2++, slot, r);
        }
        q.swap(q2);
        cnt_q = cnt_q2;
    }
    uint64_t c[7] = {cnt.rays, cnt.aabb, cnt.tri, cnt.lq, cnt.laabb, cnt.ltri, cnt.hits};
    std::memcpy(cnt_out, c, sizeof c);
    if (iterations) *iterations = it;
    return 0;
}

// The record of the shadeedge chain, in the layout of rt_sample_frames_via (include/rt_hw.h):
// warm[k] polar normals are drawn before the sampler, so its cache is full at entry; out_f row = (dir, pdf,
// the light pdf alone, the next polar normal), out_i row = (status, the next engine output, the light walk's
// AABB and triangle tests).  path 0: scene_pdf<true> over a LocalStack; path 1: light_step until the walk is
// done (status -2 at 8 * n_lights + 64 steps), then scene_pdf_lp.  warm == nullptr: a cold cache everywhere.
static void samplers_row(const rtd::DevScene &sc, int path, const float *f, uint32_t seed, uint32_t warm, float *of,
                         int64_t *oi) {
    const rtv::V3 pos{f[0], f[1], f[2]}, N{f[3], f[4], f[5]}, eye{f[6], f[7], f[8]};
    rtd::Rng rng{seed, 0u, 0.f};
    if (warm) (void)rtd::rng_normal(rng);
    rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0}, c2{0, 0, 0, 0, 0, 0, 0};
    const rtv::V3 d = rtd::scene_sample(sc, pos, N, eye, f[9], rng);
    float pdf, lp = 0.f;
    int64_t status = 0;
    if (path == 0) {
        pdf = rtd::scene_pdf<true>(sc, pos, N, eye, f[9], d, cnt);
        if (sc.n_lights) lp = rtd::light_pdf<true>(sc, pos, d, c2);
    } else {
        if (sc.n_lights) {
            const rtd::Ray lr = rtd::make_ray(pos, d);   // light_pdf's Ray(point, direction)
            const float4 dq = make_float4(d.x, d.y, d.z, 0.f);
            rtd::LocalStack S;
            rtd::TravState T;
            T.acc = 0.f;
            T.sp = 0;
            S.put(T.sp++, make_uint2(0u, 0u));
            bool active = true;
            for (long long it = 0; it < 8ll * sc.n_lights + 64 && active; ++it)
                if (rtd::light_step<true>(sc, lr, T, S, cnt, &dq)) active = false;
            lp = T.acc / (float)sc.n_lights;
            if (active) status = -2;
        }
        pdf = rtd::scene_pdf_lp(sc, N, eye, f[9], d, lp);
    }
    of[0] = d.x;
    of[1] = d.y;
    of[2] = d.z;
    of[3] = pdf;
    of[4] = lp;
    of[5] = rtd::rng_normal(rng);
    oi[0] = status;
    oi[1] = rtd::rng_next(rng);
    oi[2] = cnt.laabb;
    oi[3] = cnt.ltri;
}
extern "C" void kh_sample_frames(const rt_scene_view *v, int path, int64_t n, const float *frame, const uint32_t *seed,
                                 const uint32_t *warm, float *out_f, int64_t *out_i) {
    rtd::DevScene sc = make(v);
    for (int64_t k = 0; k < n; ++k) samplers_row(sc, path, frame + 10 * k, seed[k], warm ? warm[k] : 0u, out_f + 6 * k, out_i + 4 * k);
}
// SceneDistribution sample + pdf from explicit shading frames (the sampler goldens):
// frame = (point, normal, eye, roughness2); each draw starts from Rng(seed) with an empty
// normal cache; next_out = the engine's next output after the draw (pins draws consumed).
extern "C" void kh_samplers(const rt_scene_view *v, int64_t n, const float *frame, const uint32_t *seed,
                            float *dir_out, float *pdf_out, uint32_t *next_out) {
    rtd::DevScene sc = make(v);
    for (int64_t k = 0; k < n; ++k) {
        const float *f = frame + 10 * k;
        const rtv::V3 pos{f[0], f[1], f[2]}, N{f[3], f[4], f[5]}, eye{f[6], f[7], f[8]};
        rtd::Rng rng{seed[k], 0u, 0.f};
        rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
        const rtv::V3 d = rtd::scene_sample(sc, pos, N, eye, f[9], rng);
        pdf_out[k] = rtd::scene_pdf<false>(sc, pos, N, eye, f[9], d, cnt);
        dir_out[3 * k] = d.x;
        dir_out[3 * k + 1] = d.y;
        dir_out[3 * k + 2] = d.z;
        next_out[k] = rtd::rng_next(rng);
    }
}

// What the draws of one scene_sample were, for the aimed seeds of the shadeedge `branch` class: the mixture's
// s as mixture_pick computes it, the sampler it picks, and that sampler's own draws (light: the pick's uniform,
// u and v before the fold; VNDF: the disc pairs rejected).  The draws are restated here from the same RNG
// functions; tf row = (s, pick uniform, u, v), ti row = (sampler, disc pairs rejected, engine output after
// the restated draws and one more polar normal).  The caller checks that output against kh_sample_frames'
// own: they differ only where cosine_sample retried.
extern "C" void kh_sampler_trace(int n_lights, int64_t n, const uint32_t *seed, const uint32_t *warm, float *tf, int64_t *ti) {
    for (int64_t k = 0; k < n; ++k) {
        rtd::Rng rng{seed[k], 0u, 0.f};
        if (warm && warm[k]) (void)rtd::rng_normal(rng);
        rtd::Rng probe = rng;
        const int b = rtd::mixture_pick(probe, n_lights);
        float s = (rtd::rng_uniform_m11(rng) + 1.f) * 3 * 0.5f;
        if (!n_lights) s /= 1.5f;
        float *f = tf + 4 * k;
        f[0] = s;
        f[1] = f[2] = f[3] = 0.f;
        int64_t rejected = 0;
        if (b == 0) {
            (void)rtd::sphere(rng);
        } else if (b == 1) {
            float ux, uy;
            do {
                ux = rtd::rng_uniform_m11(rng);
                uy = rtd::rng_uniform_m11(rng);
                ++rejected;
            } while (ux * ux + uy * uy > 1.f);
            --rejected;
        } else {
            f[1] = rtd::rng_uniform_m11(rng);
            f[2] = (rtd::rng_uniform_m11(rng) + 1.f) / 2;
            f[3] = (rtd::rng_uniform_m11(rng) + 1.f) / 2;
        }
        ti[3 * k] = b;
        ti[3 * k + 1] = rejected;
        (void)rtd::rng_normal(rng);
        ti[3 * k + 2] = rtd::rng_next(rng);
    }
}

// Raw sequences: kind 0 = engine outputs, 1 = uniform(-1, 1), 2 = normal(0, 1).
extern "C" void kh_rng(uint32_t seed, int kind, int n, float *out_f, uint32_t *out_u) {
    rtd::Rng rng{seed, 0u, 0.f};
    for (int k = 0; k < n; ++k) {
        if (kind == 0) out_u[k] = rtd::rng_next(rng);
        else if (kind == 1) out_f[k] = rtd::rng_uniform_m11(rng);
        else out_f[k] = rtd::rng_normal(rng);
    }
}

// div_magic (rt_wavefront.h) against `/` for divisor d: every n below 2^20, the 2^20 values
// below 2^31, the multiples of d and their neighbours up to 2^31, and `extra` seeded draws;
// returns the number of mismatches.
extern "C" int64_t kh_div_magic_check(uint32_t d, uint32_t extra) {
    uint32_t m = 0;
    int sh = 0;
    rtd::div_magic_make(d, m, sh);
    int64_t bad = 0;
    auto chk = [&](uint64_t n) {
        if (n < (1ull << 31) && (uint64_t)rtd::div_magic((int)n, m, sh) != n / d) ++bad;
    };
    for (uint64_t n = 0; n < (1u << 20); ++n) chk(n);
    for (uint64_t n = (1ull << 31) - (1u << 20); n < (1ull << 31); ++n) chk(n);
    for (uint64_t q = 1; q * d < (1ull << 31) + d && q < (1u << 22); ++q) {
        chk(q * d - 1);
        chk(q * d);
    }
    uint64_t x = 0x9e3779b97f4a7c15ull ^ d;
    for (uint32_t i = 0; i < extra; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        chk(x & 0x7fffffffu);
    }
    return bad;
}

// The options every emulated render here starts from.  accum_host.cpp, built into the same
// library, runs its passes with them too, so one setter serves both.
emu::Options kh_options;
extern "C" void kh_set_static_per_wave(int p) { kh_options.static_per_wave = p; }
extern "C" void kh_set_handoff_spread(int on) { kh_options.spread = on != 0; }
extern "C" uint64_t kh_rounds() { return kh_options.rounds; }   // main-loop rounds of the last render
extern "C" void kh_spec_prof(uint64_t *out) {   // the 16 runahead counters (rt_mega.h RT_SPEC_STAT), not reset
    std::memcpy(out, rtd::g_spec_prof, sizeof rtd::g_spec_prof);
}
extern "C" void kh_spec_stats(uint64_t *out) {   // passes, frontier jobs, runahead jobs, added, invalidations
    out[0] = kh_options.passes;
    out[1] = rtd::g_spec_prof[2];
    out[2] = rtd::g_spec_prof[3];
    out[3] = rtd::g_spec_prof[4];
    out[4] = rtd::g_spec_prof[6];
    kh_options.passes = 0;
    std::memset(rtd::g_spec_prof, 0, sizeof rtd::g_spec_prof);
}

// rt_mega_kernel on the host (mega_emu.h render_mega): the plain kernel, the runahead kernel (a
// non-counting render, as on the GPU), the hand-off from one to the other, the light-split kernel.
extern "C" int kh_render_mega(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves,
                              int shade_min, const int32_t *order, float *out, uint64_t *cnt_out) {
    return render_mega<false, false, false>(v, spp, rank, world, row_block, waves, shade_min, order, out, cnt_out, kh_options);
}
extern "C" int kh_render_mega_spec(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves,
                                   int shade_min, const int32_t *order, float *out, uint64_t *cnt_out) {
    return render_mega<false, true, false>(v, spp, rank, world, row_block, waves, shade_min, order, out, cnt_out, kh_options);
}
extern "C" int kh_render_mega_handoff(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves,
                                      int spec_waves, int shade_min, int park_below, int resume_pct,
                                      const int32_t *order, float *out, uint64_t *cnt_out, uint64_t *parked_out) {
    return render_mega_handoff<false>(v, spp, rank, world, row_block, waves, spec_waves, shade_min, park_below, resume_pct,
                                      order, out, cnt_out, parked_out, kh_options);
}
extern "C" int kh_render_mega_lsplit(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves,
                                     int shade_min, float *out, uint64_t *cnt_out) {
    return render_mega<true, false, false>(v, spp, rank, world, row_block, waves, shade_min, nullptr, out, cnt_out, kh_options);
}

// rng_skip_sample (rt_path.h, the speculative runahead's state prediction) against the
// real sample chain: for every sample of the listed pixels (parity RNG convention), the state
// the sample ends in must equal rng_skip_sample(start, v) where v is the number of path
// vertices (SceneDistribution::sample calls) of that sample.  stats: [0] samples, [1] states
// that differ, [2] samples with v == ray_depth (the runahead's prediction).
extern "C" void kh_skip_check(const rt_scene_view *v, int spp, int64_t n, const int64_t *pix, uint64_t *stats) {
    rtd::DevScene sc = make(v);
    uint64_t tot = 0, bad = 0, full = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : tot, bad, full)
    for (int64_t q = 0; q < n; ++q) {
        const int i = (int)(pix[q] % v->width), j = (int)(pix[q] / v->width);
        const uint32_t seed = (uint32_t)(j * v->width + i) % 2147483647u;
        rtd::Rng rng{seed == 0 ? 1u : seed, 0u, 0.f};
        rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
        for (int s = 0; s < spp; ++s) {
            const rtd::Rng start = rng;
            const float ox = rtd::rng_offset(rng), oy = rtd::rng_offset(rng);
            rtd::Ray r = rtd::camera_ray(sc, i, j, ox, oy);
            rtd::PathRec P;
            int nv = 0, power = sc.ray_depth;
            while (power > 0) {   // trace_sample (rt_path.h), keeping the vertex count
                power -= 1;
                rtd::Hit hit;
                const bool ok = rtd::closest_hit<false>(sc, r, hit, cnt);
                if (!(ok && hit.t < sc.max_distance)) break;
                if (!rtd::shade_hit<false>(sc, r, hit, rng, cnt, P, nv)) break;
            }
            rtd::Rng pred = start;
            rtd::rng_skip_sample(pred, nv, sc.n_lights);
            ++tot;
            full += nv == sc.ray_depth;
            uint32_t a, b;
            std::memcpy(&a, &pred.saved, 4);
            std::memcpy(&b, &rng.saved, 4);
            bad += !(pred.x == rng.x && pred.saved_avail == rng.saved_avail && a == b);
        }
    }
    stats[0] = tot;
    stats[1] = bad;
    stats[2] = full;
}

// Per-sample vertex count and traversal cost of the listed pixels (parity RNG convention):
// the data the runahead's prediction of v is measured on (tools/runahead_predict.py).
// nv_out[q*spp + s] = vertices of sample s of pixel q, cost_out[q*spp + s] = its box + triangle tests.
extern "C" void kh_v_trace(const rt_scene_view *v, int spp, int64_t n, const int64_t *pix, uint8_t *nv_out,
                           uint32_t *cost_out) {
    rtd::DevScene sc = make(v);
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t q = 0; q < n; ++q) {
        const int i = (int)(pix[q] % v->width), j = (int)(pix[q] / v->width);
        const uint32_t seed = (uint32_t)(j * v->width + i) % 2147483647u;
        rtd::Rng rng{seed == 0 ? 1u : seed, 0u, 0.f};
        for (int s = 0; s < spp; ++s) {
            rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
            const float ox = rtd::rng_offset(rng), oy = rtd::rng_offset(rng);
            rtd::Ray r = rtd::camera_ray(sc, i, j, ox, oy);
            rtd::PathRec P;
            int nv = 0, power = sc.ray_depth;
            while (power > 0) {
                power -= 1;
                rtd::Hit hit;
                const bool ok = rtd::closest_hit<true>(sc, r, hit, cnt);
                if (!(ok && hit.t < sc.max_distance)) break;
                if (!rtd::shade_hit<true>(sc, r, hit, rng, cnt, P, nv)) break;
            }
            nv_out[q * spp + s] = (uint8_t)nv;
            cost_out[q * spp + s] = (uint32_t)(cnt.aabb + cnt.tri + cnt.laabb + cnt.ltri);
        }
    }
}

// box_pair_hit (rt_wavefront.h) against box_hit_pt on each box of the pair, over `n`
// random cases drawn from a small set of special values (planes through the origin,
// signed zeros, infinities, NaN, inverted boxes) mixed with ordinary floats.  Returns the
// number of mismatching cases (hit flags, far-box inside flag, far-box entry distance bits;
// any NaN distance equals any other: traversal only compares it).
extern "C" long long kh_box_pair_check(long long n, uint32_t seed) {
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const float specials[] = {0.f, -0.f, 1.f, -1.f, 0.5f, -2.f, 1e-30f, -1e-30f, 1e30f, -1e30f, 1e-45f,
                              __builtin_inff(), -__builtin_inff(), __builtin_nanf("")};
    auto val = [&]() -> float {
        const uint64_t r = next();
        if ((r & 3) == 0) return specials[(r >> 8) % (sizeof specials / sizeof specials[0])];
        return ((float)((r >> 16) & 0xffff) / 32768.f - 1.f) * 4.f;
    };
    long long bad = 0;
    for (long long k = 0; k < n; ++k) {
        rtd::Ray r;
        r.o = rtv::V3{val(), val(), val()};
        r.d = rtv::V3{val(), val(), val()};
        r.inv = rtv::V3{1.f / r.d.x, 1.f / r.d.y, 1.f / r.d.z};
        rtd::NodeRec L{}, R{};
        for (int i = 0; i < 3; ++i) {
            const float a = val(), b = val(), c = val(), e = val();
            const bool inv_box = (next() & 15) == 0;   // occasionally inverted
            L.mn[i] = inv_box ? std::max(a, b) : std::min(a, b);
            L.mx[i] = inv_box ? std::min(a, b) : std::max(a, b);
            R.mn[i] = std::min(c, e);
            R.mx[i] = (next() & 7) == 0 ? R.mn[i] : std::max(c, e);   // flat boxes too
            const float oi = i == 0 ? r.o.x : (i == 1 ? r.o.y : r.o.z);
            if ((next() & 7) == 0 && oi <= R.mx[i]) R.mn[i] = oi;   // plane through the origin
        }
        const bool lf = next() & 1;
        float cL[3], cR[3], cF[3];
        bool inL, inR, hL, hR, inF;
        const bool wL = rtd::box_hit_pt(L.mn, L.mx, r, cL, inL);
        const bool wR = rtd::box_hit_pt(R.mn, R.mx, r, cR, inR);
        rtd::box_pair_hit(L, R, r, lf, hL, hR, cF, inF);
        bool ok = wL == hL && wR == hR && inF == (lf ? inR : inL);
        const bool far_hit = lf ? wR : wL;
        if (ok && far_hit) {   // the entry distance is only used for a hit far box
            const float want = rtd::box_dist(lf ? cR : cL, lf ? inR : inL, r), got = rtd::box_dist(cF, inF, r);
            uint32_t a, b;
            std::memcpy(&a, &want, 4);
            std::memcpy(&b, &got, 4);
            ok = ok && (a == b || (want != want && got != got));   // (traversal only compares it)
        }
        bad += !ok;
    }
    return bad;
}

// rt_path.h unorm8 (the device's computed linear texel decode) against (float)b / 255.f for
// every byte, and rt_mega.h's packed LDS RNG word round trip on the state's extremes; returns
// the mismatches.
extern "C" long long kh_decode_check() {
    long long bad = 0;
    for (uint32_t b = 0; b < 256; ++b) {
        const float a = rtd::unorm8(b), want = (float)b / 255.f;
        bad += std::memcmp(&a, &want, 4) != 0;
    }
    const uint32_t xs[] = {0u, 1u, 2u, 48271u, 0x3fffffffu, 0x7ffffffdu, 0x7ffffffeu};
    for (uint32_t x : xs)
        for (uint32_t f = 0; f < 2; ++f) {
            uint32_t ux, uf;
            rtd::rng_word_unpack(rtd::rng_word_pack(x, f), ux, uf);
            bad += (ux != x) | (uf != f);
        }
    return bad;
}
