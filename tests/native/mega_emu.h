// mega_emu.h — TEST ONLY: the one host emulation of rt_mega_kernel's wave loop (rt_mega_device.h),
// over the kernel's own per-lane source (raytracing-hw_amd/csrc/rt_mega.h) compiled for the
// host.  kernel_host.cpp (the one-shot renders) and accum_host.cpp (the accumulator's passes)
// are entry points over it; the schedule rules it shares with the kernel and the launch plan
// are rt_launch_plan.h's (resume_deal, shade_rule, park_rule).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../raytracing-hw_amd/csrc/rt_mega.h"
#include "../../raytracing-hw_amd/csrc/rt_bvh_layout.h"
#include "../../raytracing-hw_amd/csrc/rt_launch_plan.h"
#include "../../include/rt_hw.h"

namespace emu {

// The device's view of the scene, over the host arrays of `v`.
inline rtd::DevScene make(const rt_scene_view *v) {
    rtd::DevScene s{};
    // the device copy of the triangles is padded (a leaf lane reads 4 x 16 B of its last
    // triangle: its 3 records and the next one's first)
    static thread_local std::vector<float> tri;
    tri.assign(v->tri, v->tri + 12 * (size_t)v->n_tris);
    tri.resize(tri.size() + 12, 0.f);
    s.tri = (const float4 *)tri.data();
    s.tri_attr = (const float4 *)v->tri_attr;
    s.tri_tan = (const float4 *)v->tri_tan;
    s.node = (const float4 *)v->node;
    s.light = (const float4 *)v->light;
    s.light_node = (const float4 *)v->light_node;
    s.mesh_f = v->mesh_f;
    s.mesh_tex = v->mesh_tex;
    s.mesh_nt = v->mesh_normal_transform;
    s.tex_info = (const uint4 *)v->tex_info;
    s.texels = (const uint32_t *)v->texels;
    static float lut[512];
    static bool lut_ready = false;
    if (!lut_ready) { rtd::fill_decode_lut(lut); lut_ready = true; }
    s.lut = lut;
    s.n_tris = (int)v->n_tris;
    s.n_nodes = (int)v->n_nodes;
    s.n_lights = (int)v->n_lights;
    s.ray_depth = v->ray_depth;
    s.max_distance = v->max_distance;
    s.width = v->width;
    s.height = v->height;
    s.fwidth = (float)v->width;
    s.fheight = (float)v->height;
    std::memcpy(s.cam_pos, v->cam_pos, sizeof s.cam_pos);
    std::memcpy(s.cam_axes, v->cam_axes, sizeof s.cam_axes);
    std::memcpy(s.tan_fov, v->tan_half_fov, sizeof s.tan_fov);
    return s;
}

// Rank `rank` of `world` renders the row blocks r with r % world == rank: its pixel count and
// the geometry the kernels map shard pixels to the frame with.
struct Shard {
    long long n;
    rtd::ShardGeom g;
};
inline Shard shard_of(const rt_scene_view *v, int rank, int world, int row_block) {
    long long rows = 0;
    for (int r = 0; r < v->height; ++r)
        if ((r / row_block) % world == rank) ++rows;
    const long long n = rows * v->width;
    return {n, rtd::shard_geom(v->width, rank, world, row_block, n)};
}

// What a render takes besides its arguments (rt_mega_kernel's `mode`, its queue block's
// addresses, the harness's study knobs) and what it reports besides the image.
struct Options {
    // Hand-off (rt_device.hip launch_handoff): the plain emulation parks (park_below > 0) into
    // park_list by lane slot; the runahead emulation resumes that list (resume_pct > 0).
    int park_below = 0, resume_pct = 0;
    std::vector<uint4> park_list;
    // RT_HANDOFF_SPREAD: the resume deals the slots heaviest first (work left; the harness has
    // no pre-pass estimate, so samples left), spread one per wave; else in slot order
    bool spread = true;
    int static_per_wave = 0;   // > 0: no queue; wave w takes items [w*P, w*P+P) (study of spare lanes)
    uint4 *chain = nullptr;    // CHAIN: the accumulator's records (rt_mega.h, chain buffer)
    uint64_t rounds = 0;       // out: main-loop rounds (one iteration of every live wave) of the last render
    uint64_t passes = 0;       // out: runahead management passes, added up over the renders
};

inline uint64_t parked_count(const Options &o) {
    uint64_t parked = 0;
    for (size_t k = 0; k < o.park_list.size(); k += 2) parked += o.park_list[k].x != rtd::kNoPark;
    return parked;
}

// A schedule that stops draining: report (with the runahead records still active), do not hang
// the test.
template <class Lane>
inline void report_stuck(unsigned long long rounds, int live, int waves, const rtd::WfState &st, const std::vector<Lane> &lanes,
                         bool spec) {
    std::fprintf(stderr, "render_mega: no progress after %llu rounds, %d waves live\n", rounds, live);
    for (int w = 0; spec && w < waves; ++w) {
        const rtd::SpecView V{(uint4 *)st.mid, st.lanes, (long long)w * 64};
        for (int l = 0; l < 64; ++l) {
            const uint4 a = *V.w(0, l), b = *V.w(1, l), c = *V.w(2, l), d = *V.w(3, l);
            if (b.w & rtd::kRecActive)
                std::fprintf(stderr, " w%d rec %d: pix %u f %u n %u e %u meta %u tab %08x%08x | lane state %d\n", w, l,
                             a.x, a.y, a.z, a.w, b.w, d.w, c.w, lanes[(size_t)w * 64 + l].state);
        }
    }
}

// rt_mega_kernel (kernel 0): `waves` waves of 64 lanes, round-robin one main-loop iteration at a
// time, sharing the pixel queue, with the kernel's shade_min decision.
// LSPLIT: the light-split kernel (light-pdf walk as lane states M_LTRAV / M_LREADY).
// order (may be NULL): queue item p renders shard pixel order[p], as in the ordered render.
// SPEC: the speculative sample runahead of the waves' tails (rt_mega.h spec_*), driven here
// by host loops over the wave's lanes where the kernel uses ballots (rt_mega.h spec_manage).
// CHAIN: a pass of the accumulator to absolute sample `spp`, as rt_device.hip makes it: a
// claimed pixel starts from its record (mega_assign_chain), a wave entering its tail takes X_f
// from the record (spec_convert_chain), and the three pixel-done sites store the record back
// (mega_shade, spec_job_end, spec_manage, all with CHAIN = true).
// The render counts (COUNT) unless it is SPEC, parks or is a CHAIN pass, as on the GPU.
template <bool LSPLIT, bool SPEC, bool CHAIN>
int render_mega(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves, int shade_min,
                const int32_t *order, float *out, uint64_t *cnt_out, Options &o) {
    constexpr bool kCount = !SPEC && !CHAIN;
    const rtd::DevScene sc = make(v);
    const Shard sh = shard_of(v, rank, world, row_block);
    const long long n = sh.n;
    const rtd::ShardGeom g = sh.g;
    const int D = v->ray_depth;
    const long long slots = std::max<long long>(n, (long long)waves * 64);
    std::vector<float4> ab((size_t)2 * slots * D);
    std::vector<float> cv((size_t)slots * D);
    rtd::WfState st{};
    st.n = n;
    st.D = D;
    st.rec_ab = ab.data();
    st.rec_c = cv.data();
    st.lanes = (long long)waves * 64;
    std::vector<float4> mid((size_t)5 * st.lanes);
    st.mid = mid.data();
    const rtd::NodeRec root = rtd::load_node(rtd::mega_nodes(sc), 0);
    const rtd::GlobalNodes nodes{sc.node};
    // lane state as in rt_mega_device.h: TravState for the runahead kernel, TravStateU otherwise
    using Lane = std::conditional_t<SPEC, rtd::MegaLane, rtd::MegaLaneU>;
    std::vector<Lane> lanes((size_t)waves * 64);
    std::vector<std::vector<uint2>> stacks((size_t)waves * 64, std::vector<uint2>(rtd::kStack));
    for (auto &L : lanes) { L.pix = -1; L.state = rtd::M_IDLE; }
    std::vector<char> exhausted(waves, 0), done(waves, 0), tail(waves, 0), wave_room(waves, 0);
    rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
    // the kernel's queue block (rt_mega.h QueueWord): kQueueRender the render's claim counter,
    // kQueueResume the resume launch's, kChainWord the chain buffer's address
    unsigned long long qblock[rtd::kQueueWords] = {};
    qblock[rtd::kChainWord] = (unsigned long long)(uintptr_t)o.chain;
    unsigned long long &queue = qblock[rtd::kQueueRender];
    rtd::SpecClaim claim{qblock + rtd::kQueueResume, 0, 0, nullptr, 0, false, nullptr};
    // hand-off: parking (plain) / resuming (runahead) as rt_mega_kernel's `mode`
    const bool parking = !SPEC && !LSPLIT && o.park_below > 0, resuming = SPEC && o.resume_pct > 0;
    std::vector<char> park(waves, 0);
    if (parking) o.park_list.assign((size_t)2 * waves * 64, make_uint4(rtd::kNoPark, rtd::kNoPark, rtd::kNoPark, rtd::kNoPark));
    int res_per = 0;
    long long res_n = 0;
    std::vector<char> xk((size_t)waves * 64, 0);
    std::vector<rtd::Rng> xs((size_t)waves * 64);
    std::vector<int> ridx;
    if (resuming) {
        res_n = (long long)o.park_list.size() / 2;
        res_per = (int)rtp::resume_deal(res_n, o.resume_pct, waves).per;
        claim = rtd::SpecClaim{qblock + rtd::kQueueResume, (long long)waves * res_per, res_n, o.park_list.data(), res_per,
                               (long long)waves * res_per < res_n, nullptr};
        if (o.spread) {   // rt_park_keys_kernel, the descending sort, rt_order_spread_kernel
            std::vector<std::pair<unsigned, int>> kv((size_t)res_n);
            for (long long i = 0; i < res_n; ++i) {
                const rtd::Parked q = rtd::parked(o.park_list.data(), i);
                kv[(size_t)i] = {q.pix == rtd::kNoPark ? 0u : (unsigned)(spp - (int)q.s), (int)i};
            }
            std::stable_sort(kv.begin(), kv.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
            const long long per = res_per, m = std::min<long long>(res_n, (long long)waves * per), a = m / per, b = m % per;
            ridx.resize((size_t)res_n);
            for (long long q = 0; q < res_n; ++q) {
                long long r = q;
                if (q < m) {
                    const long long gi = q / per, j = q % per;
                    r = j * a + (j < b ? j : b) + gi;
                }
                ridx[(size_t)q] = kv[(size_t)r].second;
            }
            claim.ridx = ridx.data();
        }
    }
    int live = waves;
    o.rounds = 0;
    while (live > 0) {
        if (++o.rounds > 50000000ull) {
            report_stuck(o.rounds, live, waves, st, lanes, SPEC);
            return -7;
        }
        for (int w = 0; w < waves; ++w) {
            if (done[w]) continue;
            Lane *W = &lanes[(size_t)w * 64];
            const long long slot0 = (long long)w * 64;   // the wave's first lane slot (rt_mega.h mega_slot)
            if (parking && park[w])   // lanes idle with a pixel park it (at their lane slot)
                for (int l = 0; l < 64; ++l)
                    if (W[l].state == rtd::M_IDLE && W[l].pix >= 0) {
                        rtd::g_mega_slot = slot0 + l;
                        rtd::park_pixel(o.park_list.data(), slot0 + l, W[l].pix, rtd::lane_ctr(W[l]).s, rtd::lane_rng(W[l]),
                                        rtd::lane_sum(W[l]));
                        W[l].pix = -1;
                    }
            if (!exhausted[w] && resuming) {   // the park list's slots, res_per per wave
                for (int l = 0; l < res_per; ++l) {
                    const long long p = (long long)w * res_per + l;
                    if (p >= res_n) break;
                    const rtd::Parked q = rtd::parked_item(o.park_list.data(), claim.ridx, p);
                    if (q.pix == rtd::kNoPark) continue;
                    rtd::g_mega_slot = slot0 + l;
                    rtd::mega_resume(W[l], sc, g, q, root);
                    xk[(size_t)slot0 + l] = 1;
                    xs[(size_t)slot0 + l] = q.x;
                }
                exhausted[w] = 1;
            }
            // a queue item to a lane: a fresh pixel, or (CHAIN) the pixel from its record
            auto assign = [&](int l, long long p) {
                if (p >= n) return;
                rtd::g_mega_slot = slot0 + l;
                const int pix = order ? order[p] : (int)p;
                if constexpr (CHAIN) rtd::mega_assign_chain<kCount>(W[l], sc, g, pix, root, cnt, rtd::chain_of(qblock));
                else rtd::mega_assign<kCount>(W[l], sc, g, pix, root, cnt);
            };
            if (!exhausted[w] && o.static_per_wave > 0) {   // static allotment: wave w renders items [w*P, w*P+P)
                for (int l = 0; l < 64 && l < o.static_per_wave; ++l) assign(l, (long long)w * o.static_per_wave + l);
                exhausted[w] = 1;
            }
            if (!exhausted[w]) {   // lanes without work take the next items (one claim per wave)
                uint64_t m = 0;
                for (int l = 0; l < 64; ++l) if (W[l].pix < 0) m |= 1ull << l;
                if (m) {
                    const long long base = queue;
                    const int cm = __builtin_popcountll(m);
                    queue += cm;
                    for (int l = 0; l < 64; ++l)
                        if (m >> l & 1) assign(l, base + __builtin_popcountll(m & ((1ull << l) - 1ull)));
                    if (base + cm >= n) exhausted[w] = 1;
                }
            }
            if constexpr (SPEC) {
                const rtd::SpecView V{(uint4 *)st.mid, st.lanes, slot0};
                if (exhausted[w] && !tail[w]) {   // the wave enters its tail
                    for (int l = 0; l < 64; ++l) {
                        rtd::g_mega_slot = slot0 + l;
                        if (CHAIN && !resuming) rtd::spec_convert_chain(W[l], sc, g, V, l, rtd::chain_of(qblock));
                        else rtd::spec_convert(W[l], sc, g, V, l, xk[(size_t)slot0 + l] != 0, xs[(size_t)slot0 + l]);
                    }
                    rtd::g_mega_slot = slot0;
                    rtd::spec_hint_take();
                    tail[w] = 1;
                    wave_room[w] = 0;
                }
                if (tail[w]) {
                    rtd::g_mega_slot = slot0;
                    wave_room[w] |= rtd::spec_hint_take();
                    bool fresh = false, idle = false;
                    for (int l = 0; l < 64; ++l) {
                        fresh |= W[l].state == rtd::M_DONE_NEW;
                        idle |= W[l].state == rtd::M_IDLE;
                    }
                    if (fresh || (wave_room[w] && idle)) {
                        ++o.passes;
                        wave_room[w] = rtd::spec_manage<CHAIN>(rtd::SpecLanes{W}, sc, g, V, spp, out, root, claim);
                    }
                }
            }
            bool any = false;
            int nr = 0, nt = 0, held = 0;
            for (int l = 0; l < 64; ++l) {
                any |= tail[w] ? W[l].state != rtd::M_IDLE : W[l].pix >= 0;
                nr += W[l].state == rtd::M_READY || (LSPLIT && W[l].state == rtd::M_LREADY);
                nt += W[l].state == rtd::M_TRAV || (LSPLIT && W[l].state == rtd::M_LTRAV);
                held += W[l].pix >= 0;
            }
            if (!any) {
                done[w] = 1;
                --live;
                continue;
            }
            if (parking && exhausted[w] && !park[w]) park[w] = rtp::park_rule(held, o.park_below);
            const bool shade_now = rtp::shade_rule(nr, nt, shade_min);
            for (int l = 0; l < 64; ++l) {
                rtd::ArrayStack S{stacks[(size_t)slot0 + l].data()};
                rtd::g_mega_slot = slot0 + l;
                if (kCount && !parking)
                    rtd::mega_iterate<kCount, decltype(S), decltype(nodes), false, LSPLIT, CHAIN>(
                        W[l], shade_now, sc, g, st, spp, out, nullptr, root, S, nodes, cnt, (bool)tail[w], false, qblock);
                else
                    rtd::mega_iterate<false, decltype(S), decltype(nodes), false, LSPLIT, CHAIN>(
                        W[l], shade_now, sc, g, st, spp, out, nullptr, root, S, nodes, cnt, (bool)tail[w],
                        parking && park[w], qblock);
            }
        }
    }
    if (cnt_out) {
        const uint64_t c[7] = {cnt.rays, cnt.aabb, cnt.tri, cnt.lq, cnt.laabb, cnt.ltri, cnt.hits};
        std::memcpy(cnt_out, c, sizeof c);
    }
    return 0;
}

// Hand-off (rt_device.hip launch_handoff): the plain emulation over `waves` waves parks its
// sparse tail waves (fewer than park_below pixels held once the queue is empty), then the
// runahead emulation over `spec_waves` waves resumes the park list (resume_pct percent dealt at
// its start).  A non-counting render (cnt_out: the counters of the plain part only).
template <bool CHAIN>
int render_mega_handoff(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves, int spec_waves,
                        int shade_min, int park_below, int resume_pct, const int32_t *order, float *out, uint64_t *cnt_out,
                        uint64_t *parked_out, Options &o) {
    o.park_below = park_below;
    int rc = render_mega<false, false, CHAIN>(v, spp, rank, world, row_block, waves, shade_min, order, out, cnt_out, o);
    o.park_below = 0;
    if (rc) return rc;
    if (parked_out) *parked_out = parked_count(o);
    o.resume_pct = resume_pct;
    rc = render_mega<false, true, CHAIN>(v, spp, rank, world, row_block, spec_waves, shade_min, nullptr, out, nullptr, o);
    o.resume_pct = 0;
    return rc;
}

}  // namespace emu
