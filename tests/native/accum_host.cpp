// accum_host.cpp — TEST ONLY: the accumulator's passes (rt_mega.h, chain buffer) on the host.
// kernel_host.cpp's emulation of rt_mega_kernel with the CHAIN instantiation's changes, as
// rt_device.hip makes them: a claimed pixel starts from its record (mega_assign_chain), a wave
// entering its tail takes X_f from the record (spec_convert_chain), and the three pixel-done
// sites store the record back (mega_shade, spec_job_end, spec_manage, all with CHAIN = true).
// The queue block is the kernel's (rt_mega.h QueueWord): kQueueRender the render's claim counter,
// kQueueResume the resume launch's, kChainWord the chain buffer's address.
#include "kernel_host.cpp"

template <bool SPEC>
static int render_mega_chain(const rt_scene_view *v, int spp, int rank, int world, int row_block, int waves,
                             int shade_min, uint4 *chain, float *out) {
    rtd::DevScene sc = make(v);
    sc.n_tris = (int)v->n_tris;
    sc.n_nodes = (int)v->n_nodes;
    int64_t rows = 0;
    for (int r = 0; r < v->height; ++r)
        if ((r / row_block) % world == rank) ++rows;
    const long long n = (long long)rows * v->width;
    const rtd::ShardGeom g = rtd::shard_geom(v->width, rank, world, row_block, n);
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
    using Lane = std::conditional_t<SPEC, rtd::MegaLane, rtd::MegaLaneU>;
    std::vector<Lane> lanes((size_t)waves * 64);
    std::vector<std::vector<uint2>> stacks((size_t)waves * 64, std::vector<uint2>(rtd::kStack));
    for (auto &L : lanes) { L.pix = -1; L.state = rtd::M_IDLE; }
    std::vector<char> exhausted(waves, 0), done(waves, 0), tail(waves, 0), wave_room(waves, 0);
    rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
    unsigned long long qblock[rtd::kQueueWords] = {};
    qblock[rtd::kChainWord] = (unsigned long long)(uintptr_t)chain;
    unsigned long long &queue = qblock[rtd::kQueueRender];
    rtd::SpecClaim claim{qblock + rtd::kQueueResume, 0, 0, nullptr, 0, false, nullptr};
    const bool parking = !SPEC && g_park_below > 0, resuming = SPEC && g_resume_pct > 0;
    std::vector<char> park(waves, 0);
    if (parking) g_park_list.assign((size_t)2 * waves * 64, make_uint4(rtd::kNoPark, rtd::kNoPark, rtd::kNoPark, rtd::kNoPark));
    int res_per = 0;
    long long res_n = 0;
    std::vector<char> xk((size_t)waves * 64, 0);
    std::vector<rtd::Rng> xs((size_t)waves * 64);
    if (resuming) {   // (slot order: the spread is the one-shot emulation's, kernel_host.cpp)
        res_n = (long long)g_park_list.size() / 2;
        const long long dealt = (res_n * g_resume_pct + 99) / 100;
        res_per = (int)std::min<long long>(64, std::max<long long>(1, (dealt + waves - 1) / waves));
        claim = rtd::SpecClaim{qblock + rtd::kQueueResume, (long long)waves * res_per, res_n, g_park_list.data(), res_per,
                               (long long)waves * res_per < res_n, nullptr};
    }
    int live = waves;
    unsigned long long rounds = 0;
    while (live > 0) {
        if (++rounds > 50000000ull) return -7;
        for (int w = 0; w < waves; ++w) {
            if (done[w]) continue;
            Lane *W = &lanes[(size_t)w * 64];
            if (parking && park[w])
                for (int l = 0; l < 64; ++l)
                    if (W[l].state == rtd::M_IDLE && W[l].pix >= 0) {
                        rtd::g_mega_slot = (long long)w * 64 + l;
                        rtd::park_pixel(g_park_list.data(), (long long)w * 64 + l, W[l].pix, rtd::lane_ctr(W[l]).s,
                                        rtd::lane_rng(W[l]), rtd::lane_sum(W[l]));
                        W[l].pix = -1;
                    }
            if (!exhausted[w] && resuming) {
                for (int l = 0; l < res_per; ++l) {
                    const long long p = (long long)w * res_per + l;
                    if (p >= res_n) break;
                    const rtd::Parked q = rtd::parked_item(g_park_list.data(), claim.ridx, p);
                    if (q.pix == rtd::kNoPark) continue;
                    rtd::g_mega_slot = (long long)w * 64 + l;
                    rtd::mega_resume(W[l], sc, g, q, root);
                    xk[(size_t)w * 64 + l] = 1;
                    xs[(size_t)w * 64 + l] = q.x;
                }
                exhausted[w] = 1;
            }
            if (!exhausted[w]) {
                uint64_t m = 0;
                for (int l = 0; l < 64; ++l) if (W[l].pix < 0) m |= 1ull << l;
                if (m) {
                    const long long base = queue;
                    const int cm = __builtin_popcountll(m);
                    queue += cm;
                    for (int l = 0; l < 64; ++l) {
                        if (!(m >> l & 1)) continue;
                        const long long p = base + __builtin_popcountll(m & ((1ull << l) - 1ull));
                        rtd::g_mega_slot = (long long)w * 64 + l;
                        if (p < n) rtd::mega_assign_chain<false>(W[l], sc, g, (int)p, root, cnt, rtd::chain_of(qblock));
                    }
                    if (base + cm >= n) exhausted[w] = 1;
                }
            }
            if constexpr (SPEC) {
            if (exhausted[w] && !tail[w]) {
                const rtd::SpecView V{(uint4 *)st.mid, st.lanes, (long long)w * 64};
                for (int l = 0; l < 64; ++l) {
                    rtd::g_mega_slot = (long long)w * 64 + l;
                    if (resuming) rtd::spec_convert(W[l], sc, g, V, l, xk[(size_t)w * 64 + l] != 0, xs[(size_t)w * 64 + l]);
                    else rtd::spec_convert_chain(W[l], sc, g, V, l, rtd::chain_of(qblock));
                }
                rtd::g_mega_slot = (long long)w * 64;
                rtd::spec_hint_take();
                tail[w] = 1;
                wave_room[w] = 0;
            }
            if (tail[w]) {
                rtd::g_mega_slot = (long long)w * 64;
                wave_room[w] |= rtd::spec_hint_take();
                bool fresh = false, idle = false;
                for (int l = 0; l < 64; ++l) {
                    fresh |= W[l].state == rtd::M_DONE_NEW;
                    idle |= W[l].state == rtd::M_IDLE;
                }
                if (fresh || (wave_room[w] && idle))
                    wave_room[w] = rtd::spec_manage<true>(rtd::SpecLanes{W}, sc, g,
                                                          rtd::SpecView{(uint4 *)st.mid, st.lanes, (long long)w * 64}, spp,
                                                          out, root, claim);
            }
            }
            bool any = false;
            int nr = 0, nt = 0;
            for (int l = 0; l < 64; ++l) {
                any |= tail[w] ? W[l].state != rtd::M_IDLE : W[l].pix >= 0;
                nr += W[l].state == rtd::M_READY;
                nt += W[l].state == rtd::M_TRAV;
            }
            if (!any) {
                done[w] = 1;
                --live;
                continue;
            }
            if (parking && exhausted[w] && !park[w]) {
                int held = 0;
                for (int l = 0; l < 64; ++l) held += W[l].pix >= 0;
                park[w] = held < g_park_below;
            }
            const bool shade_now = nr > 0 && (nr >= shade_min || nt == 0);
            for (int l = 0; l < 64; ++l) {
                rtd::ArrayStack S{stacks[(size_t)w * 64 + l].data()};
                rtd::g_mega_slot = (long long)w * 64 + l;
                rtd::mega_iterate<false, decltype(S), decltype(nodes), false, false, true>(
                    W[l], shade_now, sc, g, st, spp, out, nullptr, root, S, nodes, cnt, (bool)tail[w],
                    parking && park[w], qblock);
            }
        }
    }
    return 0;
}

// Fresh records of the shard's n pixels (rt_chain_init_kernel).
extern "C" void kh_accum_init(const rt_scene_view *v, int rank, int world, int row_block, uint32_t *chain) {
    rtd::DevScene sc = make(v);
    int64_t rows = 0;
    for (int r = 0; r < v->height; ++r)
        if ((r / row_block) % world == rank) ++rows;
    const long long n = (long long)rows * v->width;
    const rtd::ShardGeom g = rtd::shard_geom(v->width, rank, world, row_block, n);
    for (long long p = 0; p < n; ++p) rtd::chain_init((uint4 *)chain, sc, g, (int)p);
}

// One pass to absolute sample s1 over the records in `chain` (8 words per shard pixel).
// mode 0: the plain emulation; 1: the runahead emulation; 2: the hand-off (the plain emulation
// parks its sparse tail waves below park_below held pixels, the runahead emulation resumes).
extern "C" int kh_accum_pass(const rt_scene_view *v, int s1, int rank, int world, int row_block, int waves,
                             int shade_min, int mode, int park_below, uint32_t *chain, float *out,
                             uint64_t *parked_out) {
    uint4 *c = (uint4 *)chain;
    if (mode == 0) return render_mega_chain<false>(v, s1, rank, world, row_block, waves, shade_min, c, out);
    if (mode == 1) return render_mega_chain<true>(v, s1, rank, world, row_block, waves, shade_min, c, out);
    g_park_below = park_below;
    int rc = render_mega_chain<false>(v, s1, rank, world, row_block, waves, shade_min, c, out);
    g_park_below = 0;
    if (rc) return rc;
    uint64_t parked = 0;
    for (size_t k = 0; k < g_park_list.size(); k += 2) parked += g_park_list[k].x != rtd::kNoPark;
    if (parked_out) *parked_out = parked;
    g_resume_pct = 100;
    rc = render_mega_chain<true>(v, s1, rank, world, row_block, waves, shade_min, c, out);
    g_resume_pct = 0;
    return rc;
}
