// rt_mega_device.h — the lane-resident kernel (kernel 0, rt_mega.h: every lane runs whole pixels;
// traversal one unit per iteration, shading batched per wave, READY lanes waiting for
// MegaCfg::shade_min of them or for no lane left traversing): the tuned constants of its families
// with their measurements, MegaCfg (what one instantiation reads of them), rt_mega_kernel
// and the kernel table generated from rt_launch_plan.h's kVariants.  Included by rt_device.hip in
// the middle of the file (after the scene and HIP_TRY, which the diagnostics build's
// rt_mega_prof.h uses), so the build stays one translation unit.  The launches (launch(), the
// order pre-pass, the hand-off) and the fold kernels stay in rt_device.hip.

// Tuned constants of the default kernel (measured values in DESIGN.md §5-6).
#ifndef RT_MEGA_WPE
#define RT_MEGA_WPE 5
#endif
// The runahead instantiation runs shards of at most kSpecPixelsPerLane (2) pixels per lane
// (an 8-way shard of the headline: 1013 blocks, 4 waves per SIMD, one pixel per lane; a
// 4-way shard two): 128 VGPRs instead of 96 keep its management pass from spilling the loop.
#ifndef RT_SPEC_WPE
#define RT_SPEC_WPE 4
#endif
#ifndef RT_SHADE_MIN
#define RT_SHADE_MIN 48
#endif
// The runahead kernel (4- and 8-way shards) shades at 40 READY lanes: its waves thin out
// early, and a heavy chain's lane waits less for its batch than at the plain kernel's 48.
// Round 3 (window 3): slowest 8-way shard 207.5-207.7 ms at 40 against 208.6-211.7 at 32 and
// 214.8 at 24, 4-way 346-347 vs 352-354 (profiles/r03_ab.jsonl r03ah, r03ai).  Round 2: 294 ms
// at 32 against 297-299 at 48 (profiles/r02_tail_ab.jsonl).
// Round 5, with the runahead priority (rt_mega.h RT_SPEC_PRIO): 48 READY lanes, 8-way shards
// 187.2 max / 185.6 mean ms against 188.2-188.5 / 186.9-187.5 at 40 (profiles/r05f_prio_variants_ab.jsonl).
// Round 6, with leaf deferral (rt_wavefront.h RT_LEAF_DEFER): 44 READY lanes, 12 coop leaf
// records and at most 4 deferrals in a row, slowest 8-way shard 174.4-175.8 / mean 173.2-173.7
// ms against 176.1-176.5 / 174.4-174.9 at 48, 16 and 3 (profiles/r06w_spec_tuning_ab.jsonl,
// three runs each; 52 lanes 179.6-179.8 in r06v).
#ifndef RT_SPEC_SHADE_MIN
#define RT_SPEC_SHADE_MIN 44
#endif
// RT_PACK_TRAV: through a shading pass, a lane that does not shade holds its traversal phase,
// stack depth and state packed in one register (the loop body below).  With RT_TID_REMAT
// (rt_mega.h) the plain kernel spills 16 VGPRs instead of 33 and writes 0.11 instead of
// 0.37 TB per frame (WRITE_SIZE: 53 instead of 178 B per ray); frame 1038-1041 ms against
// 1093-1094 (profiles/r05n_ab.jsonl).  0: A/B.
#ifndef RT_PACK_TRAV
#define RT_PACK_TRAV 1
#endif
constexpr bool kPackTrav = RT_PACK_TRAV != 0;
#ifndef RT_INV_RECOMPUTE
#define RT_INV_RECOMPUTE 1
#endif
constexpr bool kInvRecompute = RT_INV_RECOMPUTE != 0;
// Traversal iterations between two shading passes run as an inner loop of their own (no pixel
// claim, runahead pass or schedule decision per iteration), one cooperative step each
// (rt_wavefront.h trav_step_coop: leaf work spread over the wave).  The lane-resident
// kernel's traversal state shares the node and leaf fields (rt_wavefront.h TravStateU; the
// runahead kernel keeps TravState).
// Leaf lanes a coop step serves (32 B of LDS per wave each).  The plain kernel's block is at
// 30 KB and must stay within 32 KB minus what the runtime keeps, for 5 blocks per CU: 16
// records (32 KB) measured 1426 ms against 1272 at 8 (4 blocks per CU).  The runahead kernel
// runs 4 blocks per CU anyway (128 VGPRs): 16 there (8-way slowest shard 245 vs 249 ms).
#ifndef RT_COOP_LEAVES
#define RT_COOP_LEAVES 8
#endif
constexpr int kCoopLeavesPlain = RT_COOP_LEAVES;
#ifndef RT_SPEC_COOP_LEAVES
#define RT_SPEC_COOP_LEAVES 12   // (16 until round 6's leaf deferral: see RT_SPEC_SHADE_MIN)
#endif
// The runahead kernel's coop step issues the child-pair loads from node lanes only
// (rt_wavefront.h trav_step_coop MASK_LOAD; the plain kernel measured slower with it).
#ifndef RT_SPEC_MASK_LOAD
#define RT_SPEC_MASK_LOAD 1
#endif
// Far frames carry the squared entry distance and the cull compares without a root
// (rt_wavefront.h RT_FAR_DIST2); per kernel, because the two measured differently.  One call,
// three interleaved runs each, new form against the sqrt form (profiles/dist2_ab.jsonl):
//   plain kernel, 1-GPU frame      1006.9-1009.1 ms against 1020.8-1022.0 (-13.2 ms, spread 2.2);
//   runahead kernel, 8-way shards  mean 171.0-171.2 against 173.2-173.5 ms, slowest
//                                  172.3-173.2 against 175.1-175.2 (-2.4 ms, spread 0.9).
// The rule was a mean gain of three times the larger spread: the plain kernel (and the other
// non-runahead instantiations, which share its traversal loop) takes the new form; the
// runahead kernel's slowest shard misses it (2.4 < 2.7 ms), so it keeps the sqrt form until a
// measurement with more runs per shard settles it.
#ifndef RT_PLAIN_FAR_DIST2
#define RT_PLAIN_FAR_DIST2 RT_FAR_DIST2
#endif
#ifndef RT_SPEC_FAR_DIST2
#define RT_SPEC_FAR_DIST2 0
#endif
constexpr bool kPlainFarDist2 = RT_PLAIN_FAR_DIST2 != 0;
// The shading pass's gather (rt_path.h RT_SHADE_GATHER), per kernel as the cull above, by the
// same rule.  One call, three interleaved runs each, against the RT_SHADE_GATHER=0 build
// (profiles/shgather_forms_ab.jsonl, the gather in both kernels):
//   plain kernel, 1-GPU frame      984.0-985.1 ms against 1007.4-1008.8 (-23.6 ms, spread 1.4);
//   runahead kernel, 8-way shards  slowest 174.3-176.1 against 174.8-176.0 ms: no gain.
// Only the plain kernel (the parity render without counters: not COUNT, FAST, LSPLIT or the
// accumulator's CHAIN) takes the gather: it is the one the rule was applied to.  The runahead
// kernel keeps the tables' form, and so do the counting, fast-mode and accumulator
// instantiations, which were not measured and whose spills the gather raises (fast 11 -> 28
// VGPRs, fast accumulator 14 -> 49, counting 48 -> 55, counting fast 31 -> 52 at compile time).
#ifndef RT_PLAIN_SHADE_GATHER
#define RT_PLAIN_SHADE_GATHER RT_SHADE_GATHER
#endif
#ifndef RT_SPEC_SHADE_GATHER
#define RT_SPEC_SHADE_GATHER 0
#endif
// Frames a coop step pops at most (rt_wavefront.h RT_MAX_POPS, trav_pop MAXP), per kernel and by
// the rule above.  One frame: the return is a single stack read without a loop, and the pop
// block, which runs in 98% of the traversal iterations for 8 of a wave's 64 lanes, is about half
// as long.  The runahead kernel's 8-way shards gain too, but their slowest shard
// misses the margin (3.0 ms against three times a spread of 1.6), so it keeps two frames.  The
// counting, fast-mode and light-split instantiations and the wavefront kernel were not measured
// and keep RT_MAX_POPS.
#ifndef RT_PLAIN_MAX_POPS
#define RT_PLAIN_MAX_POPS 1
#endif
#ifndef RT_SPEC_MAX_POPS
#define RT_SPEC_MAX_POPS 2
#endif
// No best frame when the near subtree found no hit (rt_wavefront.h RT_ACC_ELIDE, trav_pop ELIDE), per
// kernel and by the rule above.  One call each, three interleaved rounds against the form without it
// (profiles/accelide_ab.jsonl, accelide_spec_ab.jsonl):
//   plain kernel, 1-GPU frame      915.9-920.9 ms against 965.4-966.8 (-47.3 ms, spread 5.0);
//   runahead kernel, 8-way shards  slowest 167.7-168.2 against 174.7-175.0 ms (-6.9 ms, spread 0.5), mean
//                                  166.5-166.7 against 173.2-173.4, three renders per shard.
// Both take it.  The counting, fast-mode, light-split and accumulator (CHAIN, plain and runahead)
// instantiations and the wavefront kernel were not measured and push every best frame.
#ifndef RT_PLAIN_ACC_ELIDE
#define RT_PLAIN_ACC_ELIDE RT_ACC_ELIDE
#endif
#ifndef RT_SPEC_ACC_ELIDE
#define RT_SPEC_ACC_ELIDE RT_ACC_ELIDE
#endif
constexpr bool kPlainAccElide = RT_PLAIN_ACC_ELIDE != 0;
// One ray start per shading pass and the RNG state read where it is drawn from (rt_path.h
// RT_SHADE_CONVERGE, a mask: CONV_START, CONV_RNG), per kernel and by the rule above.  One call, three
// interleaved rounds against the form without them (profiles/shconv_parts_ab.jsonl):
//   plain kernel, 1-GPU frame      903.4-904.5 ms against 917.8-918.1 (-13.7 ms, spread 1.1);
//   the committed tree, two more calls (shconv_ab.jsonl, shconv_ab2.jsonl): -11.2 ms (spread 4.3, the
//   one call under three spreads) and -12.9 ms (spread 4.2).
// The plain kernel takes both.  The runahead kernel was not measured with them (its 8-way shards ran
// the parent form in that call: slowest 168.1-169.9 ms in every build), and neither were the counting,
// fast-mode, light-split and accumulator instantiations: all keep the parent form.
#ifndef RT_PLAIN_SHADE_CONVERGE
#define RT_PLAIN_SHADE_CONVERGE RT_SHADE_CONVERGE
#endif
#ifndef RT_SPEC_SHADE_CONVERGE
#define RT_SPEC_SHADE_CONVERGE 0
#endif
// Leaf rounds per coop step (rt_wavefront.h trav_step_coop round_min): a further round
// while at least this many leaf lanes are unserved.  Plain kernel: 8 (sponza 1080p 1292 ->
// 1278 ms against one round per step).  The runahead kernel's depends on the scene
// (rt_launch_plan.h kCoopRoundMinSpec, kCoopRoundNodes).
#ifndef RT_COOP_ROUND_MIN
#define RT_COOP_ROUND_MIN 8
#endif
constexpr int kCoopRoundMinPlain = RT_COOP_ROUND_MIN;

// What one instantiation of rt_mega_kernel reads of the constants above: which combinations of
// its template parameters exist, the family each belongs to, and that family's values.  The
// kernel's body asks nothing else about its parameters' combination.
template <bool COUNT, bool FAST, bool LSPLIT, bool SPEC, bool CHAIN, bool MOM>
struct MegaCfg {
    static_assert(!SPEC || (!COUNT && !FAST && !LSPLIT), "the runahead kernel renders parity passes without counters only");
    static_assert(!CHAIN || (!COUNT && !LSPLIT), "an accumulator's pass neither counts nor splits the light walk");
    static_assert(!MOM || (FAST && CHAIN), "second moments are a fast accumulator's");
    static constexpr bool spec = SPEC;                  // the runahead kernel (and its CHAIN form)
    static constexpr bool chain = CHAIN && !FAST;       // a parity accumulator's pass
    static constexpr bool fast_chain = CHAIN && FAST;   // a fast accumulator's pass
    static constexpr bool mom = MOM;                    // ... that keeps second moments
    static constexpr bool plain = !COUNT && !FAST && !LSPLIT && !SPEC && !CHAIN;   // the parity render without counters
    // waves per SIMD the register allocation targets (96 VGPRs; the runahead kernel 128)
    static constexpr int wpe = spec ? RT_SPEC_WPE : RT_MEGA_WPE;
    // a wave shades once this many lanes are READY (or none traverses)
    static constexpr int shade_min = spec ? RT_SPEC_SHADE_MIN : RT_SHADE_MIN;
    static constexpr int shade = (spec ? RT_SPEC_SHADE_GATHER : plain && RT_PLAIN_SHADE_GATHER) ? rtd::SHADE_GATHER_HOLD
                                                                                                 : rtd::SHADE_TABLES;
    static constexpr int lds_stack = spec ? rtd::kLdsStackSpec : rtd::kLdsStack;   // LDS stack frames
    static constexpr int coop_leaves = spec ? RT_SPEC_COOP_LEAVES : kCoopLeavesPlain;   // coop leaf records per wave
    static constexpr bool mask_load = spec && RT_SPEC_MASK_LOAD;
    static constexpr int leaf_defer = spec ? rtd::kLeafDefer : COUNT ? 0 : rtd::kLeafDeferPlain;
    static constexpr bool far_dist2 = spec ? RT_SPEC_FAR_DIST2 != 0 : kPlainFarDist2;
    static constexpr int max_pops = spec ? RT_SPEC_MAX_POPS : COUNT ? rtd::kMaxPops : RT_PLAIN_MAX_POPS;
    static constexpr bool acc_elide = !CHAIN && (spec ? RT_SPEC_ACC_ELIDE != 0 : plain && kPlainAccElide);
    static constexpr int converge = CHAIN ? 0 : spec ? RT_SPEC_SHADE_CONVERGE : plain ? RT_PLAIN_SHADE_CONVERGE : 0;   // (a mask)
    static constexpr int coop_round_min = kCoopRoundMinPlain;  // (the runahead kernel's comes with the launch: st.round_min)
    static constexpr bool pack_trav = kPackTrav && !LSPLIT && !spec && !FAST;   // RT_PACK_TRAV through its shading pass
};

#ifdef RT_MEGA_PROF
#include "rt_mega_prof.h"   // diagnostics build (make prof): its counters, TbAcc and report
#endif
// FAST (RT_FLAG_FAST): queue items are (chunk, pixel) work units of `cs`
// samples with per-sample Philox seeds; `out` is then the chunk-major partial buffer that
// rt_fast_reduce_kernel folds.  LSPLIT (RT_FLAG_LIGHT_SPLIT, §8(f)3): the light pdf's
// light-BVH walk as a lane state (rt_mega.h light_step).  `order` (parity mode): queue item
// p renders shard pixel order[p].  `cost` (COUNT only): per-pixel traversal tests out.
// Exit: the queue is monotonic, so once a claim reaches n_items a wave stops claiming; the
// loop ends when no lane of the wave holds work, so the grid always drains.
// SPEC (parity renders without counting): a wave whose claim finds the queue empty enters its
// tail and runs speculative sample runahead (rt_mega.h spec_manage) on its idle lanes.  A
// separate instantiation, so the kernel without it keeps its own register allocation.
// `mode` (0 for the default schedules) packs the hand-off's settings, park_below (plain kernel)
// and resume_pct (SPEC): rt_launch_plan.h mode_pack has the layout and what each one does.
// `queue` is the queue block (rt_mega.h QueueWord names its words); the pre-pass gets the
// address of its own claim counter instead.
// CHAIN (rt_accum_add; parity renders without counting, plain and runahead kernels only): the
// pass of an accumulator.  `spp` is the absolute sample the pass ends at; a pixel starts from its
// record in the chain buffer and the lane that adds its last sample stores the record back
// (rt_mega.h, chain buffer; the buffer's address in the queue block, read where used).  Separate
// instantiations again: the one-shot kernels are the code they were.
// FAST + CHAIN (rt_accum_create_fast): the pass of a fast accumulator.  `cs` is the accumulator's
// chunk size, `mode` the units per item K and st.n the items; queue item q = k * st.n + i is unit k
// of item i (pixel `order ? order[i] : i`), its samples cut from the pixel's record and the pass's
// end `spp` (rt_mega.h mega_assign_fast_chain).  The kernel only reads records; its partials go to
// the unit-major partial buffer and rt_fast_fold_chain_kernel folds them.  A unit past its pixel's
// own starts nothing (the lane claims again), so a wave may leave only once the queue is empty.
// MOM (FAST + CHAIN only, rt_accum_create_fast_moments): that pass, keeping per unit a second
// partial, of the samples' squared colours (rt_moments.h), in the second half of the partial
// buffer; rt_fast_fold_chain_kernel<true> folds both.  Its own instantiation: the others are the
// code they were.
template <bool COUNT, bool FAST = false, bool LSPLIT = false, bool SPEC = false, bool CHAIN = false, bool MOM = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MegaCfg<COUNT, FAST, LSPLIT, SPEC, CHAIN, MOM>::wpe, 8)))
rt_mega_kernel(DevScene sc_in, ShardGeom g, rtd::WfState st, int spp, float *out, unsigned long long *counters,
               unsigned long long *queue, const int *order, unsigned *cost, int cs, int mode) {
    using V = MegaCfg<COUNT, FAST, LSPLIT, SPEC, CHAIN, MOM>;
    // (V::fast_chain, a pass of a fast accumulator: `cs` is its chunk size, `mode` the units per item)
    const int park_below = V::fast_chain ? 0 : rtp::mode_park_below(mode);
    const int resume_pct = V::fast_chain ? 0 : rtp::mode_resume_pct(mode);
    const uint4 *resume = V::spec && resume_pct > 0 ? (const uint4 *)queue[rtd::kQueueParkList] : nullptr;
    // (CHAIN: the pass's item count, the shard's pixels for a full pass or a selection's length
    // for a subset pass, whose pixels `order` lists; a constant of the instantiation chooses, so
    // the one-shot kernels read what they read before)
    const long long n_items = V::fast_chain ? st.n * (long long)mode
                              : FAST     ? g.n_pixels * (long long)((spp + cs - 1) / cs)
                                         : (V::chain || (V::spec && resume)) ? st.n : g.n_pixels;
    const int lane = threadIdx.x & 63;
    // sRGB texel-decode table in LDS: the shading's lane-dependent lookups become ds_reads (the
    // linear decode is computed: rt_path.h texel_decode)
    __shared__ float lut[256];
    for (int k = threadIdx.x; k < 256; k += blockDim.x) lut[k] = sc_in.lut[k];
    __syncthreads();
    DevScene sc = sc_in;
    sc.lut = lut;
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    uint2 spill[rtd::kStack - V::lds_stack];
    rtd::LdsStackT<V::lds_stack> S{spill};
    const rtd::GlobalNodes nodes{sc.node};
    const rtd::NodeRec root = rtd::load_node(sc.node, 0);
    // lane state: the runahead kernel keeps TravState, the others share the node / leaf fields
    // (rt_wavefront.h TravStateU)
    std::conditional_t<V::spec, rtd::MegaLane, rtd::MegaLaneU> L;
    L.pix = -1;
    L.state = rtd::M_IDLE;
    // A lane that never gets a pixel still takes part in the shading pass's packing
    // (RT_PACK_TRAV: phase | state << 2 | sp << 5): its phase and stack depth are defined from
    // the start, not the register contents the previous kernel left (a stray phase bit would
    // turn an idle lane's state into TRAV or READY).
    L.T.phase = rtd::TP_POP;
    L.T.sp = 0;
#if defined(RT_DEBUG_CHECKS)
    // debug builds: rt_debug_set_poison(1) leaves out-of-range leftovers in every lane's phase
    // and stack depth instead (the state round 5's fault came from), to show that the packing
    // below masks them and that its check reports them (tests/test_gpu_parity.py)
    if (rt_debug_poison) {
        L.T.phase = 0x7ffffffd;
        L.T.sp = 0x3ffffff;
    }
#endif
    L.wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)threadIdx.x) & ~63u;
    bool exhausted = false;
    bool tail = false, wave_room = false;
#ifdef RT_MEGA_PROF
    unsigned long long pf[7] = {0, 0, 0, 0, 0, 0, 0};
    if (threadIdx.x < 8) rt_prof_lds[threadIdx.x] = 0;
    if (threadIdx.x < 16) rtd::spec_prof_lds[threadIdx.x] = 0;
    if (threadIdx.x < 4 * rtd::kPopProfLds) rtd::pop_prof_lds[threadIdx.x / rtd::kPopProfLds][threadIdx.x % rtd::kPopProfLds] = 0;
    if (threadIdx.x < 4) rtd::pop_best_lds[threadIdx.x] = 0;
    if ((threadIdx.x & 63) == 0) rtd::spec_wave_t0_lds[threadIdx.x >> 6] = wall_clock64();
    __syncthreads();
    long long tp = clock64();
    const unsigned long long wt0 = wall_clock64();
    TbAcc tbk;
#endif
    // hand-off resume: the slots past waves * per are taken in the tail (rt_mega.h SpecClaim) by
    // waves below `per` active records
    // (the resume map's address, 0 = slot order: read where used)
    rtd::SpecClaim claim{queue + rtd::kQueueResume, 0, n_items, resume, 0, false,
                         resume ? (const int *)queue[rtd::kQueueResumeMap] : nullptr};
    bool park = false;   // (plain kernel, hand-off: this wave parks its pixels)
    if constexpr (V::spec) {
        if (resume) {
            const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
            // (dealt, per: must equal rtp::resume_deal(n_items, resume_pct, waves))
            const long long dealt = (n_items * resume_pct + 99) / 100;
            const int per = (int)std::min<long long>(64, std::max<long long>(1, (dealt + waves - 1) / waves));
            const long long p = (rtd::mega_slot() >> 6) * per + lane;
            bool xk = false;
            rtd::Rng xs{0u, 0u, 0.f};
            if (lane < per && p < n_items) {
                const rtd::Parked q = rtd::parked_item(resume, claim.ridx, p);
                if (q.pix != rtd::kNoPark) {
                    rtd::mega_resume(L, sc, g, q, root);
                    xk = true;
                    xs = q.x;
                }
            }
            exhausted = true;
            claim.base = waves * per;
            claim.keep = per;
            claim.open = claim.base < n_items;
            if (lane == 0) rtd::spec_hint_take();
            rtd::spec_convert(L, sc, g, rtd::SpecView{(uint4 *)st.mid, st.lanes, rtd::mega_slot() - lane}, lane, xk, xs);
            tail = true;
#ifdef RT_MEGA_PROF
            if (lane == 0) RT_SPEC_STAT(7, 1);
#endif
        }
    }
#if defined(RT_DEBUG_CHECKS)
    unsigned long long dbg_iter = 0;   // debug builds: a wave looping this long reports and leaves
#endif
    for (;;) {
#if defined(RT_DEBUG_CHECKS)
        if (++dbg_iter > (1ull << 22)) {
            const unsigned long long w = (unsigned long long)__popcll(__ballot(L.state == rtd::M_TRAV)) |
                                         (unsigned long long)__popcll(__ballot(L.state == rtd::M_READY)) << 8 |
                                         (unsigned long long)__popcll(__ballot(L.state == rtd::M_DONE)) << 16 |
                                         (unsigned long long)__popcll(__ballot(L.state == rtd::M_DONE_NEW)) << 24 |
                                         (unsigned long long)__popcll(__ballot(L.state == rtd::M_IDLE)) << 32 |
                                         (unsigned long long)tail << 40 | (unsigned long long)park << 41 |
                                         (unsigned long long)exhausted << 42 | (unsigned long long)wave_room << 43;
            RT_CHECK(false, 15, w, (void)0);
            if constexpr (V::spec) {   // the first such wave prints its lanes and records
                const rtd::SpecView V{(uint4 *)st.mid, st.lanes, rtd::mega_slot() - lane};
                const uint4 a = *V.w(0, lane), b = *V.w(1, lane), c = *V.w(2, lane), d = *V.w(3, lane), j = *V.w(4, lane);
                if (atomicAdd(&rt_debug_prints, 1u) < 64u)
                    printf("[stuck] blk %d lane %d state %d pix %d s %d | job tag %u | rec pix %u f %u n %u e %u meta %u tab %08x%08x\n",
                           (int)blockIdx.x, lane, L.state, L.pix, rtd::lane_ctr(L).s, j.x, a.x, a.y, a.z, a.w, b.w, d.w, c.w);
            }
            break;
        }
#endif
        if (!V::spec && !COUNT && !FAST && park) {   // hand-off: lanes idle with a pixel park it
            if (L.state == rtd::M_IDLE && L.pix >= 0) {
                rtd::park_pixel((uint4 *)queue[rtd::kQueueParkList], rtd::mega_slot_of(L), L.pix, rtd::lane_ctr(L).s, rtd::lane_rng(L),
                                rtd::lane_sum(L));
                L.pix = -1;
            }
        }
        if (!exhausted) {   // lanes without work take the next items (one atomic per wave)
            const bool need = L.pix < 0 && (kClaimStride == 1 || lane % kClaimStride == 0);
            const unsigned long long m = __ballot(need);
            if (m) {
                const int leader = __ffsll((unsigned long long)m) - 1;
                const unsigned cm = (unsigned)__popcll(m);
                // claiming lanes below this one (mbcnt of the ballot: no per-lane mask held)
                const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                unsigned long long base = 0;
                if (need && below == 0) base = atomicAdd(queue + rtd::kQueueRender, (unsigned long long)cm);   // the leader
                base = __shfl(base, leader, 64);
                if (need) {
                    const long long p = (long long)base + below;
                    if (p < n_items) {
                        if constexpr (V::mom)
                            rtd::mega_assign_fast_chain<COUNT, true>(L, sc, g, p, st.n, order, cs, spp, root, cnt, rtd::chain_of(queue),
                                                                     queue);
                        else if constexpr (V::fast_chain)
                            rtd::mega_assign_fast_chain<COUNT>(L, sc, g, p, st.n, order, cs, spp, root, cnt, rtd::chain_of(queue));
                        else if (FAST) rtd::mega_assign_fast<COUNT>(L, sc, g, p, cs, spp, root, cnt);
                        else if constexpr (V::chain)
                            rtd::mega_assign_chain<COUNT>(L, sc, g, order ? order[p] : (int)p, root, cnt, rtd::chain_of(queue), spp);
                        else rtd::mega_assign<COUNT>(L, sc, g, order ? order[p] : (int)p, root, cnt);
                    }
                }
                if ((long long)base + cm >= n_items) exhausted = true;
            }
        }
        if constexpr (V::spec) {
            if (exhausted && !tail) {
                if (lane == 0) rtd::spec_hint_take();
                if constexpr (V::chain)
                    rtd::spec_convert_chain(L, sc, g, rtd::SpecView{(uint4 *)st.mid, st.lanes, rtd::mega_slot() - lane}, lane,
                                            rtd::chain_of(queue));
                else
                    rtd::spec_convert(L, sc, g, rtd::SpecView{(uint4 *)st.mid, st.lanes, rtd::mega_slot() - lane}, lane);
                tail = true;
                wave_room = false;
#ifdef RT_MEGA_PROF
                if (lane == 0) RT_SPEC_STAT(7, 1);
#endif
            }
            if (tail) {
                wave_room |= rtd::spec_hint_take();
                if (__any(L.state == rtd::M_DONE_NEW) || (wave_room && __any(L.state == rtd::M_IDLE))) {
#ifdef RT_MEGA_PROF
                    const long long c0 = clock64();
                    tbk.c[5] += 1;
#endif
                    wave_room = rtd::spec_manage<V::chain>(rtd::SpecLanes{L}, sc, g,
                                                 rtd::SpecView{(uint4 *)st.mid, st.lanes, rtd::mega_slot() - lane}, spp,
                                                 out, root, claim);
#ifdef RT_MEGA_PROF
                    if (lane == 0) {
                        RT_SPEC_STAT(0, 1);
                        RT_SPEC_STAT(1, clock64() - c0);
                    }
#endif
                }
                if (!__any(L.state != rtd::M_IDLE)) break;
            } else if (!__any(L.pix >= 0)) {
                break;
            }
        } else if constexpr (V::fast_chain) {
            // (a claim may leave every lane without a pixel, all its units being past their
            // pixels' own: the wave leaves only once the queue is empty too, else claims again)
            if (!__any(L.pix >= 0)) {
                if (exhausted) break;
                continue;
            }
        } else if (!__any(L.pix >= 0)) {
            break;
        }
        // hand-off: a wave whose queue is empty and that holds fewer than park_below pixels parks
        // each of them at its next sample end (rt_mega.h mega_shade)
        if (!V::spec && park_below > 0 && exhausted && !park) park = rtp::park_rule(__popcll(__ballot(L.pix >= 0)), park_below);
        const int nr = __popcll(__ballot(L.state == rtd::M_READY || (LSPLIT && L.state == rtd::M_LREADY)));
        const int nt = __popcll(__ballot(L.state == rtd::M_TRAV || (LSPLIT && L.state == rtd::M_LTRAV)));
        // (must equal rtp::shade_rule(nr, nt, shade_min))
        const bool shade_now = nr > 0 && (nr >= V::shade_min || nt == 0);
        // Runahead kernel (the 8-way shards): a traversal iteration issues at priority 1, a
        // shading pass at 0, so waves in their long shading code give issue slots to waves
        // stepping the frame's sample chains: slowest 8-way shard 295 -> 280 ms.  The plain
        // kernel stays at 0 (1 GPU: 1360 -> 1395 ms with the same toggle; 4-way unchanged)
        // (profiles/r02_tail_ab.jsonl).
        if constexpr (V::spec) {
            if (shade_now) __builtin_amdgcn_s_setprio(0);
            else __builtin_amdgcn_s_setprio(1);
        }
#ifdef RT_MEGA_PROF
        {
            const long long t1 = clock64();
            pf[2] += (unsigned long long)(t1 - tp);
            tp = t1;
            pf[shade_now ? 3 : 4] += 1;
            pf[shade_now ? 5 : 6] += (unsigned long long)(shade_now ? nr : nt);
            tbk.at(wt0);
            if (shade_now) {
                tbk.c[3] += 1;
                tbk.c[4] += (unsigned long long)nr;
            }
        }
#endif
        if (!LSPLIT && !shade_now) {
            // Traversal iterations until the wave would shade (the condition above): nothing
            // but trav_step and two ballots per iteration.  In a traversal iteration no lane
            // ends a path, so no lane claims a pixel and a tail wave's runahead records do not
            // change: the outer loop's work between two shading passes is only this.
            int kt = nt;
            int leaf_defer = 0;   // (the runahead kernel's leaf steps deferred in a row: rt_wavefront.h RT_LEAF_DEFER)
            do {
                if (rtd::trav_step_coop<COUNT, V::coop_leaves, V::mask_load, V::leaf_defer, V::far_dist2, V::max_pops,
                                         V::acc_elide>(
                        sc, L.r, L.T, S, nodes, cnt, L.state == rtd::M_TRAV, V::spec ? st.round_min : V::coop_round_min,
                        rtd::NoHook{}, &leaf_defer))
                    L.state = rtd::M_READY;
                const unsigned long long rb = __ballot(L.state == rtd::M_READY), tb = __ballot(L.state == rtd::M_TRAV);
                kt = __popcll(tb);
                if (kt == 0 || __popcll(rb) >= V::shade_min) break;
#ifdef RT_MEGA_PROF
                pf[4] += 1;
                pf[6] += (unsigned long long)kt;
                tbk.c[0] += 1;
                tbk.c[1] += (unsigned long long)kt;
                tbk.c[2] += (unsigned long long)__popcll(__ballot(L.state != rtd::M_IDLE));
#endif
            } while (true);
        } else if (V::pack_trav) {
            // shading pass (the inner loop above runs every traversal iteration): a lane that
            // does not shade keeps its phase, stack depth and state packed in one register
            // through the pass (RT_PACK_TRAV).  phase < 4, state < 8 and sp <= kStack hold in
            // every lane (set at the kernel's start, only ever assigned such values; checked in
            // the debug build), and the fields are masked anyway, so that a stray bit of one
            // can never reach another (round 5: an idle lane's leftover phase bit made it READY)
            RT_CHECK((unsigned)L.T.phase < 4u && (unsigned)L.state < 8u && (unsigned)L.T.sp <= (unsigned)rtd::kStack, 14,
                     (unsigned)L.T.phase | (unsigned long long)(unsigned)L.state << 32, (void)0);
            uint32_t pk = ((uint32_t)L.T.phase & 3u) | ((uint32_t)L.state & 7u) << 2 | ((uint32_t)L.T.sp & 127u) << 5;
            asm volatile("" : "+v"(pk));   // (opaque: the compiler cannot fold the unpacking back)
            if (L.state == rtd::M_READY) {
                L.T.phase = 0;   // dead in a READY lane (its stack is empty: T.sp == 0)
                L.T.sp = 0;
                rtd::mega_shade<COUNT, FAST, V::chain, V::shade, false, V::converge>(L, sc, g, st, spp, out, cost, root, S, cnt, V::spec && tail, park,
                                                                 queue);
            } else {
                L.T.phase = (int)(pk & 3u);
                L.state = (int)((pk >> 2) & 7u);
                L.T.sp = (int)(pk >> 5);
            }
        } else {
            rtd::mega_iterate<COUNT, decltype(S), decltype(nodes), FAST, LSPLIT, V::chain, V::shade, V::mom, V::converge>(
                L, shade_now, sc, g, st, spp, out, cost, root, S, nodes, cnt, V::spec && tail, false, queue);
            // RT_INV_RECOMPUTE: 1 / direction is recomputed after a shading pass (the same IEEE
            // division as make_ray, so the same bits), so a traversing lane does not hold it
            // through the pass's register peak (plain kernel 48 -> 42 spilled VGPRs; 39 with
            // RT_UV_RECOMPUTE; frame -1.5% alone, -2.6% with it: profiles/r05k_ab.jsonl).  0: A/B.
            if (kInvRecompute && shade_now) L.r.inv = rtv::divv(rtd::V3{1.f, 1.f, 1.f}, L.r.d);
        }
        if (V::pack_trav && kInvRecompute && shade_now)
            L.r.inv = rtv::divv(rtd::V3{1.f, 1.f, 1.f}, L.r.d);

#ifdef RT_MEGA_PROF
        {
            const long long t1 = clock64();
            pf[shade_now ? 0 : 1] += (unsigned long long)(t1 - tp);
            tp = t1;
            if (!LSPLIT && shade_now && lane == 0) atomicAdd(&rt_prof_lds[7], (unsigned long long)(t1 - rt_prof_mark_lds[threadIdx.x >> 6]));
        }
#endif
    }
#ifdef RT_MEGA_PROF
    tbk.flush(tbk.b);
    if (lane == 0) {
        for (int k = 0; k < 7; ++k) atomicAdd(&g_mega_prof[k], pf[k]);
        atomicAdd(&g_mega_prof[7], 1ull);
        const unsigned wi = atomicAdd(&g_wave_n, 1u);
        if (wi < (unsigned)kProfWaves) {
            g_wave_t[2 * wi] = wt0;
            g_wave_t[2 * wi + 1] = wall_clock64();
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) atomicAdd(&g_mega_seg[threadIdx.x], rt_prof_lds[threadIdx.x]);
    if (threadIdx.x < 16) atomicAdd(&rtd::g_spec_prof[threadIdx.x], rtd::spec_prof_lds[threadIdx.x]);
    if (threadIdx.x < 4) atomicAdd(&rtd::g_pop_prof[rtd::kPopProfLds + threadIdx.x], (unsigned long long)rtd::pop_best_lds[threadIdx.x]);
    if (threadIdx.x < rtd::kPopProfLds)
        atomicAdd(&rtd::g_pop_prof[threadIdx.x], rtd::pop_prof_lds[0][threadIdx.x] + rtd::pop_prof_lds[1][threadIdx.x] +
                                                     rtd::pop_prof_lds[2][threadIdx.x] + rtd::pop_prof_lds[3][threadIdx.x]);
#endif
    rtd::counters_flush<COUNT>(cnt, counters);
}

// The rt_mega_kernel instantiation of a variant: the table is rt_launch_plan.h's kVariants, entry
// for entry (the eleven share one signature), so the instantiations that exist are the lines of
// that table and nothing here names one.  Null: the variant has no kernel.
using MegaKernel = void (*)(DevScene, ShardGeom, rtd::WfState, int, float *, unsigned long long *, unsigned long long *,
                            const int *, unsigned *, int, int);
template <int... I>
inline MegaKernel mega_kernel_at(int i, std::integer_sequence<int, I...>) {
    using rtp::kVariants;
    static const MegaKernel table[] = {rt_mega_kernel<kVariants[I].count, kVariants[I].fast, kVariants[I].lsplit,
                                                      kVariants[I].spec, kVariants[I].chain, kVariants[I].mom>...};
    return table[i];
}

inline MegaKernel mega_kernel_of(const rtp::Variant &v) {
    const int i = rtp::variant_index(v);
    return i < 0 ? nullptr : mega_kernel_at(i, std::make_integer_sequence<int, rtp::kNumVariants>{});
}
