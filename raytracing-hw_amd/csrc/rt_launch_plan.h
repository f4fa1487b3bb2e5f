// rt_launch_plan.h — what a render launches, decided from plain values (host only, no HIP).
//
// rt_device.hip's launch() asks two questions before it touches the device:
//   plan_schedule   which rt_mega_kernel instantiation renders the shard, with which schedule
//                   bits, work units and pixel order (and which parameters are refused);
//   plan_grid       how many blocks that kernel gets (from its resident block count), the
//                   order spread's shape and the hand-off relaunch's deal.
// Two steps because the grid depends on the occupancy of the kernel step one chose.  Resident
// block counts are inputs, so every rule here runs without a GPU (tests/test_launch_plan.py).
// The tuning constants the rules use live here with their measurements; the #ifndef RT_… ones
// are compile-time A/B knobs (make variant VFLAGS=-DRT_…=…).  The rules the kernel's wave loop
// shares with the plan and with its host emulation (the `mode` word, the resume deal, the shade
// and park rules) are constexpr functions below, next to kHandoffBelow and kHandoffPct.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/rt_hw.h"

namespace rtp {

// The pre-pass and sort cost about one sample per pixel, so below kOrderMinSpp the order
// is not built unless asked for (RT_FLAG_HEAVY_ORDER): row-major measured faster there
// (profiles/r02_configs.jsonl: C1 256x256x4 4.5 vs 5.0 ms, C2 512x512x64 17.7 vs 18.0 ms, C5
// 3840x2160 at 16 spp 378 vs 397 ms; at 256 spp the order wins, C3 748 vs 779 ms, headline
// 1357 vs 1393 ms).
constexpr int kOrderMinSpp = 128;
constexpr int kFastMaxChunks = 128;  // fast mode: at most this many work units per pixel
// The runahead instantiation renders shards of at most kSpecPixelsPerLane pixels per resident
// lane.  Round 3 (runahead window 3): up to 2 pixels per lane, so the 4-way shards of the
// headline (2 per lane) use it too: slowest 4-way shard 347.5 vs 358.7 ms; at 4 per lane
// (2-way) 636 vs 625 (profiles/r03_ab.jsonl r03ah24).
#ifndef RT_SPEC_PIXELS_PER_LANE
#define RT_SPEC_PIXELS_PER_LANE 2
#endif
constexpr long long kSpecPixelsPerLane = RT_SPEC_PIXELS_PER_LANE;
// Hand-off (round 6): a parity render on the plain kernel (more than kSpecPixelsPerLane pixels
// per lane) ends its tail in the runahead kernel.  A plain wave whose queue is empty parks its
// pixels once fewer than kHandoffBelow of its lanes hold one (each at its next sample end, with
// its RNG state and sum), and a runahead launch over the whole resident grid resumes them
// (kHandoffPct percent dealt at its start, the rest claimed in the tail): the plain kernel's
// sparse tail waves, where most lanes idle while a few pixels finish their chains, become
// runahead records.  Headline frame 1048.3 vs 1061.5 ms on one box, 2-way shards 578.6 vs
// 580.6 ms, same bits; parking at 48 / 60 held pixels 1049.0 / 1050.8 ms, 70% dealt 1050.2 ms
// (profiles/r06g_handoff_ab.jsonl).  RT_FLAG_NO_RUNAHEAD turns it off with the runahead.
#ifndef RT_HANDOFF_BELOW
#define RT_HANDOFF_BELOW 56
#endif
#ifndef RT_HANDOFF_PCT
#define RT_HANDOFF_PCT 100
#endif
// RT_HANDOFF_SPREAD: the runahead launch deals the parked pixels with the most work left
// ((samples left) x (pre-pass estimate)) one per wave, instead of in park-list slot order,
// where a plain wave's consecutive claims (the last pixels of the order, those that end the
// frame) sit together and share one wave's idle lanes.
#ifndef RT_HANDOFF_SPREAD
#define RT_HANDOFF_SPREAD 1
#endif
constexpr int kHandoffBelow = RT_HANDOFF_BELOW;
constexpr int kHandoffPct = RT_HANDOFF_PCT;
constexpr bool kHandoffSpread = RT_HANDOFF_SPREAD != 0;

// The schedule rules the host plan, rt_mega_kernel and the host emulation of its wave loop
// (tests/native/mega_emu.h) share, each written once.  The kernel calls those that leave its
// device listing as it is (the mode word, the park rule) and keeps the others as literal
// expressions marked with the rule's name: register allocation of the plain kernel moved
// throughout when they were calls.
//
// rt_mega_kernel's `mode` argument (0 for the default schedules) packs the hand-off's settings
// into one kernel argument (the kernel is short of SGPRs, which spill into VGPRs):
//   bits 0-7   park_below > 0 (plain kernel): a wave whose queue is empty and that holds fewer
//              than park_below pixels parks them, each at its next sample end, in the park list
//              at its lane slot (rt_mega.h park_pixel; the list's address in the queue block,
//              read where used: no register held in the loop);
//   bits 8-15  resume_pct > 0 (SPEC): the items are that park list's slots (st.n of them); wave
//              w of the grid takes slots [w * per, (w + 1) * per), its lanes below per one each
//              (resume_deal), skips the empty ones and enters its tail at once; the slots past
//              the grid's share are claimed in the tail (rt_mega.h SpecClaim) through the resume
//              claim counter.
constexpr int mode_pack(int park_below, int resume_pct) { return (park_below & 255) | (resume_pct & 255) << 8; }
constexpr int mode_park_below(int mode) { return mode & 255; }
constexpr int mode_resume_pct(int mode) { return (mode >> 8) & 255; }
// The resume launch's deal: `dealt` = pct percent of the park list's slots, rounded up, go out
// at its start, `per` of them to each of its waves (one per lane: at most 64; at least 1).
struct Deal {
    long long dealt, per;
};
constexpr Deal resume_deal(long long slots, int pct, long long waves) {
    const long long dealt = (slots * pct + 99) / 100;
    return {dealt, std::min<long long>(64, std::max<long long>(1, (dealt + waves - 1) / waves))};
}
// A wave shades its nr READY lanes once there are shade_min of them or none of its nt others
// still traverses; otherwise it steps the traversing lanes.
constexpr bool shade_rule(int nr, int nt, int shade_min) { return nr > 0 && (nr >= shade_min || nt == 0); }
// A plain wave whose queue is empty parks its pixels once it holds fewer than park_below.
constexpr bool park_rule(int held, int park_below) { return held < park_below; }

// Diagnostics (A/B builds only): only every k-th lane of a wave claims pixels, so a wave
// holds at most 64 / k pixels and the grid grows k-fold (lockstep study).
#ifndef RT_CLAIM_STRIDE
#define RT_CLAIM_STRIDE 1
#endif
constexpr int kClaimStride = RT_CLAIM_STRIDE;
// Leaf rounds per coop step of the runahead kernel (rt_wavefront.h trav_step_coop round_min: a
// further round while at least this many leaf lanes are unserved): 4 on scenes of fewer than
// kCoopRoundNodes BVH nodes, where most traversal steps are leaf steps (cornell 512x512x64,
// 36 triangles: 26.8 -> 16.7 ms), one round per step (65: never a second) on larger ones (the
// 8-way sponza shards: 1% slower with rounds) (profiles/r03_ab.jsonl r03q-s).
#ifndef RT_SPEC_COOP_ROUND_MIN
#define RT_SPEC_COOP_ROUND_MIN 4
#endif
constexpr int kCoopRoundMinSpec = RT_SPEC_COOP_ROUND_MIN;   // small scenes
constexpr int kCoopRoundNodes = 4096;

// Device buffers are laid out in parts that start on 256-byte boundaries.
inline size_t align_up(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// A refusal (code RT_OK: none) with the text rt_last_error reports.
struct Refusal {
    int code = RT_OK;
    std::string msg;
    explicit operator bool() const { return code != RT_OK; }
};

struct PlanIn {
    int flags = 0, kernel = RT_KERNEL_LANE, count = 0, fast_chunk = 0;
    int spp = 0;              // the absolute sample the render ends at (p->spp, or the scene's)
    int pass_spp = 0;         // an accumulator pass: the samples it adds; 0 for a one-shot render
    long long n_pixels = 0;   // the shard's
    int ray_depth = 0, n_nodes = 0;   // the scene's
    long long spec_blocks = 0;        // resident blocks of the runahead kernel (the pass's CHAIN form for a pass)
    // A subset pass (rt_accum_add_selected): the items of its list, each one pixel raised to
    // `spp` from wherever its record stands; 0 = a full pass.  The list is the order: no
    // pre-pass runs and RT_FLAG_HEAVY_ORDER is ignored.
    long long subset_items = 0;
    // A pass of a fast accumulator (rt_accum_create_fast; with pass_spp > 0): fast_chunk is the
    // accumulator's chunk size, used as it is, and fast_units the work units every item of the
    // launch gets (the chunks the pass of the item furthest behind overlaps: rt_fast_units.h
    // units_of; the host keeps it at or below kFastMaxChunks by splitting the pass).
    bool fast_accum = false;
    int fast_units = 0;
    bool moments = false;   // that accumulator keeps second moments (rt_accum_create_fast_moments)
};

// The two order flags exclude each other (shared with the accumulator's parameter check).
inline bool order_flags_conflict(int flags) { return (flags & RT_FLAG_NATURAL_ORDER) && (flags & RT_FLAG_HEAVY_ORDER); }

// The refusals that do not depend on the shard.
inline Refusal plan_check(const PlanIn &in) {
    if (in.spp < 1) return {RT_ERR_ARG, "rt_render: samples per pixel must be >= 1"};
    if (in.kernel != RT_KERNEL_LANE && in.kernel != RT_KERNEL_WAVEFRONT)
        return {RT_ERR_ARG, "rt_render: unknown kernel " + std::to_string(in.kernel) + " (0 lane-resident, 4 wavefront)"};
    if ((in.flags & (RT_FLAG_FAST | RT_FLAG_LIGHT_SPLIT)) && in.kernel != RT_KERNEL_LANE)
        return {RT_ERR_ARG, "rt_render: fast mode and the light-split kernel run on kernel 0 only"};
    if (in.fast_chunk < 0) return {RT_ERR_ARG, "rt_render: fast_chunk must be >= 0"};
    if (order_flags_conflict(in.flags))
        return {RT_ERR_ARG, "rt_render: RT_FLAG_NATURAL_ORDER and RT_FLAG_HEAVY_ORDER exclude each other"};
    return {};
}

// The rt_mega_kernel instantiation (rt_mega_device.h mega_kernel_of).  `chain`: a pass of an
// accumulator, on the plain or the runahead kernel (parity), or with `fast` the pass of a fast
// accumulator (PlanIn.fast_accum), with `mom` one that keeps second moments; rt_accum_* refuse
// the other modes.
struct Variant {
    bool count = false, fast = false, lsplit = false, spec = false, chain = false, mom = false;
};
// The eleven instantiations that exist, in the order of the device listing: the kernel table is
// generated from these lines (rt_mega_device.h), and a variant that is not among them has no
// kernel (variant_index < 0: launch() refuses it).  A new instantiation is one line here plus
// what its MegaCfg reads.
constexpr Variant kVariants[] = {
    // count, fast, lsplit, spec, chain, mom
    {true, true, false, false, false, false},    // RT_FLAG_FAST with counters; the order pre-pass (launch_order)
    {false, false, false, true, true, false},    // a parity accumulator's pass on a small shard or subset; its hand-off relaunch
    {false, false, false, true, false, false},   // the runahead kernel: a parity render of a small shard; the hand-off relaunch
    {false, true, false, false, false, false},   // RT_FLAG_FAST
    {true, false, true, false, false, false},    // RT_FLAG_LIGHT_SPLIT with counters
    {false, false, true, false, false, false},   // RT_FLAG_LIGHT_SPLIT
    {false, false, false, false, false, false},  // the plain kernel: a parity render of a large shard
    {true, false, false, false, false, false},   // a parity render with counters
    {false, false, false, false, true, false},   // a parity accumulator's pass on a large shard
    {false, true, false, false, true, false},    // a fast accumulator's pass (rt_accum_create_fast)
    {false, true, false, false, true, true},     // a moments accumulator's pass (rt_accum_create_fast_moments)
};
constexpr int kNumVariants = (int)(sizeof kVariants / sizeof kVariants[0]);
constexpr int variant_bits(const Variant &v) {
    return v.count | v.fast << 1 | v.lsplit << 2 | v.spec << 3 | v.chain << 4 | v.mom << 5;
}
// The entry of kVariants that is v, or -1.
constexpr int variant_index(const Variant &v) {
    for (int i = 0; i < kNumVariants; ++i)
        if (variant_bits(kVariants[i]) == variant_bits(v)) return i;
    return -1;
}

struct Schedule {
    Refusal refused;
    bool lane = false;       // a lane-resident launch follows (else wavefront, or nothing: empty shard)
    Variant v;
    uint64_t sched = 0;      // rt_stats.schedule (RT_SCHED_*)
    bool handoff = false;    // the plain kernel parks its tail and a runahead launch resumes it
    int mode = 0;            // the kernel's last argument: mode_pack's word, a fast pass's units per item
    bool ordered = false;    // the heaviest-first pixel order is built (launch_order)
    int cs = 0, chunks = 1;  // fast mode: samples per work unit, units per pixel
    long long n_items = 0;   // queue items: pixels x chunks
    int round_min = 65;      // the runahead kernel's leaf rounds (WfState.round_min)
    int stats_spp = 0;       // samples per pixel this launch adds (rt_stats.samples)
    long long n_pixels = 0, spec_blocks = 0;   // (inputs plan_grid needs again)
    int ray_depth = 0;
};

inline Schedule plan_schedule(const PlanIn &in) {
    Schedule s;
    if ((s.refused = plan_check(in))) return s;
    s.n_pixels = in.n_pixels;
    s.spec_blocks = in.spec_blocks;
    s.ray_depth = in.ray_depth;
    s.stats_spp = in.pass_spp > 0 ? in.pass_spp : in.spp;
    if (in.n_pixels <= 0) return s;   // an empty shard launches nothing
    if (in.kernel == RT_KERNEL_WAVEFRONT) {   // (launch_wavefront has its own limits)
        s.sched = RT_SCHED_WAVEFRONT;
        return s;
    }
    if (in.ray_depth < 1 || in.ray_depth > 15) s.refused = {RT_ERR_LIMIT, "ray_depth must be in [1, 15]"};
    else if (in.spp >= (1 << 20)) s.refused = {RT_ERR_LIMIT, "rt_render: spp must be < 2^20"};
    if (s.refused) return s;
    s.lane = true;
    Variant &v = s.v;
    v.count = in.count != 0;
    const bool fast_pass = in.fast_accum && in.pass_spp > 0;
    v.fast = fast_pass || (in.flags & RT_FLAG_FAST) != 0;
    v.lsplit = !v.fast && (in.flags & RT_FLAG_LIGHT_SPLIT) != 0;
    v.chain = in.pass_spp > 0;
    v.mom = fast_pass && in.moments;
    // fast mode (RT_FLAG_FAST): work units of `cs` samples, Philox seed per sample, at most
    // kFastMaxChunks units per pixel (partials: pixels x chunks x 12 B)
    if (fast_pass) {
        // (the accumulator's chunk size is fixed for its life: a boundary that moved with the
        // pass would change the sum; the FAST + CHAIN kernel, never ordered, no runahead)
        if (in.fast_chunk < 1 || in.fast_units < 1 || in.fast_units > kFastMaxChunks) {
            s.refused = {RT_ERR_ARG, "rt_accum_add: a fast pass needs a chunk size >= 1 and 1 .. " +
                                         std::to_string(kFastMaxChunks) + " units per item"};
            s.lane = false;
            return s;
        }
        s.cs = in.fast_chunk;
        s.chunks = in.fast_units;
    } else if (v.fast) {
        s.cs = std::min(in.spp, std::max(in.fast_chunk > 0 ? in.fast_chunk : 2, (in.spp + kFastMaxChunks - 1) / kFastMaxChunks));
        s.chunks = (in.spp + s.cs - 1) / s.cs;
    }
    const bool subset = v.chain && in.subset_items > 0;
    s.n_items = subset ? in.subset_items * (fast_pass ? s.chunks : 1) : in.n_pixels * s.chunks;
    // Speculative sample runahead (rt_mega.h) where the frame is mostly tail: a shard of at most
    // kSpecPixelsPerLane pixels per resident lane (the 8-way split of the headline: 342 -> 304
    // ms in round 2; at 4-way, 2 pixels per lane, 359 -> 348 ms in round 3).  A larger shard
    // runs the plain kernel and hands its tail off to the runahead kernel.
    const bool parity = !v.fast && !v.lsplit && !v.count && !(in.flags & RT_FLAG_NO_RUNAHEAD);
    // (decided on the items: a small subset of a large shard is all tail)
    v.spec = parity && s.n_items * kClaimStride <= kSpecPixelsPerLane * in.spec_blocks * 256;
    s.handoff = parity && !v.spec && kClaimStride == 1;
    s.sched = v.fast ? RT_SCHED_FAST : v.lsplit ? RT_SCHED_LIGHT_SPLIT : v.spec ? RT_SCHED_RUNAHEAD : RT_SCHED_LANE;
    if (s.handoff) s.sched |= RT_SCHED_RUNAHEAD;
    s.mode = v.fast && v.chain ? s.chunks : mode_pack(s.handoff ? kHandoffBelow : 0, 0);
    // (a pass is ordered by the rule on its own samples)
    s.ordered = !v.fast && !subset && !(in.flags & RT_FLAG_NATURAL_ORDER) &&
                (s.stats_spp >= kOrderMinSpp || (in.flags & RT_FLAG_HEAVY_ORDER));
    s.round_min = in.n_nodes < kCoopRoundNodes ? kCoopRoundMinSpec : 65;
    return s;
}

struct Grid {
    Refusal refused;
    long long blocks = 0, slots = 0;   // 256-thread blocks of the main launch; its lane slots
    // the order spread deals one pixel of every cost stratum to each claim of 64 of the launch's
    // first round (one per wave): `groups` claims of `per` items (rt_order_spread_kernel)
    long long groups = 0, per = 64;
    // the hand-off's relaunch over the runahead kernel's whole resident grid: its blocks and
    // waves, the park-list slots dealt at its start and how many of them each wave takes
    // (resume_deal, as at the kernel's resume site).
    long long blocks2 = 0, waves2 = 0, dealt = 0, per2 = 0;
    int mode2 = 0;          // the relaunch's `mode` argument
    bool spread2 = false;   // the parked pixels are dealt heaviest first (else in slot order)
};

// `variant_blocks`: resident blocks of the kernel plan_schedule chose (s.v).
inline Grid plan_grid(const Schedule &s, long long variant_blocks) {
    Grid g;
    const long long need = (s.n_items * kClaimStride + 255) / 256;
    g.blocks = std::max<long long>(std::min(need, variant_blocks), 1);
    g.slots = g.blocks * 256;
    // vertex records are addressed with 32-bit byte offsets (rt_path.h LaneRec)
    if ((unsigned long long)g.slots * (unsigned long long)s.ray_depth * 32ull >= (1ull << 32)) {
        g.refused = {RT_ERR_LIMIT, "rt_render: vertex records beyond 4 GiB"};
        return g;
    }
    g.groups = 4 * g.blocks;
    if (s.handoff) {
        g.blocks2 = s.spec_blocks;
        g.waves2 = 4 * g.blocks2;   // (256-thread blocks)
        const Deal deal = resume_deal(g.slots, kHandoffPct, g.waves2);
        g.dealt = deal.dealt;
        g.per2 = deal.per;
        g.mode2 = mode_pack(0, kHandoffPct);
        // (with the pixel order's estimates at hand; the order buffer holds n_pixels per array)
        g.spread2 = kHandoffSpread && s.ordered && g.slots <= s.n_pixels;
    }
    return g;
}

}  // namespace rtp
