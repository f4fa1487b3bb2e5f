// rt_accum_plan.h — what an accumulator is and what its passes launch, decided from plain values
// (host only, no HIP).
//
// rt_device.hip's rt_accum_* entries keep the device buffers and launch.  What needs no device is
// here and runs without one (tests/test_accum_plan.py): the three kinds, what each refuses to
// render with, the host state, the passes of rt_accum_add / rt_accum_add_selected, how a long
// fast pass is cut into launches.  The kinds' checkpoint file is rt_accum_file.h.
#pragma once
#include <cstdint>
#include <string>

#include "rt_fast_units.h"
#include "rt_launch_plan.h"

namespace rtap {

using rtp::Refusal;

// Parity: the reference's sums bit for bit (rt_accum_create).  Fast: Philox units of a fixed chunk
// size (rt_accum_create_fast, rt_fast_units.h).  Moments: a fast one that also keeps the
// per-sample second moments (rt_accum_create_fast_moments, rt_moments.h).
enum class Kind { Parity, Fast, Moments };

// A kind's checkpoint file: magic, version, bytes per pixel (a moments file: two records).
struct KindInfo {
    char magic[8];
    uint32_t version;
    int record_bytes;
    bool fast;
};
constexpr KindInfo kKinds[3] = {
    {{'R', 'T', 'A', 'C', 'C', 'U', 'M', '\0'}, 1, 32, false},
    {{'R', 'T', 'F', 'A', 'C', 'C', 'U', 'M'}, 1, 32, true},
    {{'R', 'T', 'M', 'A', 'C', 'C', 'U', 'M'}, 1, 64, true},
};
constexpr const KindInfo &info(Kind k) { return kKinds[(int)k]; }

// What an accumulator renders with (after the unknown-flag check of its entry).  Parity: a parity
// render on the lane-resident kernel.  Fast kinds: fast units on that kernel; the order flags and
// RT_FLAG_NO_RUNAHEAD are accepted and ignored (fast units are never ordered and have no chain to
// run ahead of), RT_FLAG_FAST may be set or not.
inline Refusal check_params(Kind kind, int flags, int count, int kernel, int fast_chunk, const std::string &who) {
    const auto flag_refusal = [&]() -> Refusal {
        if (flags & RT_FLAG_LIGHT_SPLIT) return {RT_ERR_ARG, who + ": the light-split kernel has no accumulator"};
        if (flags & RT_FLAG_KERNEL_TIMES) return {RT_ERR_ARG, who + ": RT_FLAG_KERNEL_TIMES is a wavefront option; accumulators run on kernel 0"};
        return {};
    };
    const auto shape_refusal = [&]() -> Refusal {
        if (count != 0) return {RT_ERR_ARG, who + ": counting renders have no accumulator (count must be 0)"};
        if (kernel != RT_KERNEL_LANE) return {RT_ERR_ARG, who + ": accumulators run on the lane-resident kernel only (kernel 0)"};
        return {};
    };
    if (info(kind).fast) {
        if (Refusal r = shape_refusal()) return r;
        if (Refusal r = flag_refusal()) return r;
        if (fast_chunk < 0) return {RT_ERR_ARG, who + ": fast_chunk must be >= 0"};
        return {};
    }
    if (flags & RT_FLAG_FAST)
        return {RT_ERR_ARG, who + ": fast mode has no accumulator here (a one-shot fast sum is defined per (spp, fast_chunk)); "
                                  "use rt_accum_create_fast"};
    if (Refusal r = flag_refusal()) return r;
    if (Refusal r = shape_refusal()) return r;
    if (rtp::order_flags_conflict(flags))
        return {RT_ERR_ARG, who + ": RT_FLAG_NATURAL_ORDER and RT_FLAG_HEAVY_ORDER exclude each other"};
    return {};
}

// The host state of an accumulator (rt_accum embeds it).
struct State {
    // The largest and the smallest per-pixel sample count: equal until a subset pass leaves pixels behind.
    int samples = 0, min_samples = 0;
    int fast_c = 0;          // a fast accumulator's chunk size, fixed for its life; 0 = parity
    bool has_mark = false;   // rt_accum_mark's copy exists (none after create / load)
    // rt_accum_select's pending list, dropped by every pass: the listed pixels, the samples they
    // lack, the target, the counts' range after the pass, the smallest count among the listed.
    bool sel_pending = false;
    long long sel_n = 0;
    unsigned long long sel_samples = 0;
    int sel_target = 0, sel_min = 0, sel_max = 0, sel_from = 0;

    bool uniform() const { return min_samples == samples; }
};

// A pass: the items (every pixel, or the pending list's n_items) raised to `target`, the one
// furthest behind standing at `from` (a fast pass's units per item come from it).
struct Pass {
    Refusal refused;
    bool launch = true;   // false: an empty selection, nothing to raise
    int from = 0, target = 0;
    bool items = false;   // the pending selection's list is the item list, of n_items
    long long n_items = 0;
    int n = 0;            // a parity pass's marker in the launch plan (pass_spp): the samples a full pass adds, 1 for a subset
    unsigned long long samples = 0;   // rt_stats.samples of the pass
};

// rt_accum_add: n_samples more for every one of the shard's n_pixels.  An accepted pass drops the
// pending selection (it changes the records the list was made from).
inline Pass plan_add(State &s, int n_samples, long long n_pixels) {
    Pass ps;
    if (n_samples < 1) ps.refused = {RT_ERR_ARG, "rt_accum_add: n_samples must be >= 1"};
    else if ((long long)s.samples + n_samples >= (1 << 20))
        ps.refused = {RT_ERR_LIMIT, "rt_accum_add: total samples per pixel must be < 2^20"};
    else if (!s.uniform())
        ps.refused = {RT_ERR_ARG, "rt_accum_add: the pixels hold between " + std::to_string(s.min_samples) + " and " +
                                      std::to_string(s.samples) + " samples; level them first: rt_accum_select with target = " +
                                      std::to_string(s.samples) + " and no threshold, then rt_accum_add_selected"};
    if (ps.refused) return ps;
    s.sel_pending = false;
    ps.from = s.samples, ps.target = s.samples + n_samples, ps.n = n_samples;
    ps.samples = (unsigned long long)n_pixels * (unsigned long long)n_samples;
    return ps;
}

// rt_accum_add_selected: the pending list's pixels raised to the selection's target.  The
// selection is dropped whether the pass is launched or not.
inline Pass plan_add_selected(State &s) {
    Pass ps;
    if (!s.sel_pending) {
        ps.refused = {RT_ERR_ARG, "rt_accum_add_selected: no pending selection (rt_accum_select first; every pass drops it)"};
        return ps;
    }
    s.sel_pending = false;
    ps.launch = s.sel_n != 0;
    ps.from = s.sel_from, ps.target = s.sel_target;   // (the listed pixel furthest behind, below the target by the rule)
    ps.items = true, ps.n_items = s.sel_n, ps.n = 1, ps.samples = s.sel_samples;
    return ps;
}

// A fast pass from `from` (the smallest count among its items) to `target`: one launch carries at
// most kFastMaxChunks units per item, so a longer pass runs as successive complete passes (render
// + fold) to chunk boundaries on the way; same bits, the records carry everything.  Where the
// launch that starts at `from` ends: the target, or the end of its last whole chunk.
inline int next_launch(int from, int target, int c) {
    if (rtfu::units_of(from, target, c) <= rtp::kFastMaxChunks) return target;
    return (int)(((long long)(from / c) + rtp::kFastMaxChunks) * c);
}

// The state once the pass is queued.
inline void commit_add(State &s, const Pass &ps) {
    s.samples = s.min_samples = ps.target;
    s.sel_pending = false;
}
inline void commit_selected(State &s) {
    s.samples = s.sel_max;
    s.min_samples = s.sel_min;
    s.sel_pending = false;
}

}  // namespace rtap
