// rt_fast_units.h — the work units of a fast accumulator's pass (host and device, no HIP).
//
// A fast accumulator (include/rt_hw.h rt_accum_create_fast) has a chunk size c >= 1, fixed for
// its life: chunk j of a pixel is its samples [j c, (j + 1) c), whatever the passes' sizes.  A
// pixel with n samples holds the partials of its chunks added in chunk order, the oracle's
// rt_oracle_render_fast(spp = n, chunk = c).  Per pixel the record keeps
//   next    the samples it has;
//   total   the fold, from +0.f, of the partials of all complete chunks, in chunk order;
//   open    the running partial of the chunk that contains `next` when next % c != 0, else
//           zero words;
// and its reported sum is `total` when next % c == 0, else total + open (always added: the
// oracle's `total += part` of a ragged last chunk).
//
// A pass raises a pixel from `next` to `target`.  Its units are the chunks that [next, target)
// overlaps, unit k being chunk next / c + k cut to the pass; unit 0 of a pixel that starts
// inside a chunk starts from `open`, so its partial already holds it.  The render kernel
// (rt_mega.h mega_assign_fast_chain) asks unit_range, rt_fast_fold_chain_kernel folds the
// partials with fold(); tests/native/fast_units_host.cpp runs the same text on the CPU.  Every
// translation unit that includes it is built with -ffp-contract=off; the arithmetic is f32
// additions in the order written.
#pragma once
#include <cstdint>

#include "rt_libm.h"

namespace rtfu {

// Samples [s0, s1) of one pixel; empty when s0 >= s1.
struct Range {
    int s0, s1;
};

// The chunks [next, target) overlaps; 0 when there is nothing to render.
RT_HD int units_of(int next, int target, int c) { return next >= target ? 0 : (target - 1) / c - next / c + 1; }

// Unit k of the pass [next, target): chunk j = next / c + k, cut to the pass.  Empty for k at or
// past units_of(next, target, c): an item of a launch sized for a pixel further behind.
RT_HD Range unit_range(int next, int target, int c, int k) {
    const long long j = (long long)(next / c) + k;
    const long long lo = j * c, hi = lo + c;
    return Range{(int)(lo > next ? (lo < target ? lo : target) : next), (int)(hi < target ? hi : target)};
}

// Unit k of that pass starts from the record's `open` (else from +0.f).
RT_HD bool unit_continues(int next, int c, int k) { return k == 0 && next % c != 0; }

// The record's arithmetic part (its words: rt_records.h).
struct Rec {
    int next;
    float total[3], open[3];
};

// The pixel's units rendered, partial of unit k and channel ch = part(k, ch): the record after
// the pass.  A unit whose chunk is complete at `target` adds into `total`, in order; a last unit
// whose chunk is not becomes `open`.  next >= target: the record as it was.
template <class Part>
RT_HD void fold(Rec &r, int target, int c, const Part &part) {
    const int K = units_of(r.next, target, c);
    for (int k = 0; k < K; ++k) {
        const Range u = unit_range(r.next, target, c, k);
        const bool complete = u.s1 % c == 0;
        for (int ch = 0; ch < 3; ++ch) {
            const float v = part(k, ch);
            if (complete) {
                r.total[ch] += v;
                r.open[ch] = 0.f;
            } else {
                r.open[ch] = v;
            }
        }
    }
    if (K > 0) r.next = target;
}

// The sum the accumulator reports for the record.
RT_HD void reported(const Rec &r, int c, float *out) {
    for (int ch = 0; ch < 3; ++ch) out[ch] = r.next % c == 0 ? r.total[ch] : r.total[ch] + r.open[ch];
}

// Checkpoint check: the record's `open` words are zero where no chunk is open (rt_records.h
// open_words_fit finds them in a whole record).
RT_HD bool open_words_fit(uint32_t next, int c, const uint32_t *open_words) {
    return next % (uint32_t)c != 0u || (open_words[0] | open_words[1] | open_words[2]) == 0u;
}

}  // namespace rtfu
