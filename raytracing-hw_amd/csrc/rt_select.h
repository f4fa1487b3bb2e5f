// rt_select.h — which pixels of an accumulator a subset pass raises (host and device, no HIP).
//
// rt_accum_select (include/rt_hw.h) chooses, per shard pixel, whether the next subset pass
// renders it up to the absolute sample `target`.  The rule takes plain values, so the device
// kernel (rt_accum_device.h rt_select_kernel) and the CPU test (tests/native/select_host.cpp) share
// this one text.  All arithmetic is f32 in the order written; every translation unit that
// includes it is built with -ffp-contract=off, and the device build with correctly rounded
// divide and sqrt, so host and device agree bit for bit.
//
// Names: n_b = the record's next sample (samples the pixel has), S_b = its current sum;
// n_a, S_a = the same two at the last rt_accum_mark (0 and unused without a mark).
//   1. outside the window, mask byte 0, or n_b >= target                    -> not selected
//   2. threshold <= 0                                                       -> selected
//   3. n_b == 0 or n_a == 0 (no estimate yet)                               -> selected
//      n_b == n_a (no new evidence since the pixel was last judged)         -> not selected
//   4. e = sum_c |mean of the samples since the mark - mean of those before| /
//          sqrt(sum_c mean of all + 1e-4);  selected iff e > threshold (a NaN e never is:
//      more samples cannot repair a non-finite sum).
// Rule 1's `n_b < target` is the liveness invariant of the chain kernels: an item
// whose record is at or past the pass's end sample would never finish.
#pragma once
#include <cmath>
#include <cstdint>

#include "rt_libm.h"

namespace rtsel {

// rt_select as plain values (the mask is passed per pixel).
struct Rule {
    int target;
    int x0, y0, x1, y1;   // frame window, half-open; all 0 = whole frame
    float threshold;      // <= 0: no error test
};

RT_HD bool whole_frame(const Rule &r) { return r.x0 == 0 && r.y0 == 0 && r.x1 == 0 && r.y1 == 0; }

RT_HD bool in_window(const Rule &r, int x, int y) {
    return whole_frame(r) || (x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1);
}

// Step 4's estimate; needs 0 < n_a < n_b.  Two independent means (the samples before the mark
// and the samples since), normalised like the half-buffer criterion of Dammertz et al.
RT_HD float error_estimate(int n_a, const float *S_a, int n_b, const float *S_b) {
    const float ra = 1.f / (float)n_a, rn = 1.f / (float)(n_b - n_a), rb = 1.f / (float)n_b;
    float d[3], mb[3];
    for (int c = 0; c < 3; ++c) {
        const float ma = S_a[c] * ra;
        const float mn = (S_b[c] - S_a[c]) * rn;
        mb[c] = S_b[c] * rb;
        d[c] = std::fabs(mn - ma);
    }
    return ((d[0] + d[1]) + d[2]) / std::sqrt(((mb[0] + mb[1]) + mb[2]) + 1e-4f);
}

// The rule.  mask_byte: the pixel's byte of rt_select.mask (any non-zero value without a mask).
RT_HD bool selected(const Rule &r, int x, int y, unsigned mask_byte, int n_b, const float *S_b, int n_a,
                    const float *S_a) {
    if (!in_window(r, x, y) || mask_byte == 0u || n_b >= r.target) return false;
    if (!(r.threshold > 0.f)) return true;
    if (n_b == 0 || n_a == 0) return true;
    if (n_b == n_a) return false;
    return error_estimate(n_a, S_a, n_b, S_b) > r.threshold;   // (false for a NaN estimate)
}

// Argument checks of rt_accum_select that need no device: 0 = fine, 1 = RT_ERR_ARG, 2 = RT_ERR_LIMIT.
inline int check_rule(const Rule &r, int width, int height) {
    if (r.target < 1) return 1;
    if (r.target >= (1 << 20)) return 2;
    if (whole_frame(r)) return 0;
    if (r.x0 < 0 || r.y0 < 0 || r.x1 < r.x0 || r.y1 < r.y0 || r.x1 > width || r.y1 > height) return 1;
    return 0;
}

// The per-pixel frame finish of a sample-count map (rt_tonemap_u8_counts): the reciprocal the
// sum is multiplied by, as rt_tonemap_u8 multiplies by 1.f / (float)spp; 0 samples: 0.
RT_HD float count_normalizer(int n) { return n > 0 ? 1.f / (float)n : 0.f; }

}  // namespace rtsel
