// rt_moments.h — per-sample second moments of a fast accumulator (host and device, no HIP).
//
// A moments accumulator (include/rt_hw.h rt_accum_create_fast_moments) keeps, beside the sum S of
// a pixel's sample colours x, the sum Q of their squares: for sample s with colour x (the three
// f32 values fold_path returns) q[ch] = x[ch] * x[ch], one f32 multiply.  Q is the fast fold of q
// exactly as S is the fast fold of x (rt_fast_units.h): the partials of a chunk are added in
// sample order from +0.f, the chunk partials in chunk order from +0.f, and an open chunk is
// carried as `open2` and reported as total2 + open2 when n % c != 0.  The moment record is a
// second rtfu::Rec, folded by rtfu::fold and reported by rtfu::reported: there is no second fold.
// Non-finite samples give non-finite moments; nothing is clamped here.
//
// From (n, S, Q) two estimates are defined, shared by the device kernels (rt_denoise_device.h
// rt_variance_kernel, rt_accum_device.h rt_select_kernel's variance form), the host entry
// (rt_variance_from_moments) and the CPU test (tests/native/moments_host.cpp).  All arithmetic is
// f32 in the order written; every translation unit that includes this file is built with
// -ffp-contract=off, and the device build with correctly rounded divide and sqrt, so host and
// device agree bit for bit.
//
// Known limit: v = Q / n - (S / n)^2 cancels in f32.  Each of the two terms carries at most n + 2
// roundings, so the absolute error of the variance of the mean is bounded by
// 4 (n + 2) 2^-24 (Q / n) / (n - 1) (a factor 2 of margin included; tests/test_moments.py checks
// it against a float64 two-pass variance).  Where the true variance is far below the mean square
// (a nearly constant pixel) the estimate is noise of that size, clamped at 0 from below.
#pragma once
#include <cmath>
#include <cstdint>

#include "rt_records.h"
#include "rt_select.h"

namespace rtmo {

constexpr float kAlbedoFloor = 1e-3f;   // (rt_denoise.h's floor: the demodulation the filter applies)

RT_HD bool finite(float v) { return (rtm::f2u(v) & 0x7f800000u) != 0x7f800000u; }

// One sample's moment.
RT_HD void square(const float *x, float *q) {
    for (int ch = 0; ch < 3; ++ch) q[ch] = x[ch] * x[ch];
}

// Per channel, for n >= 2: the mean m and the variance of the mean vm (the sample variance over
// n - 1, clamped at 0 from below).
RT_HD void mean_and_variance(int n, const float *S, const float *Q, float *m, float *vm) {
    const float r = 1.f / (float)n, r1 = 1.f / (float)(n - 1);
    for (int ch = 0; ch < 3; ++ch) {
        m[ch] = S[ch] * r;
        const float e2 = Q[ch] * r;
        float v = e2 - m[ch] * m[ch];
        v = v > 0.f ? v : 0.f;
        vm[ch] = v * r1;
    }
}

// The denoiser's `variance` input (rt_denoise_guided): the variance of the demodulated mean,
// summed over the channels.  A miss, n < 2 or a non-finite result: 0.
RT_HD float variance_of_mean(int n, const float *S, const float *Q, const float *albedo, bool hit) {
    if (!hit || n < 2) return 0.f;
    float m[3], vm[3], d[3];
    mean_and_variance(n, S, Q, m, vm);
    for (int ch = 0; ch < 3; ++ch) {
        const float a = albedo[ch] > kAlbedoFloor ? albedo[ch] : kAlbedoFloor;
        d[ch] = vm[ch] / (a * a);
    }
    const float V = (d[0] + d[1]) + d[2];
    return finite(V) ? V : 0.f;
}

// The selection's estimate (rt_accum_select_variance); needs n >= 2.  The standard error of the
// mean, normalised as rtsel::error_estimate is.
RT_HD float relative_error(int n, const float *S, const float *Q) {
    float m[3], vm[3];
    mean_and_variance(n, S, Q, m, vm);
    return ((std::sqrt(vm[0]) + std::sqrt(vm[1])) + std::sqrt(vm[2])) / std::sqrt(((m[0] + m[1]) + m[2]) + 1e-4f);
}

// rt_accum_select_variance's rule: steps 1 and 2 of rt_select.h's, then
//   n_b < 2 (no estimate yet)                         -> selected
//   otherwise selected iff relative_error > threshold (a NaN estimate never is).
// No mark is read.
RT_HD bool selected(const rtsel::Rule &r, int x, int y, unsigned mask_byte, int n_b, const float *S_b, const float *Q_b) {
    if (!rtsel::in_window(r, x, y) || mask_byte == 0u || n_b >= r.target) return false;
    if (!(r.threshold > 0.f)) return true;
    if (n_b < 2) return true;
    return relative_error(n_b, S_b, Q_b) > r.threshold;
}

// The first-hit record's (rt_gbuffer.h) part the variance needs: words 4-6 the base colour, word
// 7 the triangle id as int bits (negative: a miss).
RT_HD float variance_of_pixel(int n, const float *S, const float *Q, const float *grecord) {
    return variance_of_mean(n, S, Q, grecord + 4, (int32_t)rtm::f2u(grecord[7]) >= 0);
}

// Checkpoint check of a moment record: its open and pad words are zero where no chunk is open.
using rtrec::record_words_fit;   // (the words and their names: rt_records.h)

}  // namespace rtmo
