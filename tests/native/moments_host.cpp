// moments_host.cpp — TEST ONLY: the CPU ground truth of a moments accumulator
// (raytracing-hw_amd/csrc/rt_moments.h).  It returns the fast colour of sample s of pixel p from
// the render kernels' own source compiled for the host (rt_path.h: fast_sample_seed, rng_offset,
// camera_ray, trace_sample, the text kernel_host.cpp's kh_render runs), and puts the rt_moments.h
// functions and rt_fast_units.h's fold, on colours or on their squares, behind a C interface for
// tests/test_moments.py and tests/test_gpu_moments.py.  Not part of the product.
#include "mega_emu.h"
#include "../../raytracing-hw_amd/csrc/rt_moments.h"

using namespace emu;

extern "C" {

// The fast colours of samples [s0, s1) of frame pixels [p0, p1) (p = j * W + i), three floats
// each, pixel-major: out[((p - p0) * (s1 - s0) + (s - s0)) * 3 + ch].
void mh_colours(const rt_scene_view *v, long long p0, long long p1, int s0, int s1, float *out) {
    const rtd::DevScene sc = make(v);
    const int ns = s1 - s0;
#pragma omp parallel for schedule(dynamic, 16)
    for (long long p = p0; p < p1; ++p) {
        const int i = (int)(p % sc.width), j = (int)(p / sc.width);
        rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
        for (int s = s0; s < s1; ++s) {
            rtd::Rng rng{rtd::fast_sample_seed((uint32_t)p, (uint32_t)s), 0u, 0.f};
            const float ox = rtd::rng_offset(rng);
            const float oy = rtd::rng_offset(rng);
            const rtd::Ray r = rtd::camera_ray(sc, i, j, ox, oy);
            const rtv::V3 c = rtd::trace_sample<false>(sc, r, rng, cnt);
            float *o = out + ((p - p0) * ns + (s - s0)) * 3;
            o[0] = c.x;
            o[1] = c.y;
            o[2] = c.z;
        }
    }
}

// One pixel's pass [rec.next, target) as the render kernel and the fold kernel run it: unit k's
// partial is its samples added in order onto +0.f, or onto the record's open partial where
// unit_continues says so, then rtfu::fold.  x: the colours of samples [rec.next, target), three
// floats each; square != 0: their squares (rtmo::square) are folded instead.  rec: next,
// total[3], open[3] as 7 words; the record after the pass in rec, its reported value in out.
void mh_fold(unsigned *rec, int target, int c, const float *x, int square, float *out) {
    rtfu::Rec r;
    r.next = (int)rec[0];
    std::memcpy(r.total, rec + 1, 12);
    std::memcpy(r.open, rec + 4, 12);
    const int next = r.next, K = rtfu::units_of(next, target, c);
    std::vector<float> parts((size_t)(K > 0 ? K : 1) * 3, 0.f);
    for (int k = 0; k < K; ++k) {
        const rtfu::Range u = rtfu::unit_range(next, target, c, k);
        float part[3] = {0.f, 0.f, 0.f};
        if (rtfu::unit_continues(next, c, k)) std::memcpy(part, r.open, 12);
        for (int s = u.s0; s < u.s1; ++s) {
            float q[3];
            if (square) rtmo::square(x + 3 * (size_t)(s - next), q);
            else std::memcpy(q, x + 3 * (size_t)(s - next), 12);
            for (int ch = 0; ch < 3; ++ch) part[ch] += q[ch];
        }
        std::memcpy(&parts[3 * (size_t)k], part, 12);
    }
    const float *pp = parts.data();
    rtfu::fold(r, target, c, [pp](int k, int ch) { return pp[3 * k + ch]; });
    rec[0] = (unsigned)r.next;
    std::memcpy(rec + 1, r.total, 12);
    std::memcpy(rec + 4, r.open, 12);
    rtfu::reported(r, c, out);
}

float mh_variance_of_mean(int n, const float *S, const float *Q, const float *albedo, int hit) {
    return rtmo::variance_of_mean(n, S, Q, albedo, hit != 0);
}

float mh_relative_error(int n, const float *S, const float *Q) { return rtmo::relative_error(n, S, Q); }

// Per channel the mean and the variance of the mean (n >= 2), for the cancellation bound.
void mh_mean_and_variance(int n, const float *S, const float *Q, float *m, float *vm) { rtmo::mean_and_variance(n, S, Q, m, vm); }

int mh_selected(int target, int x0, int y0, int x1, int y1, float threshold, int x, int y, unsigned mask_byte, int n_b,
                const float *S_b, const float *Q_b) {
    return rtmo::selected(rtsel::Rule{target, x0, y0, x1, y1, threshold}, x, y, mask_byte, n_b, S_b, Q_b);
}

int mh_record_words_fit(unsigned next, int c, const unsigned *words) { return rtmo::record_words_fit(next, c, words); }

}  // extern "C"
