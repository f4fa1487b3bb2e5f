// fast_units_host.cpp — TEST ONLY: rt_fast_units.h (the work units and the fold of a fast
// accumulator's pass) and the launch plan's fast-pass fields behind a C interface for
// tests/test_fast_accum.py.  Both headers are host-clean, so this builds with plain g++ (with
// -ffp-contract=off, as every unit that includes rt_fast_units.h).
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_fast_units.h"
#include "plan_io.h"

extern "C" {

int fu_units_of(int next, int target, int c) { return rtfu::units_of(next, target, c); }

void fu_unit_range(int next, int target, int c, int k, int *s0, int *s1) {
    const rtfu::Range u = rtfu::unit_range(next, target, c, k);
    *s0 = u.s0;
    *s1 = u.s1;
}

int fu_unit_continues(int next, int c, int k) { return rtfu::unit_continues(next, c, k); }

struct Parts {
    const float *p;
    float operator()(int k, int ch) const { return p[3 * k + ch]; }
};

// rec: next, total[3], open[3] as 7 words (floats by their bits); parts: units x 3 floats, unit
// k's partial (unit 0's started from rec's open when the pass starts inside a chunk: the caller
// makes it so).  Folds to `target`; the record after it in rec, its reported sum in sum.
void fu_fold(unsigned *rec, int target, int c, const float *parts, float *sum) {
    rtfu::Rec r;
    r.next = (int)rec[0];
    std::memcpy(r.total, rec + 1, 12);
    std::memcpy(r.open, rec + 4, 12);
    rtfu::fold(r, target, c, Parts{parts});
    rec[0] = (unsigned)r.next;
    std::memcpy(rec + 1, r.total, 12);
    std::memcpy(rec + 4, r.open, 12);
    rtfu::reported(r, c, sum);
}

int fu_open_words_fit(unsigned next, int c, const unsigned *open_words) { return rtfu::open_words_fit(next, c, open_words); }

int fu_max_chunks() { return rtp::kFastMaxChunks; }

// The launch plan (plan_io.h), for the fast-pass fields.
int fu_plan(const plan_in *i, plan_out *o) { return plan_fill(i, o); }

}  // extern "C"
