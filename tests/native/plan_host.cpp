// plan_host.cpp — TEST ONLY: rt_launch_plan.h (the render's launch plan) behind a C interface
// for tests/test_launch_plan.py.  The header is host only, so this builds with plain g++; the
// resident block counts the device would report are inputs.  ph_mode_* and ph_deal are the rules
// the header names once for the plan, the kernel and the kernel's host emulation.
#include "plan_io.h"

extern "C" {

int ph_plan(const plan_in *i, plan_out *o) { return plan_fill(i, o); }

int ph_mode_pack(int park_below, int resume_pct) { return rtp::mode_pack(park_below, resume_pct); }
void ph_mode_unpack(int mode, int *park_below, int *resume_pct) {
    *park_below = rtp::mode_park_below(mode);
    *resume_pct = rtp::mode_resume_pct(mode);
}
void ph_deal(long long slots, int pct, long long waves, long long *dealt, long long *per) {
    const rtp::Deal d = rtp::resume_deal(slots, pct, waves);
    *dealt = d.dealt;
    *per = d.per;
}

}  // extern "C"
