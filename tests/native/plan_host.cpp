// plan_host.cpp — TEST ONLY: rt_launch_plan.h (the render's launch plan) behind a C interface
// for tests/test_launch_plan.py.  The header is host only, so this builds with plain g++; the
// resident block counts the device would report are inputs.  ph_mode_* and ph_deal are the rules
// the header names once for the plan, the kernel and the kernel's host emulation.
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_launch_plan.h"

extern "C" {

struct ph_in {
    int flags, kernel, count, fast_chunk, spp, pass_spp;
    long long n_pixels;
    int ray_depth, n_nodes;
    long long spec_blocks;      // resident blocks of the runahead kernel
    long long variant_blocks;   // resident blocks of the kernel step one chooses (the caller knows which)
};

struct ph_out {
    int err;                    // the refusal of either step (RT_OK: none)
    int lane;
    int v_count, v_fast, v_lsplit, v_spec, v_chain;
    unsigned long long sched;
    int handoff, ordered, cs, chunks;
    long long n_items;
    int round_min, stats_spp;
    long long blocks, slots, groups, per;
    long long blocks2, waves2, dealt, per2;
    int spread2;
    char msg[192];
};

static int refuse(const rtp::Refusal &r, ph_out *o) {
    o->err = r.code;
    std::strncpy(o->msg, r.msg.c_str(), sizeof o->msg - 1);
    return r.code;
}

int ph_plan(const ph_in *i, ph_out *o) {
    std::memset(o, 0, sizeof *o);
    rtp::PlanIn in;
    in.flags = i->flags;
    in.kernel = i->kernel;
    in.count = i->count;
    in.fast_chunk = i->fast_chunk;
    in.spp = i->spp;
    in.pass_spp = i->pass_spp;
    in.n_pixels = i->n_pixels;
    in.ray_depth = i->ray_depth;
    in.n_nodes = i->n_nodes;
    in.spec_blocks = i->spec_blocks;
    const rtp::Schedule s = rtp::plan_schedule(in);
    if (s.refused) return refuse(s.refused, o);
    o->lane = s.lane;
    o->v_count = s.v.count;
    o->v_fast = s.v.fast;
    o->v_lsplit = s.v.lsplit;
    o->v_spec = s.v.spec;
    o->v_chain = s.v.chain;
    o->sched = s.sched;
    o->handoff = s.handoff;
    o->ordered = s.ordered;
    o->cs = s.cs;
    o->chunks = s.chunks;
    o->n_items = s.n_items;
    o->round_min = s.round_min;
    o->stats_spp = s.stats_spp;
    if (!s.lane) return RT_OK;
    const rtp::Grid g = rtp::plan_grid(s, i->variant_blocks);
    if (g.refused) return refuse(g.refused, o);
    o->blocks = g.blocks;
    o->slots = g.slots;
    o->groups = g.groups;
    o->per = g.per;
    o->blocks2 = g.blocks2;
    o->waves2 = g.waves2;
    o->dealt = g.dealt;
    o->per2 = g.per2;
    o->spread2 = g.spread2;
    return RT_OK;
}

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
