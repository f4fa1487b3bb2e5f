// plan_io.h — TEST ONLY: rt_launch_plan.h's inputs and results as plain C structs, and the one
// copy in and out of them (plan_fill).  plan_host.cpp, select_host.cpp and fast_units_host.cpp
// export it under their own names; tests/plan_util.py holds the matching ctypes structures.  A new
// plan field is added here and there.
#pragma once
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_launch_plan.h"

extern "C" {

struct plan_in {
    int flags, kernel, count, fast_chunk, spp, pass_spp;
    long long n_pixels;
    int ray_depth, n_nodes;
    long long spec_blocks;      // resident blocks of the runahead kernel
    long long variant_blocks;   // resident blocks of the kernel step one chooses (the caller knows which)
    long long subset_items;
    int fast_accum, fast_units, moments;
};

struct plan_out {
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
    int v_mom, variant_index, mode, mode2;
    char msg[192];
};

}  // extern "C"

inline int plan_refuse(const rtp::Refusal &r, plan_out *o) {
    o->err = r.code;
    std::strncpy(o->msg, r.msg.c_str(), sizeof o->msg - 1);
    return r.code;
}

// plan_schedule, then plan_grid for a lane-resident launch; returns o->err.
inline int plan_fill(const plan_in *i, plan_out *o) {
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
    in.subset_items = i->subset_items;
    in.fast_accum = i->fast_accum != 0;
    in.fast_units = i->fast_units;
    in.moments = i->moments != 0;
    const rtp::Schedule s = rtp::plan_schedule(in);
    if (s.refused) return plan_refuse(s.refused, o);
    o->lane = s.lane;
    o->v_count = s.v.count;
    o->v_fast = s.v.fast;
    o->v_lsplit = s.v.lsplit;
    o->v_spec = s.v.spec;
    o->v_chain = s.v.chain;
    o->v_mom = s.v.mom;
    o->variant_index = rtp::variant_index(s.v);
    o->sched = s.sched;
    o->handoff = s.handoff;
    o->mode = s.mode;
    o->ordered = s.ordered;
    o->cs = s.cs;
    o->chunks = s.chunks;
    o->n_items = s.n_items;
    o->round_min = s.round_min;
    o->stats_spp = s.stats_spp;
    if (!s.lane) return RT_OK;
    const rtp::Grid g = rtp::plan_grid(s, i->variant_blocks);
    if (g.refused) return plan_refuse(g.refused, o);
    o->blocks = g.blocks;
    o->slots = g.slots;
    o->groups = g.groups;
    o->per = g.per;
    o->blocks2 = g.blocks2;
    o->waves2 = g.waves2;
    o->dealt = g.dealt;
    o->per2 = g.per2;
    o->spread2 = g.spread2;
    o->mode2 = g.mode2;
    return RT_OK;
}
