// fast_units_host.cpp — TEST ONLY: rt_fast_units.h (the work units and the fold of a fast
// accumulator's pass) and the launch plan's fast-pass fields behind a C interface for
// tests/test_fast_accum.py.  Both headers are host-clean, so this builds with plain g++ (with
// -ffp-contract=off, as every unit that includes rt_fast_units.h).
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_fast_units.h"
#include "../../raytracing-hw_amd/csrc/rt_launch_plan.h"

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

// plan_host.cpp's input with the fields that came later, and its output.
struct fu_in {
    int flags, kernel, count, fast_chunk, spp, pass_spp;
    long long n_pixels;
    int ray_depth, n_nodes;
    long long spec_blocks, variant_blocks, subset_items;
    int fast_accum, fast_units;
};

struct fu_out {
    int err, lane;
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

int fu_plan(const fu_in *i, fu_out *o) {
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
    const rtp::Schedule s = rtp::plan_schedule(in);
    if (s.refused) {
        o->err = s.refused.code;
        std::strncpy(o->msg, s.refused.msg.c_str(), sizeof o->msg - 1);
        return o->err;
    }
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
    if (g.refused) {
        o->err = g.refused.code;
        std::strncpy(o->msg, g.refused.msg.c_str(), sizeof o->msg - 1);
        return o->err;
    }
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

}  // extern "C"
