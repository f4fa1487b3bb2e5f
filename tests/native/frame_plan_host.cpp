// frame_plan_host.cpp — TEST ONLY: rt_frame_plan.h (the whole-frame render's plan and stats
// merge) behind a C interface for tests/test_frame_plan.py.  The header is host only, so this
// builds with plain g++; the visible device count is an input.
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_frame_plan.h"

extern "C" {

struct fp_in {
    int width, height, n_shards;
    const int32_t *devices;   // [n_shards] or null
    int row_block, spp, visible_devices, want_sums;
};

// The arrays are the caller's: dev_of, dev_index, rows, max_rows, sum_bytes, buf_bytes with room
// for cap_shards entries, uniq for 64 (rtp::kMaxDevices), base for cap_shards + 1, frame_row_of
// for `height`.  A plan with more shards than cap_shards fills the scalars only.
struct fp_out {
    int err;
    char msg[192];
    int n, n_uniq, root;
    int *dev_of, *uniq, *dev_index;
    long long *rows, *base;
    int32_t *frame_row_of;
    unsigned long long row_u8, row_f;
    unsigned long long o_stage_u8, o_frame_u8, o_stage_f, o_frame_f, o_row_map, root_bytes;
    long long *max_rows;                       // [n_uniq]
    unsigned long long *sum_bytes, *buf_bytes;  // [n_uniq]
};

static rtp::FramePlan plan_of(const fp_in *i) {
    rtp::FrameIn in;
    in.width = i->width;
    in.height = i->height;
    in.n_shards = i->n_shards;
    in.devices = i->devices;
    in.row_block = i->row_block;
    in.spp = i->spp;
    in.visible_devices = i->visible_devices;
    in.want_sums = i->want_sums != 0;
    return rtp::plan_frame(in);
}

int fp_plan(const fp_in *i, int cap_shards, fp_out *o) {
    const rtp::FramePlan f = plan_of(i);
    o->err = f.refused.code;
    std::memset(o->msg, 0, sizeof o->msg);
    std::strncpy(o->msg, f.refused.msg.c_str(), sizeof o->msg - 1);
    if (f.refused) return f.refused.code;
    o->n = f.n;
    o->n_uniq = (int)f.uniq.size();
    o->root = f.root();
    o->row_u8 = f.row_u8;
    o->row_f = f.row_f;
    o->o_stage_u8 = f.o_stage_u8;
    o->o_frame_u8 = f.o_frame_u8;
    o->o_stage_f = f.o_stage_f;
    o->o_frame_f = f.o_frame_f;
    o->o_row_map = f.o_row_map;
    o->root_bytes = f.root_bytes;
    if (f.n > cap_shards) return RT_OK;
    for (int r = 0; r < f.n; ++r) {
        o->dev_of[r] = f.dev_of[r];
        o->dev_index[r] = f.dev_index[r];
        o->rows[r] = f.rows[r];
        o->base[r] = f.base[r];
    }
    o->base[f.n] = f.base[f.n];
    for (size_t ui = 0; ui < f.uniq.size(); ++ui) {
        o->uniq[ui] = f.uniq[ui];
        o->max_rows[ui] = f.dev[ui].max_rows;
        o->sum_bytes[ui] = f.dev[ui].sum_bytes;
        o->buf_bytes[ui] = f.dev[ui].buf_bytes;
    }
    for (size_t k = 0; k < f.frame_row_of.size(); ++k) o->frame_row_of[k] = f.frame_row_of[k];
    return RT_OK;
}

// The frame's stats from shard_stats[n] under the plan of `i` (which must not be refused).
int fp_merge(const fp_in *i, const rt_stats *shard_stats, double gather_ms, rt_stats *out) {
    const rtp::FramePlan f = plan_of(i);
    if (f.refused) return f.refused.code;
    rtp::merge_frame_stats(f, shard_stats, gather_ms, out);
    return RT_OK;
}

}  // extern "C"
