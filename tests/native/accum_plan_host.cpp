// accum_plan_host.cpp — TEST ONLY: rt_accum_plan.h (the accumulator's kinds, parameter checks,
// host state and passes) and rt_accum_file.h (its checkpoint file) behind a C interface for
// tests/test_accum_plan.py.  Both headers are host only, so this builds with plain g++ (with
// -ffp-contract=off, as every unit that includes rt_fast_units.h).
#include <cstring>

#include "../../raytracing-hw_amd/csrc/rt_accum_file.h"

extern "C" {

struct ap_kind {
    char magic[8];
    unsigned version;
    int record_bytes, fast;
};

void ap_kind_info(int kind, ap_kind *o) {
    const rtap::KindInfo &k = rtap::info((rtap::Kind)kind);
    std::memcpy(o->magic, k.magic, 8);
    o->version = k.version;
    o->record_bytes = k.record_bytes;
    o->fast = k.fast;
}

static int refusal_out(const rtp::Refusal &r, char *msg, size_t cap) {
    std::memset(msg, 0, cap);
    std::strncpy(msg, r.msg.c_str(), cap - 1);
    return r.code;
}

int ap_check_params(int kind, int flags, int count, int kernel, int fast_chunk, const char *who, char *msg256) {
    return refusal_out(rtap::check_params((rtap::Kind)kind, flags, count, kernel, fast_chunk, who), msg256, 256);
}

struct ap_state {
    int samples, min_samples, fast_c, has_mark, sel_pending;
    long long sel_n;
    unsigned long long sel_samples;
    int sel_target, sel_min, sel_max, sel_from;
};

struct ap_pass {
    int err;
    char msg[256];
    int launch, from, target, items;
    long long n_items;
    int n;
    unsigned long long samples;
};

static rtap::State state_in(const ap_state *i) {
    rtap::State s;
    s.samples = i->samples;
    s.min_samples = i->min_samples;
    s.fast_c = i->fast_c;
    s.has_mark = i->has_mark != 0;
    s.sel_pending = i->sel_pending != 0;
    s.sel_n = i->sel_n;
    s.sel_samples = i->sel_samples;
    s.sel_target = i->sel_target;
    s.sel_min = i->sel_min;
    s.sel_max = i->sel_max;
    s.sel_from = i->sel_from;
    return s;
}

static void state_out(const rtap::State &s, ap_state *o) {
    *o = ap_state{s.samples,   s.min_samples, s.fast_c,  s.has_mark, s.sel_pending, s.sel_n,
                  s.sel_samples, s.sel_target,  s.sel_min, s.sel_max,  s.sel_from};
}

static rtap::Pass pass_in(const ap_pass *i) {
    rtap::Pass ps;
    ps.launch = i->launch != 0;
    ps.from = i->from;
    ps.target = i->target;
    ps.items = i->items != 0;
    ps.n_items = i->n_items;
    ps.n = i->n;
    ps.samples = i->samples;
    return ps;
}

static int pass_out(const rtap::Pass &ps, ap_pass *o) {
    o->err = refusal_out(ps.refused, o->msg, sizeof o->msg);
    o->launch = ps.launch;
    o->from = ps.from;
    o->target = ps.target;
    o->items = ps.items;
    o->n_items = ps.n_items;
    o->n = ps.n;
    o->samples = ps.samples;
    return o->err;
}

// The plans take the state and leave it as the plan left it (the pending selection dropped).
int ap_plan_add(ap_state *s, int n_samples, long long n_pixels, ap_pass *o) {
    rtap::State st = state_in(s);
    const int rc = pass_out(rtap::plan_add(st, n_samples, n_pixels), o);
    state_out(st, s);
    return rc;
}

int ap_plan_add_selected(ap_state *s, ap_pass *o) {
    rtap::State st = state_in(s);
    const int rc = pass_out(rtap::plan_add_selected(st), o);
    state_out(st, s);
    return rc;
}

void ap_commit_add(ap_state *s, const ap_pass *ps) {
    rtap::State st = state_in(s);
    rtap::commit_add(st, pass_in(ps));
    state_out(st, s);
}

void ap_commit_selected(ap_state *s) {
    rtap::State st = state_in(s);
    rtap::commit_selected(st);
    state_out(st, s);
}

int ap_next_launch(int from, int target, int c) { return rtap::next_launch(from, target, c); }
int ap_units_of(int from, int target, int c) { return rtfu::units_of(from, target, c); }
int ap_max_chunks() { return rtp::kFastMaxChunks; }

// ---------------------------------------------------------------- the file
struct ap_facts {
    int width, height, ray_depth;
    unsigned n_tris, n_nodes, n_lights;
    float cam[14];
};

static rtaf::SceneFacts facts_in(const ap_facts *i) {
    rtaf::SceneFacts f{i->width, i->height, i->ray_depth, i->n_tris, i->n_nodes, i->n_lights, {}};
    std::memcpy(f.cam, i->cam, sizeof f.cam);
    return f;
}

// The writer as rt_accum_save drives it: header_of, the shard and count fields, write.
// rec / mom: n_pixels x 8 words (mom only for a moments file).  0, or -1 on a failed write.
int ap_write(const char *path, int kind, const ap_facts *facts, int rank, int world, int row_block, long long n_pixels,
             int samples, int per_pixel, int fast_c, const unsigned *rec, const unsigned *mom) {
    rtaf::AccumHeader h = rtaf::header_of(facts_in(facts), (rtap::Kind)kind);
    h.rank = rank, h.world = world, h.row_block = row_block;
    h.n_pixels = n_pixels, h.samples = samples, h.pad[0] = (uint32_t)fast_c;
    h.reserved = per_pixel;
    const std::vector<uint32_t> r(rec, rec + 8 * n_pixels);
    const std::vector<uint32_t> m(mom, mom + (mom ? 8 * n_pixels : 0));
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return -1;
    bool ok = rtaf::write(f, h, r, m);
    ok = (std::fclose(f) == 0) && ok;
    return ok ? 0 : -1;
}

struct ap_file {
    int err;
    char msg[256];
    int kind, fast_c, lo, hi;
    unsigned char header[128];
    long long n_pixels;
    int shard_calls;   // how often read() asked for the shard check
};

// read() with no shard check (shard_refusal 0), or with one that is counted and refuses with
// that code.  rec, mom, sums, moments: room for cap_pixels pixels each.
int ap_read(const char *path, const ap_facts *facts, const char *who, int shard_refusal, long long cap_pixels, ap_file *o,
            unsigned *rec, unsigned *mom, float *sums, float *moments) {
    int calls = 0;
    const auto shard = [&](const rtaf::File &) -> rtp::Refusal {
        ++calls;
        return {shard_refusal, std::string(who) + ": the shard check"};
    };
    const rtaf::File f = shard_refusal ? rtaf::read(path, facts_in(facts), who, shard) : rtaf::read(path, facts_in(facts), who);
    o->err = refusal_out(f.refused, o->msg, sizeof o->msg);
    o->shard_calls = calls;
    if (f.refused) return o->err;
    o->kind = (int)f.kind;
    o->fast_c = f.fast_c();
    o->lo = f.lo;
    o->hi = f.hi;
    o->n_pixels = f.h.n_pixels;
    std::memcpy(o->header, &f.h, 128);
    if (f.h.n_pixels > cap_pixels) return -100;
    std::memcpy(rec, f.rec.data(), f.rec.size() * 4);
    std::memcpy(mom, f.mom.data(), f.mom.size() * 4);
    std::memcpy(sums, f.sums.data(), f.sums.size() * 4);
    std::memcpy(moments, f.moments.data(), f.moments.size() * 4);
    return RT_OK;
}

}  // extern "C"
