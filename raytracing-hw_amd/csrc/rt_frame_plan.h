// rt_frame_plan.h — how a whole frame is split over shards and devices, decided from plain
// values (host only, no HIP).
//
// rt_device.hip's rt_render_frame asks this header before it touches a device:
//   plan_frame          which device renders shard r and which device is the root, which
//                       shards share a device (and therefore its two shard buffers), which rows
//                       shard r owns and where they land in the root's staging buffer, the byte
//                       layout of the root buffer, the size of every device's shard buffers
//                       (and which arguments are refused);
//   merge_frame_stats   how the shards' rt_stats fold into the frame's.
// The visible device count is an input, so the arithmetic of a frame over several devices runs
// without any (tests/test_frame_plan.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_hw.h"
#include "rt_launch_plan.h"

namespace rtp {

constexpr int kMaxDevices = 64;   // device ids a scene keeps a copy for (rt_scene.h kRtMaxDevices)

struct FrameIn {
    int width = 0, height = 0;         // the scene's
    int n_shards = 0;                  // <= 0: one shard per visible device
    const int32_t *devices = nullptr;  // [n_shards] the device of shard r; null: shard r on device r
    int row_block = 0;                 // normalised (> 0)
    int spp = 0;                       // resolved against the scene's samples
    int visible_devices = 0;           // hipGetDeviceCount
    bool want_sums = false;            // the float frame is asked for (out_sum)
};

// A device's two shard buffers (both of buf_bytes): [float sums | 8-bit rows] of its largest
// shard.  The float part is there whether or not the frame's sums are asked for: the shard is
// rendered into it.
struct FrameDevice {
    int64_t max_rows = 0;
    size_t sum_bytes = 0;   // max_rows * row_f, 256-B aligned: the 8-bit rows' offset
    size_t buf_bytes = 0;   // sum_bytes + max_rows * row_u8
};

struct FramePlan {
    Refusal refused;
    int width = 0, height = 0, row_block = 0, spp = 0;   // the inputs every step needs again
    bool want_sums = false;
    int n = 0;                    // shards
    std::vector<int> dev_of;      // [n] device of shard r
    std::vector<int> uniq;        // the distinct devices in first-appearance order; uniq[0] is the root
    std::vector<int> dev_index;   // [n] index of shard r's device in uniq
    // The row partition: shard r owns the rows with (row / row_block) % n == r, rows[r] of them.
    // Staging on the root keeps the shards one after another, shard r's rows from staging row
    // base[r] (n + 1 entries, base[n] = height); frame_row_of[staging row] is its frame row.
    std::vector<int64_t> rows, base;
    std::vector<int32_t> frame_row_of;
    size_t row_u8 = 0, row_f = 0;   // bytes per row: 8-bit RGB, float RGB
    // The root buffer: [stage u8 | frame u8 | stage f32 | frame f32 | row map], each part 256-B
    // aligned; the two f32 parts are empty unless the sums are asked for.
    size_t o_stage_u8 = 0, o_frame_u8 = 0, o_stage_f = 0, o_frame_f = 0, o_row_map = 0, root_bytes = 0;
    std::vector<FrameDevice> dev;   // [uniq.size()]
    int root() const { return uniq[0]; }
};

// The one refusal that needs no device count (rt_render_frame gives it before it asks for one):
// a devices array needs its length, one entry per shard, so n_shards must be given.
inline Refusal frame_check_devices(int n_shards, const int32_t *devices) {
    if (devices && n_shards <= 0)
        return {RT_ERR_ARG, "rt_render_frame: devices given without n_shards (one device per shard)"};
    return {};
}

inline int frame_shards(const FrameIn &in) { return in.n_shards > 0 ? in.n_shards : in.visible_devices; }

// The refusals that do not depend on the scene's size.
inline Refusal frame_check(const FrameIn &in) {
    if (const Refusal r = frame_check_devices(in.n_shards, in.devices)) return r;
    const int n = frame_shards(in);
    if (n < 1 || n > (1 << 16)) return {RT_ERR_ARG, "rt_render_frame: bad shard count " + std::to_string(n)};
    for (int r = 0; r < n; ++r) {
        const int d = in.devices ? in.devices[r] : r;
        if (d < 0 || d >= in.visible_devices || d >= kMaxDevices)
            return {RT_ERR_DEVICE, "rt_render_frame: shard " + std::to_string(r) + " on device " + std::to_string(d) + ", " +
                                       std::to_string(in.visible_devices) + " visible"};
    }
    if (in.spp < 1) return {RT_ERR_ARG, "rt_render_frame: samples per pixel must be >= 1"};
    return {};
}

inline FramePlan plan_frame(const FrameIn &in) {
    FramePlan f;
    if ((f.refused = frame_check(in))) return f;
    const int n = f.n = frame_shards(in), H = in.height, rb = in.row_block;
    if (H <= 0 || rb <= 0) {
        f.refused = {RT_ERR_ARG, "rt_render_frame: bad row partition (height " + std::to_string(H) + ", row_block " +
                                     std::to_string(rb) + ")"};
        return f;
    }
    f.width = in.width;
    f.height = H;
    f.row_block = rb;
    f.spp = in.spp;
    f.want_sums = in.want_sums;
    f.dev_of.resize(n);
    f.dev_index.resize(n);
    for (int r = 0; r < n; ++r) {
        const int d = f.dev_of[r] = in.devices ? in.devices[r] : r;
        size_t ui = 0;
        while (ui < f.uniq.size() && f.uniq[ui] != d) ++ui;
        if (ui == f.uniq.size()) f.uniq.push_back(d);
        f.dev_index[r] = (int)ui;
    }
    // one pass over the rows counts every shard's, one more places them from base[] on
    f.rows.assign(n, 0);
    f.base.assign(n + 1, 0);
    f.frame_row_of.resize(H);
    for (int row = 0; row < H; ++row) ++f.rows[(row / rb) % n];
    for (int r = 0; r < n; ++r) f.base[r + 1] = f.base[r] + f.rows[r];
    std::vector<int64_t> at(f.base.begin(), f.base.end() - 1);
    for (int row = 0; row < H; ++row) f.frame_row_of[at[(row / rb) % n]++] = row;

    f.row_u8 = (size_t)in.width * 3;
    f.row_f = f.row_u8 * sizeof(float);
    const size_t b_u8 = align_up((size_t)H * f.row_u8), b_f = in.want_sums ? align_up((size_t)H * f.row_f) : 0;
    f.o_stage_u8 = 0;
    f.o_frame_u8 = f.o_stage_u8 + b_u8;
    f.o_stage_f = f.o_frame_u8 + b_u8;
    f.o_frame_f = f.o_stage_f + b_f;
    f.o_row_map = f.o_frame_f + b_f;
    f.root_bytes = f.o_row_map + align_up((size_t)H * sizeof(int32_t));

    f.dev.resize(f.uniq.size());
    for (int r = 0; r < n; ++r) {
        FrameDevice &d = f.dev[f.dev_index[r]];
        if (f.rows[r] > d.max_rows) d.max_rows = f.rows[r];
    }
    for (FrameDevice &d : f.dev) {
        d.sum_bytes = align_up((size_t)d.max_rows * f.row_f);
        d.buf_bytes = d.sum_bytes + (size_t)d.max_rows * f.row_u8;
    }
    return f;
}

// The frame's stats from its shards' (shard_stats[f.n]): counters summed, schedule bits united;
// a device's shards run in turn, so render_ms and order_ms are those of the slowest device (its
// shards summed).  Every field a frame does not report is zero.
inline void merge_frame_stats(const FramePlan &f, const rt_stats *shard_stats, double gather_ms, rt_stats *out) {
    *out = rt_stats{};
    std::vector<double> dev_ms(f.uniq.size(), 0.0), dev_order(f.uniq.size(), 0.0);
    for (int r = 0; r < f.n; ++r) {
        const rt_stats &x = shard_stats[r];
        out->pixels += x.pixels;
        out->samples += x.samples;
        out->rays += x.rays;
        out->aabb_tests += x.aabb_tests;
        out->tri_tests += x.tri_tests;
        out->light_queries += x.light_queries;
        out->light_aabb_tests += x.light_aabb_tests;
        out->light_tri_tests += x.light_tri_tests;
        out->shading_hits += x.shading_hits;
        out->extend_rays += x.extend_rays;
        out->schedule |= x.schedule;
        dev_ms[f.dev_index[r]] += x.render_ms;
        dev_order[f.dev_index[r]] += x.order_ms;
    }
    out->render_ms = *std::max_element(dev_ms.begin(), dev_ms.end());
    out->order_ms = *std::max_element(dev_order.begin(), dev_order.end());
    out->gather_ms = gather_ms;
    out->devices = (uint64_t)f.uniq.size();
}

}  // namespace rtp
