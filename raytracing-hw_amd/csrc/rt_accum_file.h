// rt_accum_file.h — an accumulator's checkpoint file (rt_accum_save / rt_accum_load), host only.
//
// The file: AccumHeader, then n_pixels records of 8 words in the chain buffer's layout, then (a
// moments file) n_pixels moment records of 8 words, all verbatim (rt_records.h: parity, fast and
// moment records).  Little-endian, as the devices and their hosts are.  The magic
// (rt_accum_plan.h kKinds, version 1 each) says which kind it holds; a fast kind's chunk size is
// in pad[0].
// write() is the writer; read() checks a file whole against the scene and rebuilds what the fold
// kernels report for its records, before any device call (tests/test_accum_plan.py).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "rt_accum_plan.h"
#include "rt_records.h"

namespace rtaf {

using rtap::Kind;
using rtp::Refusal;

struct AccumHeader {
    char magic[8];
    uint32_t version;
    int32_t width, height, ray_depth;
    int32_t rank, world, row_block;
    uint32_t n_tris, n_nodes, n_lights;
    int64_t n_pixels;
    int32_t samples, reserved;   // reserved 1: per-pixel counts, `samples` is the largest
    float cam[14];               // cam_pos, cam_axes, tan_half_fov
    uint32_t pad[2];             // pad[0]: a fast kind's chunk size
};
static_assert(sizeof(AccumHeader) == 128, "rt_accum file header is 128 bytes");

// What the header records of the scene it was made for.
struct SceneFacts {
    int32_t width, height, ray_depth;
    uint32_t n_tris, n_nodes, n_lights;
    float cam[14];
};

// A kind's header for the scene; the shard, the counts and the chunk size are the caller's.
inline AccumHeader header_of(const SceneFacts &s, Kind kind) {
    AccumHeader h;
    std::memset(&h, 0, sizeof h);
    std::memcpy(h.magic, rtap::info(kind).magic, 8);
    h.version = rtap::info(kind).version;
    h.width = s.width, h.height = s.height, h.ray_depth = s.ray_depth;
    h.n_tris = s.n_tris, h.n_nodes = s.n_nodes, h.n_lights = s.n_lights;
    std::memcpy(h.cam, s.cam, sizeof h.cam);
    return h;
}

// The header, the records and (a moments file) the moment records; false on a short write.
inline bool write(std::FILE *f, const AccumHeader &h, const std::vector<uint32_t> &rec, const std::vector<uint32_t> &mom) {
    bool ok = std::fwrite(&h, sizeof h, 1, f) == 1;
    ok = ok && (rec.empty() || std::fwrite(rec.data(), 4, rec.size(), f) == rec.size());
    ok = ok && (mom.empty() || std::fwrite(mom.data(), 4, mom.size(), f) == mom.size());
    return ok;
}

// A file as read() found it.
struct File {
    Refusal refused;
    Kind kind = Kind::Parity;
    AccumHeader h{};
    std::vector<uint32_t> rec, mom;     // n_pixels x 8 words each (mom: a moments file)
    int lo = 0, hi = 0;                 // the smallest and largest next sample of the records
    std::vector<float> sums, moments;   // n_pixels x 3: the records' reported sums (and moments), as the fold kernels write them
    int fast_c() const { return rtap::info(kind).fast ? (int)h.pad[0] : 0; }
};

// Reads `path` and checks it whole; `who` opens every message.  In this order: the file and its
// header, the header against the scene, the header's shard fields, `shard` (if given: the
// caller's check that the shard of this scene has h.n_pixels pixels, called once kind and h are
// set), then every record.
inline File read(const char *path, const SceneFacts &scene, const std::string &who,
                 const std::function<Refusal(const File &)> &shard = nullptr) {
    File f;
    AccumHeader &h = f.h;
    std::FILE *fp = std::fopen(path, "rb");
    if (!fp) {
        f.refused = {RT_ERR_IO, who + ": cannot open"};
        return f;
    }
    const auto is = [&](Kind k) { return std::memcmp(h.magic, rtap::info(k).magic, 8) == 0; };
    if (std::fread(&h, sizeof h, 1, fp) != 1) f.refused = {RT_ERR_FORMAT, who + ": shorter than its header"};
    else if (!is(f.kind = Kind::Moments) && !is(f.kind = Kind::Fast) && !is(f.kind = Kind::Parity))
        f.refused = {RT_ERR_FORMAT, who + ": not an accumulator file (magic)"};
    else if (h.version != rtap::info(f.kind).version)
        f.refused = {RT_ERR_FORMAT, who + ": version " + std::to_string(h.version) + ", this library reads " +
                                        std::to_string(rtap::info(f.kind).version)};
    else if (rtap::info(f.kind).fast && (h.pad[0] < 1u || h.pad[0] > (uint32_t)INT32_MAX))
        f.refused = {RT_ERR_FORMAT, who + ": bad chunk size " + std::to_string(h.pad[0])};
    else if (h.n_pixels < 0 || h.n_pixels > INT32_MAX || h.samples < 0 || h.samples >= (1 << 20))
        f.refused = {RT_ERR_FORMAT, who + ": bad pixel or sample count"};
    else if (h.reserved != 0 && h.reserved != 1)
        f.refused = {RT_ERR_FORMAT, who + ": bad count form " + std::to_string(h.reserved) + " (0 uniform, 1 per pixel)"};
    else {
        std::fseek(fp, 0, SEEK_END);
        const long long len = (long long)std::ftell(fp);
        const long long want_len = (long long)sizeof h + h.n_pixels * rtap::info(f.kind).record_bytes;
        if (len != want_len)
            f.refused = {RT_ERR_FORMAT, who + ": " + std::to_string(len) + " bytes, expected " + std::to_string(want_len)};
        else {
            std::fseek(fp, (long)sizeof h, SEEK_SET);
            f.rec.resize((size_t)h.n_pixels * 8);
            if (f.kind == Kind::Moments) f.mom.resize((size_t)h.n_pixels * 8);
            if ((!f.rec.empty() && std::fread(f.rec.data(), 4, f.rec.size(), fp) != f.rec.size()) ||
                (!f.mom.empty() && std::fread(f.mom.data(), 4, f.mom.size(), fp) != f.mom.size()))
                f.refused = {RT_ERR_IO, who + ": read failed"};
        }
    }
    std::fclose(fp);
    if (f.refused) return f;
    if (h.width != scene.width || h.height != scene.height || h.ray_depth != scene.ray_depth)
        f.refused = {RT_ERR_ARG, who + ": made for a " + std::to_string(h.width) + " x " + std::to_string(h.height) +
                                     " frame at ray depth " + std::to_string(h.ray_depth) + ", the scene is " +
                                     std::to_string(scene.width) + " x " + std::to_string(scene.height) + " at " +
                                     std::to_string(scene.ray_depth)};
    else if (h.n_tris != scene.n_tris || h.n_nodes != scene.n_nodes || h.n_lights != scene.n_lights ||
             std::memcmp(h.cam, scene.cam, sizeof h.cam) != 0)
        f.refused = {RT_ERR_ARG, who + ": made for another scene or camera"};
    else if (h.world < 1 || h.rank < 0 || h.rank >= h.world || h.row_block < 1)
        f.refused = {RT_ERR_ARG, who + ": bad shard (rank " + std::to_string(h.rank) + ", world " + std::to_string(h.world) +
                                     ", row_block " + std::to_string(h.row_block) + ")"};
    else if (shard)
        f.refused = shard(f);
    if (f.refused) return f;
    // (per-pixel counts, reserved = 1: any next sample up to the header's; else all equal to it)
    const bool fast = rtap::info(f.kind).fast, moments = f.kind == Kind::Moments;
    const int c = f.fast_c();
    uint32_t lo = (uint32_t)h.samples, hi = h.reserved && h.n_pixels ? 0u : (uint32_t)h.samples;
    f.sums.resize((size_t)h.n_pixels * 3);
    if (moments) f.moments.resize((size_t)h.n_pixels * 3);
    for (long long k = 0; k < h.n_pixels; ++k) {
        const uint32_t *rec = &f.rec[rtrec::kWords * k], nx = rec[rtrec::kNext];
        const uint32_t *mom = moments ? &f.mom[rtrec::kWords * k] : nullptr;
        if (rec[rtrec::kPixel] != (uint32_t)k || (h.reserved ? nx > (uint32_t)h.samples : nx != (uint32_t)h.samples))
            f.refused = {RT_ERR_FORMAT, who + ": record " + std::to_string(k) + " does not belong to this file"};
        else if (fast && !rtrec::open_words_fit(nx, c, rec))
            f.refused = {RT_ERR_FORMAT, who + ": record " + std::to_string(k) + " holds an open partial at a chunk boundary"};
        else if (moments && !rtrec::record_words_fit(nx, c, mom))
            f.refused = {RT_ERR_FORMAT, who + ": moment record " + std::to_string(k) +
                                            " holds an open partial or pad words at a chunk boundary"};
        if (f.refused) return f;
        lo = std::min(lo, nx);
        hi = std::max(hi, nx);
        // the reported values (rt_fast_units.h reported; a parity record's sum as it is)
        if (fast) rtfu::reported(rtrec::fast_unpack(rec).r, c, &f.sums[3 * k]);
        else std::memcpy(&f.sums[3 * k], rtrec::parity_unpack(rec).sum, 12);
        if (moments) {
            rtfu::Rec m;
            m.next = (int)nx;
            rtrec::moment_unpack(mom, m);
            rtfu::reported(m, c, &f.moments[3 * k]);
        }
    }
    f.lo = (int)lo;
    f.hi = (int)hi;
    return f;
}

}  // namespace rtaf
