// rt_main.cpp — drop-in CLI for the reference's `solution` (src/main.cpp:22-60, run.sh:2):
//   rt_solution input.gltf width height samples [output.ppm]
// Same positional arguments, same default output name, same terminate-with-message
// behaviour on errors (std::runtime_error), rendering through librt_hw_amd on every GPU of
// the node (rt_render_frame: one row-block shard per device, finished on its GPU and gathered
// device-to-device onto GPU 0; RT_GPUS=n uses devices 0..n-1).
// Progressive rendering (two more environment variables; unset, the run is the one above):
//   RT_PASS_SPP=k       render in passes of k samples (one accumulator per device, rt_accum_*);
//                       after every pass the frame so far is written to the output file and a
//                       line "Progress: done / total samples" is printed.  The final file is
//                       byte-identical to the one-shot run's.
//   RT_CHECKPOINT=pfx   after every pass shard r of n is saved to pfx.<r>of<n>; if those files
//                       exist at the start the run resumes from them (and fails with the
//                       library's message when they do not fit the scene).
// Adaptive rendering (per-pixel sample counts, rt_accum_select / rt_accum_add_selected):
//   RT_ADAPT=t          the samples argument is the maximum per pixel and RT_PASS_SPP=k the step
//                       (default 16).  Every shard renders k samples, marks, renders k more; then
//                       rounds of: select the pixels below min(maximum, largest count + k) whose
//                       error estimate exceeds t (t <= 0: all of them), stop when no shard
//                       selects any or the maximum is reached, else mark and render the selected.
//                       Prints "Progress: refined <pixels> pixels to <target> samples" per round
//                       and writes the frame with every pixel divided by its own count.
//   RT_COUNTS_OUT=path  (with RT_ADAPT) the sample-count map as a binary 16-bit PGM: "P5", maxval
//                       65535, big-endian, counts clamped to it.
// Fast mode (RT_FLAG_FAST: per-sample Philox streams, not the reference's RNG convention):
//   RT_FAST=c           chunks of c samples (c >= 1).  Alone: the one-shot frame in fast mode with
//                       fast_chunk = c.  With RT_PASS_SPP and / or RT_ADAPT: the passes run on fast
//                       accumulators (rt_accum_create_fast) with chunk size c; a checkpoint resumes
//                       only into the kind and chunk size that wrote it.
// Measured variance (per-sample second moments; unset, every byte written is the one above):
//   RT_MOMENTS=1        needs RT_FAST and a pass mode (RT_PASS_SPP or RT_ADAPT): the passes run on
//                       moments accumulators (rt_accum_create_fast_moments).  With RT_DENOISE_GUIDED
//                       every frame written is filtered with the measured variance
//                       (rt_accum_frame_u8_guided_measured; several GPUs: each shard's
//                       rt_accum_variance gathered like its sums).  With RT_ADAPT the rounds select by
//                       the relative standard error (rt_accum_select_variance) and set no mark.  A
//                       checkpoint of such a run resumes only into such a run with the same chunk.
//   RT_VARIANCE_OUT=path  (with RT_MOMENTS) the measured variance of the final frame as a
//                       one-channel PFM ("Pf", scale -1: little-endian floats, bottom row first).
// Denoising and feature images (rt_denoise*, rt_gbuffer; unset, the bytes are the ones above):
//   RT_DENOISE=k        every frame the run writes (the one-shot frame, each pass's preview, the
//                       adaptive result) passes through the edge-avoiding a-trous filter with k
//                       iterations (1..6; the other parameters at their defaults) before the 8-bit
//                       finish.  One GPU with passes: on the accumulator (rt_accum_frame_u8_denoised).
//                       Otherwise the float frame (and the counts) assembled from the shards and the
//                       frame's G-buffer, rendered once on device 0, are filtered on device 0
//                       (rt_denoise_frame_u8).  k = 0 is refused here, although the library takes
//                       iterations = 0 (the unfiltered mean): it would be the run with RT_DENOISE unset.
//   RT_DENOISE_GUIDED=k the same frames through the filter's variance-guided mode with its firefly
//                       clamp instead (rt_accum_frame_u8_guided, rt_denoise_guided_frame_u8; k
//                       iterations, 1..6, the other parameters at their defaults).  Setting both
//                       variables is an error, reported before anything is rendered.
//   RT_AOV_OUT=pfx      the first-hit features of the frame: pfx.normal.ppm (N * 0.5 + 0.5),
//                       pfx.albedo.ppm (the linear base colour) and pfx.depth.pgm (binary 16-bit PGM,
//                       big-endian, hit distance / the frame's largest; a miss is 0).
// A moving camera (rt_scene_set_camera, rt_history_*; unset, every byte written is the one above):
//   RT_CAMERAS=file     one camera per line, 14 floats: position, right, up, forward, tan_half_fov x
//                       and y (empty lines and lines that start with # are skipped).  Every line
//                       renders one one-shot frame at the given samples from that camera, written to
//                       the output name with the line's index before the extension (out.0000.ppm,
//                       out.0001.ppm, ...); each raw frame is the reference's frame for that camera.
//                       Excludes RT_PASS_SPP, RT_ADAPT and RT_CHECKPOINT; a malformed line is an
//                       error, reported before anything is rendered.
//   RT_TEMPORAL=alpha   (needs RT_CAMERAS) every frame's sums pass through a reprojected temporal
//                       history on device 0 before the finish (alpha 0: the default 0.2); RT_DENOISE
//                       or RT_DENOISE_GUIDED then filter the integrated mean at spp 1 with the
//                       history's G-buffer.  A still camera gains nothing this way (parity frames of
//                       one view are identical): RT_PASS_SPP is the tool for a still view.
// Moving objects (rt_scene_update_tris; unset, every byte written is the one above):
//   RT_MOVES=file       one frame per line, groups of four numbers `mesh dx dy dz`: the mesh's triangles
//                       are drawn with v0 + (dx, dy, dz), an offset from the loaded position (a mesh a
//                       line does not name is at its loaded position; empty lines and lines that start
//                       with # are skipped).  Frames are written as RT_CAMERAS writes them
//                       (out.0000.ppm, ...), and the exclusions are RT_CAMERAS'.  With RT_CAMERAS both
//                       files must hold as many frames.  A malformed line, an unknown mesh and an
//                       emissive mesh (lights do not move) are errors that name the line, reported
//                       before anything is rendered.
//   RT_MOTION=1         (needs RT_MOVES and RT_TEMPORAL; RT_CAMERAS is then optional) the history opts in to
//                       per-pixel motion records (rt_history_enable_motion): a moved object keeps its
//                       history instead of restarting or smearing it.  Without it every message and
//                       refusal is as above.
//   RT_MOVE_LIGHTS=1    (with RT_MOVES) the scene opts in to movable lights (rt_scene_enable_light_updates):
//                       a line may name an emissive mesh, whose light records and light BVH boxes then
//                       follow its triangles, and the covering ranges are not cut at emissive triangles.
// Posed objects (rt_scene_pose_meshes; unset, every byte written is the one above):
//   RT_POSES=file       one frame per line, groups of eleven numbers `mesh tx ty tz qx qy qz qw sx sy sz`:
//                       the mesh's whole node matrix is matrix4::TRS of them (rt_trs_matrix), not an offset
//                       from the loaded one, and its triangles are recomputed on the device from the
//                       object-space vertices; a mesh a line does not name keeps its last pose.  Frames,
//                       exclusions and errors are RT_MOVES'; RT_CAMERAS, RT_TEMPORAL, RT_MOTION,
//                       RT_MOVE_LIGHTS and the denoisers combine with it as with RT_MOVES.  Setting both
//                       RT_POSES and RT_MOVES is an error.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iomanip>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rt_hw.h"

static void check(int rc) {
    if (rc != RT_OK) throw std::runtime_error(rt_last_error());
}

// The whole frame's first-hit records (RT_GBUFFER_WORDS floats per pixel), rendered on device 0.
static std::vector<float> frame_gbuffer(rt_scene *scene, int width, int height) {
    std::vector<float> g((size_t)width * height * RT_GBUFFER_WORDS);
    rt_params p{};
    p.world = 1;
    p.row_block = 8;
    check(rt_gbuffer(scene, &p, g.data()));
    return g;
}

// RT_DENOISE / RT_DENOISE_GUIDED: the filter's parameters (k iterations, the rest at their
// defaults), or none.
struct Denoise {
    bool on = false, guided = false;
    bool measured = false;   // (RT_MOMENTS with the guided mode: the filter's variance input is the measured one)
    rt_denoise_params params{-1, 0.f, 0.f, 0};
    rt_denoise_guided_params guided_params{-1, 0.f, 0.f, 0, 0.f};
    std::vector<float> gbuffer;   // the frame's, rendered at the first frame that needs it

    int accum_frame(rt_accum *acc, uint8_t *rgb) const {
        if (guided && measured) return rt_accum_frame_u8_guided_measured(acc, &guided_params, rgb);
        return guided ? rt_accum_frame_u8_guided(acc, &guided_params, rgb) : rt_accum_frame_u8_denoised(acc, &params, rgb);
    }
    // (variance: the frame's measured variance, or NULL for the filter's own estimate)
    int frame(const float *sums, const int32_t *counts, int spp, int width, int height, uint8_t *rgb,
              const float *variance = nullptr) const {
        return guided ? rt_denoise_guided_frame_u8(sums, counts, spp, width, height, gbuffer.data(), variance, &guided_params, 0, rgb)
                      : rt_denoise_frame_u8(sums, counts, spp, width, height, gbuffer.data(), &params, 0, rgb);
    }
};

static void write_file(const std::string &path, const char *header, const std::vector<uint8_t> &bytes) {
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("RT_AOV_OUT: cannot write " + path);
    std::fputs(header, f);
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (std::fclose(f) != 0 || !ok) throw std::runtime_error("RT_AOV_OUT: short write to " + path);
}

// RT_AOV_OUT: the normal, albedo and depth images of the frame's G-buffer.
static void write_aovs(const std::string &prefix, const std::vector<float> &g, int width, int height) {
    const size_t n = (size_t)width * height;
    auto byte_of = [](float v) { return (uint8_t)(std::min(std::max(v, 0.f), 1.f) * 255.f + 0.5f); };
    std::vector<uint8_t> normal(n * 3), albedo(n * 3), depth(n * 2);
    float far = 0.f;
    for (size_t p = 0; p < n; ++p) far = std::max(far, g[p * RT_GBUFFER_WORDS + 3]);
    for (size_t p = 0; p < n; ++p) {
        const float *r = &g[p * RT_GBUFFER_WORDS];
        for (int c = 0; c < 3; ++c) {
            normal[3 * p + c] = byte_of(r[c] * 0.5f + 0.5f);
            albedo[3 * p + c] = byte_of(r[4 + c]);
        }
        const int d = far > 0.f ? (int)(std::min(std::max(r[3] / far, 0.f), 1.f) * 65535.f + 0.5f) : 0;
        depth[2 * p] = (uint8_t)(d >> 8);
        depth[2 * p + 1] = (uint8_t)(d & 255);
    }
    const std::string size = std::to_string(width) + " " + std::to_string(height);
    write_file(prefix + ".normal.ppm", ("P6\n" + size + "\n255\n").c_str(), normal);
    write_file(prefix + ".albedo.ppm", ("P6\n" + size + "\n255\n").c_str(), albedo);
    write_file(prefix + ".depth.pgm", ("P5\n" + size + "\n65535\n").c_str(), depth);
}

// The frame in passes: device d renders shard (rank d, world n) through its own accumulator.
// `adapt` (RT_ADAPT): its threshold; the passes are then those of adaptive rendering (above).
// `moments` (RT_MOMENTS): on moments accumulators; `variance_out` (RT_VARIANCE_OUT): the PFM's path.
static void render_passes(rt_scene *scene, int width, int height, int samples, int n_gpus, int pass_spp,
                          const char *ckpt, const std::string &output, const float *adapt = nullptr,
                          const char *counts_out = nullptr, int fast_chunk = 0, Denoise *dn = nullptr,
                          bool moments = false, const char *variance_out = nullptr) {
    const int n = n_gpus > 0 ? n_gpus : rt_device_count();
    if (n < 1) throw std::runtime_error("no HIP device");
    if (samples < 1) throw std::runtime_error("samples per pixel must be >= 1");
    struct Accums {   // (freed on every way out)
        std::vector<rt_accum *> v;
        ~Accums() { for (rt_accum *a : v) rt_accum_free(a); }
    } held;
    held.v.assign((size_t)n, nullptr);
    std::vector<rt_accum *> &acc = held.v;
    auto file_of = [&](int r) { return std::string(ckpt) + "." + std::to_string(r) + "of" + std::to_string(n); };
    bool resume = ckpt != nullptr;
    for (int r = 0; resume && r < n; ++r) {
        std::FILE *f = std::fopen(file_of(r).c_str(), "rb");
        if (f) std::fclose(f);
        else resume = false;
    }
    for (int r = 0; r < n; ++r) {
        if (resume) {
            check(rt_accum_load(scene, r, file_of(r).c_str(), &acc[(size_t)r]));
            const int have = rt_accum_fast_chunk(acc[(size_t)r]);
            const bool have_moments = rt_accum_has_moments(acc[(size_t)r]) != 0;
            if (have != fast_chunk || have_moments != moments)
                throw std::runtime_error("checkpoint " + file_of(r) + " holds " +
                                         (have ? "a fast accumulator with chunks of " + std::to_string(have) : std::string("a parity accumulator")) +
                                         (have_moments ? " and moments" : "") + ", the run asks for " +
                                         (fast_chunk ? "RT_FAST=" + std::to_string(fast_chunk) : std::string("parity passes (RT_FAST unset)")) +
                                         (moments ? " with RT_MOMENTS" : have_moments ? " without RT_MOMENTS" : ""));
        } else {
            check(rt_scene_upload(scene, r));
            rt_params p{};
            p.rank = r;
            p.world = n;
            p.row_block = 8;
            p.device = r;
            p.fast_chunk = fast_chunk;
            check(moments      ? rt_accum_create_fast_moments(scene, &p, &acc[(size_t)r])
                  : fast_chunk ? rt_accum_create_fast(scene, &p, &acc[(size_t)r])
                               : rt_accum_create(scene, &p, &acc[(size_t)r]));
        }
    }
    int done = rt_accum_samples(acc[0]);
    for (int r = 1; r < n; ++r) {   // (adaptive shards may differ: `done` is then the largest count)
        const int dr = rt_accum_samples(acc[(size_t)r]);
        if (dr != done && !adapt) throw std::runtime_error("checkpoint shards are at different sample counts");
        done = std::max(done, dr);
    }
    if (done > samples)
        throw std::runtime_error("checkpoint holds " + std::to_string(done) + " samples, more than the " +
                                 std::to_string(samples) + " asked for");
    if (resume) std::cout << "Resumed from " << ckpt << " at " << done << " samples." << std::endl;
    std::vector<uint8_t> rgb((size_t)width * height * 3), part;
    std::vector<int32_t> rows((size_t)height);
    std::vector<float> sums, spart;
    std::vector<int32_t> counts, cshard;
    std::vector<float> variance, vpart;
    auto gather_variance = [&]() {   // every shard's measured variance in frame order
        variance.resize((size_t)width * height);
        for (int r = 0; r < n; ++r) {
            const int64_t k = rt_shard_rows(height, r, n, 8, rows.data());
            if (k < 0) check((int)k);
            vpart.resize((size_t)k * width);
            check(rt_accum_variance(acc[(size_t)r], vpart.data()));
            for (int64_t i = 0; i < k; ++i)
                std::copy(vpart.begin() + i * width, vpart.begin() + (i + 1) * width, variance.begin() + (size_t)rows[(size_t)i] * width);
        }
    };
    auto write_frame = [&]() {
        if (dn && dn->on && n == 1) {   // the accumulator owns the whole frame: filtered where it lives
            check(dn->accum_frame(acc[0], rgb.data()));
            check(rt_write_ppm(output.c_str(), rgb.data(), width, height));
            return;
        }
        if (dn && dn->on) {   // the shards' sums and counts in frame order, filtered on device 0
            sums.resize((size_t)width * height * 3);
            counts.resize((size_t)width * height);
            for (int r = 0; r < n; ++r) {
                const int64_t k = rt_shard_rows(height, r, n, 8, rows.data());
                if (k < 0) check((int)k);
                spart.resize((size_t)k * width * 3);
                cshard.resize((size_t)k * width);
                check(rt_accum_sums(acc[(size_t)r], spart.data()));
                check(rt_accum_counts(acc[(size_t)r], cshard.data()));
                for (int64_t i = 0; i < k; ++i) {
                    std::copy(spart.begin() + i * width * 3, spart.begin() + (i + 1) * width * 3,
                              sums.begin() + (size_t)rows[(size_t)i] * width * 3);
                    std::copy(cshard.begin() + i * width, cshard.begin() + (i + 1) * width,
                              counts.begin() + (size_t)rows[(size_t)i] * width);
                }
            }
            // (after rt_accum_sums has waited for every shard's pass: nothing else runs on device 0)
            if (dn->gbuffer.empty()) dn->gbuffer = frame_gbuffer(scene, width, height);
            if (dn->guided && dn->measured) gather_variance();
            check(dn->frame(sums.data(), counts.data(), 0, width, height, rgb.data(),
                            dn->guided && dn->measured ? variance.data() : nullptr));
            check(rt_write_ppm(output.c_str(), rgb.data(), width, height));
            return;
        }
        for (int r = 0; r < n; ++r) {
            const int64_t k = rt_shard_rows(height, r, n, 8, rows.data());
            if (k < 0) check((int)k);
            part.resize((size_t)k * width * 3);
            check(rt_accum_frame_u8(acc[(size_t)r], part.data()));
            for (int64_t i = 0; i < k; ++i)
                std::copy(part.begin() + i * width * 3, part.begin() + (i + 1) * width * 3,
                          rgb.begin() + (size_t)rows[(size_t)i] * width * 3);
        }
        check(rt_write_ppm(output.c_str(), rgb.data(), width, height));
    };
    auto save_all = [&]() {
        if (ckpt)
            for (int r = 0; r < n; ++r) check(rt_accum_save(acc[(size_t)r], file_of(r).c_str()));
    };
    auto write_variance = [&]() {   // RT_VARIANCE_OUT: one channel, little-endian floats, bottom row first
        if (!variance_out) return;
        gather_variance();
        std::FILE *f = std::fopen(variance_out, "wb");
        if (!f) throw std::runtime_error(std::string("RT_VARIANCE_OUT: cannot write ") + variance_out);
        std::fprintf(f, "Pf\n%d %d\n-1.0\n", width, height);
        bool ok = true;
        for (int y = height - 1; y >= 0; --y)
            ok = ok && std::fwrite(&variance[(size_t)y * width], sizeof(float), (size_t)width, f) == (size_t)width;
        if (std::fclose(f) != 0 || !ok) throw std::runtime_error(std::string("RT_VARIANCE_OUT: short write to ") + variance_out);
    };
    if (adapt) {
        const int k = pass_spp > 0 ? pass_spp : 16;
        auto add_all = [&](int m) {
            for (int r = 0; r < n; ++r) check(rt_accum_add(acc[(size_t)r], m, nullptr, nullptr));
            done += m;
        };
        if (done == 0) {   // (a resumed run goes on with the rounds below; it has no mark: its first round selects by count alone)
            add_all(std::min(k, samples));
            if (!moments)   // (the variance rule reads no mark)
                for (int r = 0; r < n; ++r) check(rt_accum_mark(acc[(size_t)r], nullptr));
            if (done < samples) add_all(std::min(k, samples - done));
            std::cout << "Progress: " << done << " / " << samples << " samples" << std::endl;
        }
        while (done < samples) {
            rt_select sel{};
            sel.target = std::min(samples, done + k);
            sel.threshold = *adapt;
            int64_t total = 0;
            for (int r = 0; r < n; ++r) {
                int64_t m = 0;
                check(moments ? rt_accum_select_variance(acc[(size_t)r], &sel, nullptr, &m)
                              : rt_accum_select(acc[(size_t)r], &sel, nullptr, &m));
                total += m;
            }
            if (total == 0) break;
            for (int r = 0; r < n; ++r) {
                if (!moments) check(rt_accum_mark(acc[(size_t)r], nullptr));
                check(rt_accum_add_selected(acc[(size_t)r], nullptr, nullptr));
            }
            done = sel.target;
            std::cout << "Progress: refined " << total << " pixels to " << sel.target << " samples" << std::endl;
            save_all();
        }
        write_frame();
        save_all();
        write_variance();
        if (counts_out) {
            std::vector<int32_t> cpart;
            std::vector<uint8_t> pgm((size_t)width * height * 2);
            for (int r = 0; r < n; ++r) {
                const int64_t kr = rt_shard_rows(height, r, n, 8, rows.data());
                if (kr < 0) check((int)kr);
                cpart.resize((size_t)kr * width);
                check(rt_accum_counts(acc[(size_t)r], cpart.data()));
                for (int64_t i = 0; i < kr; ++i)
                    for (int x = 0; x < width; ++x) {
                        const int32_t c = std::min<int32_t>(std::max<int32_t>(cpart[(size_t)i * width + x], 0), 65535);
                        uint8_t *o = &pgm[((size_t)rows[(size_t)i] * width + x) * 2];
                        o[0] = (uint8_t)(c >> 8);
                        o[1] = (uint8_t)(c & 255);
                    }
            }
            std::FILE *f = std::fopen(counts_out, "wb");
            if (!f) throw std::runtime_error(std::string("RT_COUNTS_OUT: cannot write ") + counts_out);
            std::fprintf(f, "P5\n%d %d\n65535\n", width, height);
            const bool ok = std::fwrite(pgm.data(), 1, pgm.size(), f) == pgm.size();
            if (std::fclose(f) != 0 || !ok) throw std::runtime_error(std::string("RT_COUNTS_OUT: short write to ") + counts_out);
        }
        return;
    }
    if (done == samples && done > 0) write_frame();
    while (done < samples) {
        const int k = pass_spp > 0 ? std::min(pass_spp, samples - done) : samples - done;
        for (int r = 0; r < n; ++r) check(rt_accum_add(acc[(size_t)r], k, nullptr, nullptr));   // (asynchronous: the devices overlap)
        done += k;
        write_frame();   // (waits for every device's pass)
        if (ckpt)
            for (int r = 0; r < n; ++r) check(rt_accum_save(acc[(size_t)r], file_of(r).c_str()));
        std::cout << "Progress: " << done << " / " << samples << " samples" << std::endl;
    }
    write_variance();
}

// RT_CAMERAS: the file's cameras, or false and why.
static bool read_cameras(const char *path, std::vector<rt_camera> &cams, std::string &why) {
    std::ifstream f(path);
    if (!f) {
        why = std::string("RT_CAMERAS: cannot read ") + path;
        return false;
    }
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        std::istringstream in(line);
        float w[14];
        int got = 0;
        std::string token;
        while (in >> token) {
            char *end = nullptr;
            const float v = std::strtof(token.c_str(), &end);
            if (end == token.c_str() || *end != '\0' || !std::isfinite(v) || got == 14) {
                got = -1;
                break;
            }
            w[got++] = v;
        }
        if (got != 14 || !(w[12] > 0.f) || !(w[13] > 0.f)) {
            why = std::string("RT_CAMERAS: ") + path + " line " + std::to_string(no) +
                  ": expected 14 finite floats (position, right, up, forward, tan_half_fov x and y > 0)";
            return false;
        }
        rt_camera c;
        std::copy(w, w + 3, c.pos);
        std::copy(w + 3, w + 12, c.axes);
        std::copy(w + 12, w + 14, c.tan_half_fov);
        cams.push_back(c);
    }
    if (cams.empty()) {
        why = std::string("RT_CAMERAS: no camera in ") + path;
        return false;
    }
    return true;
}

// RT_MOVES: the file's frames (a frame: the meshes it names and their offsets), or false and why.
struct Move {
    uint32_t mesh;
    float d[3];
};
static bool read_moves(const char *path, const rt_scene_view &view, bool move_lights, std::vector<std::vector<Move>> &frames,
                       std::string &why) {
    std::ifstream f(path);
    if (!f) {
        why = std::string("RT_MOVES: cannot read ") + path;
        return false;
    }
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        const std::string where = std::string("RT_MOVES: ") + path + " line " + std::to_string(no) + ": ";
        std::istringstream in(line);
        std::vector<std::string> tok;
        for (std::string t; in >> t;) tok.push_back(t);
        if (tok.size() % 4 != 0) {
            why = where + "expected groups of four numbers: mesh dx dy dz";
            return false;
        }
        std::vector<Move> frame;
        for (size_t k = 0; k < tok.size(); k += 4) {
            char *end = nullptr;
            const long long m = std::strtoll(tok[k].c_str(), &end, 10);
            if (end == tok[k].c_str() || *end != '\0') {
                why = where + "expected groups of four numbers: mesh dx dy dz";
                return false;
            }
            if (m < 0 || m >= (long long)view.n_meshes) {
                why = where + "unknown mesh " + tok[k] + " (the scene has " + std::to_string(view.n_meshes) + ")";
                return false;
            }
            const float *e = view.mesh_f + 12 * (size_t)m + 3;
            if (!move_lights && (e[0] != 0.f || e[1] != 0.f || e[2] != 0.f)) {
                why = where + "mesh " + tok[k] + " is emissive; moving lights are not supported";
                return false;
            }
            Move mv{(uint32_t)m, {0.f, 0.f, 0.f}};
            for (int c = 0; c < 3; ++c) {
                const std::string &t = tok[k + 1 + (size_t)c];
                mv.d[c] = std::strtof(t.c_str(), &end);
                if (end == t.c_str() || *end != '\0' || !std::isfinite(mv.d[c])) {
                    why = where + "expected groups of four numbers: mesh dx dy dz (finite offsets)";
                    return false;
                }
            }
            frame.push_back(mv);
        }
        frames.push_back(frame);
    }
    if (frames.empty()) {
        why = std::string("RT_MOVES: no frame in ") + path;
        return false;
    }
    return true;
}

// RT_POSES: the file's frames (a frame: the meshes it names and their node matrices), or false and why.
struct Pose {
    uint32_t mesh;
    double m[16];
};
static bool read_poses(const char *path, const rt_scene_view &view, bool move_lights, std::vector<std::vector<Pose>> &frames,
                       std::string &why) {
    std::ifstream f(path);
    if (!f) {
        why = std::string("RT_POSES: cannot read ") + path;
        return false;
    }
    const char *shape = "expected groups of eleven numbers: mesh tx ty tz qx qy qz qw sx sy sz";
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        const size_t first = line.find_first_not_of(" \t\r");
        if (first == std::string::npos || line[first] == '#') continue;
        const std::string where = std::string("RT_POSES: ") + path + " line " + std::to_string(no) + ": ";
        std::istringstream in(line);
        std::vector<std::string> tok;
        for (std::string t; in >> t;) tok.push_back(t);
        if (tok.size() % 11 != 0) {
            why = where + shape;
            return false;
        }
        std::vector<Pose> frame;
        for (size_t k = 0; k < tok.size(); k += 11) {
            char *end = nullptr;
            const long long m = std::strtoll(tok[k].c_str(), &end, 10);
            if (end == tok[k].c_str() || *end != '\0') {
                why = where + shape;
                return false;
            }
            if (m < 0 || m >= (long long)view.n_meshes) {
                why = where + "unknown mesh " + tok[k] + " (the scene has " + std::to_string(view.n_meshes) + ")";
                return false;
            }
            const float *e = view.mesh_f + 12 * (size_t)m + 3;
            if (!move_lights && (e[0] != 0.f || e[1] != 0.f || e[2] != 0.f)) {
                why = where + "mesh " + tok[k] + " is emissive; posing a light needs RT_MOVE_LIGHTS=1";
                return false;
            }
            float w[10];
            for (int c = 0; c < 10; ++c) {
                const std::string &t = tok[k + 1 + (size_t)c];
                w[c] = std::strtof(t.c_str(), &end);
                if (end == t.c_str() || *end != '\0' || !std::isfinite(w[c])) {
                    why = where + shape + " (finite)";
                    return false;
                }
            }
            Pose p{(uint32_t)m, {0}};
            check(rt_trs_matrix(w, w + 3, w + 7, p.m));
            for (const Pose &q : frame)
                if (q.mesh == p.mesh) {
                    why = where + "mesh " + tok[k] + " named twice";
                    return false;
                }
            frame.push_back(p);
        }
        frames.push_back(frame);
    }
    if (frames.empty()) {
        why = std::string("RT_POSES: no frame in ") + path;
        return false;
    }
    return true;
}

// RT_POSES: one rt_scene_pose_meshes call per frame; a mesh the frame does not name keeps its last pose.
static void apply_poses(rt_scene *scene, const std::vector<Pose> &now) {
    std::vector<uint32_t> mesh;
    std::vector<double> m;
    for (const Pose &p : now) {
        mesh.push_back(p.mesh);
        m.insert(m.end(), p.m, p.m + 16);
    }
    check(rt_scene_pose_meshes(scene, (uint32_t)mesh.size(), mesh.data(), m.data()));
}

// RT_MOVES: the scene's triangles as frame `now` places them, given what frame `before` (NULL: none)
// had moved.  `base`: the loaded tri array.  A triangle of a mesh `now` names gets v0 = loaded v0 +
// offset (one f32 add per component); every other one is at its loaded position.  A mesh's triangles
// lie scattered in post-build order and every call refits the whole tree, so the update is the range
// from the first to the last triangle of the meshes either frame names, cut only at emissive
// triangles (which may not be touched; with RT_MOVE_LIGHTS they may, and the caller passes no mesh as
// emissive): few calls, the other meshes' records in between as they are.
static void apply_moves(rt_scene *scene, const std::vector<float> &base, const std::vector<uint32_t> &tri_mesh,
                        const std::vector<uint8_t> &mesh_emissive, const std::vector<Move> *before, const std::vector<Move> &now) {
    std::vector<const Move *> move_of(mesh_emissive.size(), nullptr);
    std::vector<uint8_t> touched(mesh_emissive.size(), 0);
    if (before)
        for (const Move &m : *before) touched[m.mesh] = 1;
    for (const Move &m : now) touched[m.mesh] = 1, move_of[m.mesh] = &m;   // (named twice: the last group holds)
    const size_t n = tri_mesh.size();
    size_t lo = n, hi = 0;
    for (size_t t = 0; t < n; ++t)
        if (touched[tri_mesh[t]]) lo = std::min(lo, t), hi = t + 1;
    std::vector<float> rec;
    for (size_t k = lo; k < hi;) {
        if (mesh_emissive[tri_mesh[k]]) {
            ++k;
            continue;
        }
        size_t e = k;
        while (e < hi && !mesh_emissive[tri_mesh[e]]) ++e;
        rec.assign(base.begin() + 12 * (long)k, base.begin() + 12 * (long)e);
        for (size_t t = k; t < e; ++t)
            if (const Move *mv = move_of[tri_mesh[t]])
                for (int c = 0; c < 3; ++c) rec[12 * (t - k) + (size_t)c] = rec[12 * (t - k) + (size_t)c] + mv->d[c];
        check(rt_scene_update_tris(scene, (uint32_t)k, (uint32_t)(e - k), rec.data(), nullptr, nullptr));
        k = e;
    }
}

// out.ppm -> out.0003.ppm (a name without an extension: the index appended).
static std::string indexed_name(const std::string &path, size_t k) {
    char idx[16];
    std::snprintf(idx, sizeof idx, ".%04zu", k);
    const size_t slash = path.find_last_of('/'), dot = path.find_last_of('.');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return path + idx;
    return path.substr(0, dot) + idx + path.substr(dot);
}

// RT_CAMERAS, RT_MOVES, RT_POSES: one one-shot frame per camera (`cams` empty: the scene's camera for
// every frame of `moves` or `poses`) through the existing frame path; `moves` or `poses` (both empty:
// nothing moves; never both) place the objects before each frame; with `temporal` (RT_TEMPORAL) every frame's sums pass through a history on
// device 0 before the finish.
static void render_cameras(rt_scene *scene, int width, int height, int samples, int n_gpus, int fast_chunk, Denoise &dn,
                           const std::vector<rt_camera> &cams, const std::vector<std::vector<Move>> &moves,
                           const std::vector<std::vector<Pose>> &poses, bool move_lights, const std::string &output, bool temporal, float alpha, const char *aov_out, bool motion) {
    struct Held {   // (freed on every way out, before the scene)
        rt_history *h = nullptr;
        ~Held() { rt_history_free(h); }
    } held;
    rt_params p{};
    p.spp = samples;
    p.row_block = 8;
    if (fast_chunk) {
        p.flags = RT_FLAG_FAST;
        p.fast_chunk = fast_chunk;
    }
    rt_temporal_params tp{alpha, 0.f, 0.f, 0.f, 0};
    std::vector<uint8_t> rgb((size_t)width * height * 3);
    std::vector<float> sums;
    std::vector<float> base;          // RT_MOVES: the loaded triangles and their meshes
    std::vector<uint32_t> tri_mesh;
    std::vector<uint8_t> mesh_emissive;
    if (!moves.empty()) {
        rt_scene_view v;
        check(rt_scene_get_view(scene, &v));
        base.assign(v.tri, v.tri + 12 * (size_t)v.n_tris);
        tri_mesh.resize(v.n_tris);
        for (size_t t = 0; t < v.n_tris; ++t) std::memcpy(&tri_mesh[t], v.tri_attr + 16 * t + 15, 4);
        for (size_t m = 0; m < v.n_meshes; ++m) {
            const float *e = v.mesh_f + 12 * m + 3;
            mesh_emissive.push_back(!move_lights && (e[0] != 0.f || e[1] != 0.f || e[2] != 0.f));
        }
    }
    const size_t n_frames = !cams.empty() ? cams.size() : !poses.empty() ? poses.size() : moves.size();
    for (size_t k = 0; k < n_frames; ++k) {
        if (!cams.empty()) check(rt_scene_set_camera(scene, &cams[k]));
        if (!poses.empty()) apply_poses(scene, poses[k]);
        if (!moves.empty()) apply_moves(scene, base, tri_mesh, mesh_emissive, k ? &moves[k - 1] : nullptr, moves[k]);
        rt_stats st{};
        if (temporal || dn.on) {
            sums.resize((size_t)width * height * 3);
            check(rt_render_frame(scene, &p, n_gpus, nullptr, nullptr, sums.data(), &st));
        }
        if (temporal) {
            if (!held.h) {
                check(rt_history_create(scene, 0, &held.h));   // (the frame has uploaded the scene to device 0)
                if (motion) check(rt_history_enable_motion(held.h));
            }
            check(rt_history_push_frame_u8(held.h, sums.data(), nullptr, samples, &tp, dn.on && !dn.guided ? &dn.params : nullptr,
                                           dn.guided ? &dn.guided_params : nullptr, rgb.data()));
        } else if (dn.on) {
            dn.gbuffer = frame_gbuffer(scene, width, height);   // (this camera's)
            check(dn.frame(sums.data(), nullptr, samples, width, height, rgb.data()));
        } else {
            check(rt_render_frame(scene, &p, n_gpus, nullptr, rgb.data(), nullptr, &st));
        }
        const std::string name = indexed_name(output, k);
        check(rt_write_ppm(name.c_str(), rgb.data(), width, height));
        if (aov_out && *aov_out) write_aovs(indexed_name(aov_out, k), frame_gbuffer(scene, width, height), width, height);
        std::cout << "Frame " << k << " drawn into " << name << " (render " << st.render_ms << " ms)" << std::endl;
    }
}

static int int_arg(const char *s) { return std::stoi(std::string(s).substr(0, std::string(s).find(' '))); }

int main(int argc, char *argv[]) {
    if (argc < 5 || argc > 6)
        throw std::runtime_error("Invalid arguments - " + std::to_string(argc) + " (expected: 5)");
    std::string input = argv[1];
    int width = int_arg(argv[2]), height = int_arg(argv[3]), samples = int_arg(argv[4]);
    std::string output = argc == 6 ? argv[5] : "output.ppm";

    std::cout << "Loading scene." << std::endl;
    auto t0 = std::chrono::steady_clock::now();
    rt_scene *scene = nullptr;
    check(rt_scene_load_gltf(input.c_str(), width, height, samples, &scene));
    auto t1 = std::chrono::steady_clock::now();
    std::cout << "Scene loaded: " << std::setprecision(2) << std::chrono::duration<double>(t1 - t0).count()
              << " seconds." << std::endl;
    std::cout << std::setprecision(6) << "Rendering scene." << std::endl;
    const char *g = std::getenv("RT_GPUS");
    const int n_gpus = g ? std::atoi(g) : 0;   // 0: every visible device
    const char *pass_env = std::getenv("RT_PASS_SPP"), *ckpt = std::getenv("RT_CHECKPOINT");
    const char *adapt_env = std::getenv("RT_ADAPT"), *counts_out = std::getenv("RT_COUNTS_OUT");
    const bool adaptive = adapt_env && *adapt_env;
    const float adapt = adaptive ? std::strtof(adapt_env, nullptr) : 0.f;
    Denoise dn;
    if (const char *dn_env = std::getenv("RT_DENOISE"); dn_env && *dn_env) {
        dn.on = true;
        dn.params.iterations = std::atoi(dn_env);
        if (dn.params.iterations < 1 || dn.params.iterations > 6) {
            std::cerr << "rt_solution: RT_DENOISE must be 1..6" << std::endl;
            rt_scene_free(scene);
            return 1;
        }
    }
    if (const char *dg_env = std::getenv("RT_DENOISE_GUIDED"); dg_env && *dg_env) {
        if (dn.on) {
            std::cerr << "rt_solution: RT_DENOISE and RT_DENOISE_GUIDED are both set; choose one filter" << std::endl;
            rt_scene_free(scene);
            return 1;
        }
        dn.on = dn.guided = true;
        dn.guided_params.iterations = std::atoi(dg_env);
        if (dn.guided_params.iterations < 1 || dn.guided_params.iterations > 6) {
            std::cerr << "rt_solution: RT_DENOISE_GUIDED must be 1..6" << std::endl;
            rt_scene_free(scene);
            return 1;
        }
    }
    const char *aov_out = std::getenv("RT_AOV_OUT");
    const char *fast_env = std::getenv("RT_FAST");
    const int fast_chunk = fast_env && *fast_env ? std::atoi(fast_env) : 0;
    if (fast_env && *fast_env && fast_chunk < 1) throw std::runtime_error("RT_FAST must be >= 1");
    const char *mom_env = std::getenv("RT_MOMENTS"), *var_out = std::getenv("RT_VARIANCE_OUT");
    const bool moments = mom_env && *mom_env && std::atoi(mom_env) != 0;
    if (moments && !fast_chunk) {
        std::cerr << "rt_solution: RT_MOMENTS needs RT_FAST (only fast accumulators keep moments)" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    if (moments && !(pass_env && *pass_env) && !adaptive) {
        std::cerr << "rt_solution: RT_MOMENTS needs a pass mode (RT_PASS_SPP or RT_ADAPT): moments live in accumulators" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    if (var_out && *var_out && !moments) {
        std::cerr << "rt_solution: RT_VARIANCE_OUT needs RT_MOMENTS" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    dn.measured = moments;
    const char *cams_env = std::getenv("RT_CAMERAS"), *temporal_env = std::getenv("RT_TEMPORAL");
    const char *moves_env = std::getenv("RT_MOVES");
    const bool cams_on = cams_env && *cams_env, temporal_on = temporal_env && *temporal_env;
    const char *poses_env = std::getenv("RT_POSES");
    const bool poses_on = poses_env && *poses_env;
    if (poses_on && moves_env && *moves_env) {
        std::cerr << "rt_solution: RT_POSES and RT_MOVES are both set; choose one way to move the meshes" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    const bool moves_on = (moves_env && *moves_env) || poses_on;   // (a frame per line, either way)
    const char *move_lights_env = std::getenv("RT_MOVE_LIGHTS");
    const bool move_lights = moves_on && move_lights_env && std::atoi(move_lights_env) != 0;
    const char *motion_env = std::getenv("RT_MOTION");
    const bool motion_on = motion_env && *motion_env && std::atoi(motion_env) != 0;
    if (motion_on && (!temporal_on || !moves_on)) {
        std::cerr << "rt_solution: RT_MOTION needs " << (!temporal_on ? "RT_TEMPORAL" : "RT_MOVES or RT_POSES")
                  << " (motion records carry a temporal history along moved objects)" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    if (temporal_on && !cams_on && !motion_on) {
        std::cerr << "rt_solution: RT_TEMPORAL needs RT_CAMERAS (a still view gains nothing from a history: use RT_PASS_SPP)" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    if (cams_on && ((pass_env && *pass_env) || (ckpt && *ckpt) || adaptive)) {
        std::cerr << "rt_solution: RT_CAMERAS excludes RT_PASS_SPP, RT_ADAPT and RT_CHECKPOINT (one one-shot frame per camera)" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    if (moves_on && ((pass_env && *pass_env) || (ckpt && *ckpt) || adaptive)) {
        std::cerr << "rt_solution: " << (poses_on ? "RT_POSES" : "RT_MOVES") << " excludes RT_PASS_SPP, RT_ADAPT and RT_CHECKPOINT (one one-shot frame per line)" << std::endl;
        rt_scene_free(scene);
        return 1;
    }
    if (cams_on || moves_on) {
        std::vector<rt_camera> cams;
        std::vector<std::vector<Move>> moves;
        std::vector<std::vector<Pose>> poses;
        std::string why;
        const float alpha = temporal_on ? std::strtof(temporal_env, nullptr) : 0.f;
        bool ok = !cams_on || read_cameras(cams_env, cams, why);
        if (ok && moves_on) {
            rt_scene_view v;
            check(rt_scene_get_view(scene, &v));
            if (move_lights && rt_scene_enable_light_updates(scene) != RT_OK) {
                why = std::string("RT_MOVE_LIGHTS: ") + rt_last_error();
                ok = false;
            }
            if (ok && poses_on && rt_scene_enable_poses(scene) != RT_OK) {
                why = std::string("RT_POSES: ") + rt_last_error();
                ok = false;
            }
            ok = ok && (poses_on ? read_poses(poses_env, v, move_lights, poses, why) : read_moves(moves_env, v, move_lights, moves, why));
            const size_t n_lines = poses_on ? poses.size() : moves.size();
            if (ok && cams_on && cams.size() != n_lines) {
                why = "RT_CAMERAS holds " + std::to_string(cams.size()) + " frames and " + (poses_on ? "RT_POSES " : "RT_MOVES ") + std::to_string(n_lines) +
                      ": the line counts must be equal";
                ok = false;
            }
        }
        if (!ok || !(alpha >= 0.f && alpha <= 1.f)) {
            std::cerr << "rt_solution: " << (why.empty() ? std::string("RT_TEMPORAL must be in 0..1") : why) << std::endl;
            rt_scene_free(scene);
            return 1;
        }
        const size_t n_frames = cams_on ? cams.size() : poses_on ? poses.size() : moves.size();
        try {
            render_cameras(scene, width, height, samples, n_gpus, fast_chunk, dn, cams, moves, poses, move_lights, output, temporal_on, alpha, aov_out,
                           motion_on);
        } catch (const std::exception &e) {
            std::cerr << "rt_solution: " << e.what() << std::endl;
            rt_scene_free(scene);
            return 1;
        }
        double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::cout << "      " << total << " seconds (" << total * 1000 << " ms) elapsed." << std::endl;
        std::cout << n_frames << " frames drawn into " << indexed_name(output, 0) << " .. " << indexed_name(output, n_frames - 1)
                  << std::endl;
        rt_scene_free(scene);
        return 0;
    }
    if ((pass_env && *pass_env) || (ckpt && *ckpt) || adaptive) {
        const int pass_spp = pass_env && *pass_env ? std::atoi(pass_env) : 0;
        if (pass_env && *pass_env && pass_spp < 1) throw std::runtime_error("RT_PASS_SPP must be >= 1");
        try {
            render_passes(scene, width, height, samples, n_gpus, pass_spp, ckpt && *ckpt ? ckpt : nullptr, output,
                          adaptive ? &adapt : nullptr, adaptive && counts_out && *counts_out ? counts_out : nullptr,
                          fast_chunk, &dn, moments, moments && var_out && *var_out ? var_out : nullptr);
            if (aov_out && *aov_out) {
                if (dn.gbuffer.empty()) dn.gbuffer = frame_gbuffer(scene, width, height);
                write_aovs(aov_out, dn.gbuffer, width, height);
            }
        } catch (const std::exception &e) {   // (a checkpoint that does not fit, a failed pass: the message, status 1)
            std::cerr << "rt_solution: " << e.what() << std::endl;
            rt_scene_free(scene);
            return 1;
        }
        double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::cout << "      " << total << " seconds (" << total * 1000 << " ms) elapsed." << std::endl;
        std::cout << "Frame drawn into " << output << std::endl;
        rt_scene_free(scene);
        return 0;
    }
    rt_params p{};
    p.spp = samples;
    p.row_block = 8;
    if (fast_chunk) {
        p.flags = RT_FLAG_FAST;
        p.fast_chunk = fast_chunk;
    }
    rt_stats st{};
    // every shard finished to 8 bits on its GPU and gathered device-to-device onto GPU 0
    std::vector<uint8_t> rgb((size_t)width * height * 3);
    if (dn.on) {   // the float frame gathered instead, filtered on device 0, then the same finish
        std::vector<float> sums((size_t)width * height * 3);
        check(rt_render_frame(scene, &p, n_gpus, nullptr, nullptr, sums.data(), &st));
        dn.gbuffer = frame_gbuffer(scene, width, height);
        check(dn.frame(sums.data(), nullptr, samples, width, height, rgb.data()));
    } else {
        check(rt_render_frame(scene, &p, n_gpus, nullptr, rgb.data(), nullptr, &st));
    }
    if (aov_out && *aov_out) {
        if (dn.gbuffer.empty()) dn.gbuffer = frame_gbuffer(scene, width, height);
        write_aovs(aov_out, dn.gbuffer, width, height);
    }
    double total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "      " << total << " seconds (" << total * 1000 << " ms) elapsed; render " << st.render_ms
              << " ms on " << st.devices << " MI355X." << std::endl;
    check(rt_write_ppm(output.c_str(), rgb.data(), width, height));
    std::cout << "Frame drawn into " << output << std::endl;
    rt_scene_free(scene);
    return 0;
}
