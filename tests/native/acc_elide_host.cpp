// acc_elide_host.cpp — TEST ONLY: the traversal's frame rule (rt_wavefront.h trav_pop ELIDE: no best
// frame when the near subtree found no hit) on the CPU, as a stand-alone program built with
// -fsanitize=address,undefined by tests/test_acc_elide.py.
//
//   acc_elide_host trace CASE.bin ...      every ray of every case through trav_step with every best frame,
//                                          through trav_step with the rule, and through closest_hit
//   acc_elide_host emu CASE.bin OUT.bin    the case's frame through the host emulation of the lane-resident
//                                          kernel (mega_emu.h), whose per-lane step follows RT_LANE_ACC_ELIDE
//                                          of this build; writes the sums and the counters to OUT.bin
//
// A case file (tests/test_acc_elide.py case_blob) holds a flattened scene (include/rt_hw.h rt_scene_view,
// array by array) and rays.  trace checks, per ray: primitive, t bits, AABB tests and triangle tests equal
// across the three; with the rule no best frame holding 1e9 is ever written, and the frames pushed and the
// deepest stack are at most those of the form with every best frame; per case with geometry, strictly fewer
// frames in total with the rule (a rule that is silently off fails).  Prints one line per case and exits 0,
// or the first failures and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mega_emu.h"

namespace {

struct Case {
    std::string name;
    int32_t hd[12];   // width, height, samples, ray_depth, n_tris, n_nodes, n_lights, n_light_nodes, n_meshes, n_textures, n_rays, 0
    float cam[17];    // max_distance, cam_pos[3], cam_axes[9], cam_fov[2], tan_half_fov[2]
    uint64_t n_texel_bytes;
    std::vector<float> tri, tri_attr, tri_tan, node, light, light_node, mesh_f, org, dir;
    std::vector<int32_t> mesh_tex;
    std::vector<double> mesh_nt;
    std::vector<uint32_t> tex_info;
    std::vector<uint8_t> texels;
    rt_scene_view view() const {
        rt_scene_view v{};
        v.width = hd[0]; v.height = hd[1]; v.samples = hd[2]; v.ray_depth = hd[3];
        v.max_distance = cam[0];
        std::memcpy(v.cam_pos, cam + 1, 12);
        std::memcpy(v.cam_axes, cam + 4, 36);
        std::memcpy(v.cam_fov, cam + 13, 8);
        std::memcpy(v.tan_half_fov, cam + 15, 8);
        v.n_tris = (uint32_t)hd[4]; v.tri = tri.data(); v.tri_attr = tri_attr.data(); v.tri_tan = tri_tan.data();
        v.n_nodes = (uint32_t)hd[5]; v.node = node.data();
        v.n_lights = (uint32_t)hd[6]; v.light = light.data();
        v.n_light_nodes = (uint32_t)hd[7]; v.light_node = light_node.data();
        v.n_meshes = (uint32_t)hd[8]; v.mesh_f = mesh_f.data(); v.mesh_tex = mesh_tex.data();
        v.mesh_normal_transform = mesh_nt.data();
        v.n_textures = (uint32_t)hd[9]; v.tex_info = tex_info.data(); v.texels = texels.data();
        v.n_texel_bytes = n_texel_bytes;
        return v;
    }
};

template <class T>
bool read_vec(FILE *f, std::vector<T> &v, size_t n) {
    v.assign(n + 16, T());   // (never empty; the traversal reads whole records only)
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

bool load(const char *path, Case &c) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    bool ok = std::fread(c.hd, 4, 12, f) == 12 && std::fread(c.cam, 4, 17, f) == 17 && std::fread(&c.n_texel_bytes, 8, 1, f) == 1;
    for (int k = 0; ok && k < 11; ++k) ok = c.hd[k] >= 0;
    if (ok) {
        const size_t nt = (size_t)c.hd[4], nn = (size_t)c.hd[5], nl = (size_t)c.hd[6], nln = (size_t)c.hd[7], nm = (size_t)c.hd[8],
                     nx = (size_t)c.hd[9], nr = (size_t)c.hd[10];
        ok = read_vec(f, c.tri, 12 * nt) && read_vec(f, c.tri_attr, 16 * nt) && read_vec(f, c.tri_tan, 12 * nt) &&
             read_vec(f, c.node, 8 * nn) && read_vec(f, c.light, 16 * nl) && read_vec(f, c.light_node, 8 * nln) &&
             read_vec(f, c.mesh_f, 12 * nm) && read_vec(f, c.mesh_tex, 4 * nm) && read_vec(f, c.mesh_nt, 16 * nm) &&
             read_vec(f, c.tex_info, 4 * nx) && read_vec(f, c.texels, (size_t)c.n_texel_bytes) && read_vec(f, c.org, 3 * nr) &&
             read_vec(f, c.dir, 3 * nr);
    }
    std::fclose(f);
    c.name = path;
    return ok;
}

// An array stack that counts what is written to it (in the style of far_dist_host.cpp's WatchStack).
struct CountStack {
    uint2 *p;
    long long pushes = 0, best_1e9 = 0;
    int deepest = 0;
    void put(int i, uint2 v) {
        ++pushes;
        if (i + 1 > deepest) deepest = i + 1;
        const float held = __uint_as_float(v.y);
        if (v.x == rtd::kFrameAcc && held == 1e9f) ++best_1e9;
        p[i] = v;
    }
    uint2 get(int i) const { return p[i]; }
};

struct Walk {
    rtd::Hit best;
    rtd::Counters cnt{0, 0, 0, 0, 0, 0, 0};
    long long pushes, best_1e9;
    int deepest;
    bool ended;
};

template <bool ELIDE>
Walk walk(const rtd::DevScene &sc, const rtd::NodeRec &root, const rtd::Ray &r, long long bound) {
    Walk w;
    const rtd::GlobalNodes nodes{sc.node};
    float e;
    const uint32_t bits = rtd::box_hit<false>(root.mn, root.mx, r, e) ? 0u : 8u;
    uint2 frames[rtd::kStack];
    CountStack S{frames};
    rtd::TravState T;
    bool active = rtd::trav_start<true>(bits, root.a, root.b, T, w.cnt);
    for (long long it = 0; active && it < bound; ++it)
        if (rtd::trav_step<true, rtd::kFarDist2, ELIDE>(sc, r, T, S, nodes, w.cnt)) active = false;
    w.ended = !active;
    w.best = T.best;
    w.pushes = S.pushes;
    w.best_1e9 = S.best_1e9;
    w.deepest = S.deepest;
    return w;
}

int g_fail = 0;
void fail(const Case &c, const char *what, long long ray) {
    if (++g_fail <= 20) std::fprintf(stderr, "FAIL %s: %s (ray %lld)\n", c.name.c_str(), what, ray);
}

bool same_hit(const rtd::Hit &a, const rtd::Hit &b) { return a.prim == b.prim && std::memcmp(&a.t, &b.t, 4) == 0; }

void trace(const Case &c) {
    const rt_scene_view v = c.view();
    const rtd::DevScene sc = emu::make(&v);
    const long long n = c.hd[10];
    if (c.hd[4] < 1 || c.hd[5] < 1) {
        std::printf("%s: no geometry\n", c.name.c_str());
        return;
    }
    const rtd::NodeRec root = rtd::load_node(sc.node, 0);
    const long long bound = 4ll * ((long long)c.hd[4] + c.hd[5]) + 64;   // (a walk visits a node or triangle at most once)
    long long off = 0, on = 0, held_1e9 = 0, hits = 0;
    int deep_off = 0, deep_on = 0;
    for (long long i = 0; i < n; ++i) {
        const rtd::Ray r = rtd::make_ray(rtv::V3{c.org[3 * i], c.org[3 * i + 1], c.org[3 * i + 2]},
                                         rtv::V3{c.dir[3 * i], c.dir[3 * i + 1], c.dir[3 * i + 2]});
        const Walk a = walk<false>(sc, root, r, bound), b = walk<true>(sc, root, r, bound);
        rtd::Counters cc{0, 0, 0, 0, 0, 0, 0};
        rtd::Hit want{1e9f, 0.f, 0.f, -1};
        rtd::closest_hit<true>(sc, r, want, cc);
        if (!a.ended || !b.ended) fail(c, "a walk did not end", i);
        if (!same_hit(a.best, b.best)) fail(c, "the two frame rules differ in primitive or t", i);
        if (a.best.prim != want.prim || (want.prim >= 0 && !same_hit(a.best, want))) fail(c, "trav_step differs from closest_hit", i);
        if (a.cnt.aabb != b.cnt.aabb || a.cnt.aabb != cc.aabb) fail(c, "AABB tests differ", i);
        if (a.cnt.tri != b.cnt.tri || a.cnt.tri != cc.tri) fail(c, "triangle tests differ", i);
        if (b.best_1e9 != 0) fail(c, "a best frame holding 1e9 was written under the rule", i);
        if (b.pushes > a.pushes) fail(c, "more frames pushed under the rule", i);
        if (b.deepest > a.deepest) fail(c, "a deeper stack under the rule", i);
        if (a.pushes - b.pushes != a.best_1e9) fail(c, "the frames saved are not the best frames that held 1e9", i);
        off += a.pushes;
        on += b.pushes;
        held_1e9 += a.best_1e9;
        hits += a.best.prim >= 0;
        if (a.deepest > deep_off) deep_off = a.deepest;
        if (b.deepest > deep_on) deep_on = b.deepest;
    }
    if (!(on < off)) fail(c, "not strictly fewer frames in total under the rule", -1);
    std::printf("%s: %lld rays, %lld hits, frames %lld -> %lld (%lld best frames held 1e9), deepest %d -> %d: equal\n", c.name.c_str(),
                n, hits, off, on, held_1e9, deep_off, deep_on);
}

int emulate(const Case &c, const char *out_path) {
    const rt_scene_view v = c.view();
    std::vector<float> out((size_t)v.width * v.height * 3, 0.f);
    uint64_t cnt[7] = {};
    emu::Options o;
    if (emu::render_mega<false, false, false>(&v, v.samples, 0, 1, 8, 2, 32, nullptr, out.data(), cnt, o) != 0) return 1;
    FILE *f = std::fopen(out_path, "wb");
    if (!f) return 1;
    const bool ok = std::fwrite(out.data(), 4, out.size(), f) == out.size() && std::fwrite(cnt, 8, 7, f) == 7;
    std::fclose(f);
    std::printf("emu %s: lane step %s, %llu rays\n", c.name.c_str(), rtd::kLaneAccElide ? "with the rule" : "with every best frame",
                (unsigned long long)cnt[0]);
    return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "emu" && argc == 4) {
        Case c;
        if (!load(argv[2], c)) {
            std::fprintf(stderr, "FAIL: cannot read %s\n", argv[2]);
            return 1;
        }
        return emulate(c, argv[3]);
    }
    if (mode != "trace" || argc < 3) {
        std::fprintf(stderr, "usage: acc_elide_host trace CASE.bin ... | emu CASE.bin OUT.bin\n");
        return 2;
    }
    for (int a = 2; a < argc; ++a) {
        Case c;
        if (!load(argv[a], c)) {
            std::fprintf(stderr, "FAIL: cannot read %s\n", argv[a]);
            ++g_fail;
            continue;
        }
        trace(c);
    }
    if (g_fail) std::fprintf(stderr, "%d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
