// Stand-alone proof of the shading gather's addressing (rt_path.h shade_pre, RT_SHADE_GATHER),
// on the CPU, before it reaches a device: a load through a wrong "safe" address would be a
// device fault.  Built with -fsanitize=address,undefined by tests/test_shade_gather_host.py.
//
//   shade_gather_host [scene.bin ...]
//
// For every scene (the built-in ones and each file: u32 n_meshes, n_textures, n_texels, then
// mesh_f 12 f32/mesh, mesh_tex 4 i32/mesh, tex_info 4 u32/texture, texels RGBA8) it tiles the
// textures and builds the material records with the upload's own functions (rt_material.h),
// then for every (mesh, slot) and a sweep of texture coordinates runs the gather's address
// function over the device layout, tex_taps<true>, and checks that
//   - every tap lies inside the texel array, and inside the slot's own texture;
//   - an absent slot has the descriptor (0, 1, 1) and every tap is texel 0;
//   - tex_decode of the four tiled texels is, bit for bit, tex_sample_ti on the row-major
//     host view of the same texture, and a plain restatement of the reference's bilinear
//     sample with % (finite coordinates; both decodes).
// Prints one line per scene and exits 0, or the first failures and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../raytracing-hw_amd/csrc/rt_material.h"
#include "../../raytracing-hw_amd/csrc/rt_path.h"

namespace {

struct SceneTables {
    std::string name;
    std::vector<float> mesh_f;
    std::vector<int32_t> mesh_tex;
    std::vector<uint32_t> tex_info;
    std::vector<uint8_t> texels;
};

int g_fail = 0;
void fail(const SceneTables &s, const char *what, size_t mesh, int slot, float x, float y) {
    if (++g_fail <= 20) std::fprintf(stderr, "FAIL %s: %s (mesh %zu slot %d tc %a %a)\n", s.name.c_str(), what, mesh, slot, x, y);
}

uint32_t lcg(uint32_t &st) { return st = st * 1664525u + 1013904223u; }

void add_texture(SceneTables &s, uint32_t w, uint32_t h, uint32_t &seed) {
    s.tex_info.insert(s.tex_info.end(), {(uint32_t)(s.texels.size() / 4), w, h, 4u});
    for (uint32_t k = 0; k < w * h * 4; ++k) s.texels.push_back((uint8_t)(lcg(seed) >> 24));
}
void add_mesh(SceneTables &s, int b, int n, int mr, int e) {
    for (int k = 0; k < 12; ++k) s.mesh_f.push_back(0.125f * (float)(k + 1) + (float)s.mesh_tex.size());
    s.mesh_tex.insert(s.mesh_tex.end(), {b, n, mr, e});
}

bool load(const char *path, SceneTables &s) {
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    uint32_t hd[3];
    bool ok = std::fread(hd, 4, 3, f) == 3;
    if (ok) {
        s.mesh_f.resize((size_t)hd[0] * 12);
        s.mesh_tex.resize((size_t)hd[0] * 4);
        s.tex_info.resize((size_t)hd[1] * 4);
        s.texels.resize((size_t)hd[2] * 4);
        ok = std::fread(s.mesh_f.data(), 4, s.mesh_f.size(), f) == s.mesh_f.size() &&
             std::fread(s.mesh_tex.data(), 4, s.mesh_tex.size(), f) == s.mesh_tex.size() &&
             std::fread(s.tex_info.data(), 4, s.tex_info.size(), f) == s.tex_info.size() &&
             std::fread(s.texels.data(), 1, s.texels.size(), f) == s.texels.size();
    }
    std::fclose(f);
    s.name = path;
    return ok;
}

// Texture::interpolate_sample restated plainly over the row-major texels (finite coordinates).
rtv::V4 plain_sample(const SceneTables &s, const float *lut, int t, float x, float y, bool srgb) {
    const uint32_t off = s.tex_info[4 * t];
    const int W = (int)s.tex_info[4 * t + 1], H = (int)s.tex_info[4 * t + 2];
    x -= std::floor(x);
    y -= std::floor(y);
    x *= (float)W;
    y *= (float)H;
    const int px = (int)std::floor(x), py = (int)std::floor(y);
    const float dx = x - std::floor(x), dy = y - std::floor(y);
    float v[4][4];
    for (int ddx = 0; ddx < 2; ++ddx)
        for (int ddy = 0; ddy < 2; ++ddy) {
            const size_t i = (size_t)off + (size_t)((py + ddy) % H) * W + (size_t)((px + ddx) % W);
            for (int c = 0; c < 4; ++c) v[ddx * 2 + ddy][c] = lut[(srgb ? 0 : 256) + s.texels[4 * i + c]];
        }
    float r[4];
    for (int c = 0; c < 4; ++c)
        r[c] = v[0][c] * (1 - dx) * (1 - dy) + v[1][c] * (1 - dx) * dy + v[2][c] * dx * (1 - dy) + v[3][c] * dx * dy;
    return rtv::V4{r[0], r[1], r[2], r[3]};
}

bool same(rtv::V4 a, rtv::V4 b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check(const SceneTables &s) {
    const size_t n_meshes = s.mesh_f.size() / 12, n_tex = s.tex_info.size() / 4;
    std::vector<uint32_t> tinfo, tiled, rec;
    rtmat::tile_textures(s.tex_info, s.texels, tinfo, tiled);
    if (tiled.empty()) fail(s, "the device texel array is empty", 0, 0, 0.f, 0.f);
    if (!rtmat::build_records(s.mesh_f.data(), s.mesh_tex.data(), n_meshes, tinfo.data(), n_tex, rec)) {
        fail(s, "build_records refused the scene", 0, 0, 0.f, 0.f);
        return;
    }
    if (rec.size() != n_meshes * 32) fail(s, "record size", 0, 0, 0.f, 0.f);
    std::vector<float> lut(512);
    rtd::fill_decode_lut(lut.data());
    std::vector<uint32_t> rows(s.texels.size() / 4 + 1);
    if (!s.texels.empty()) std::memcpy(rows.data(), s.texels.data(), s.texels.size());
    rtd::DevScene sc{};
    sc.texels = rows.data();
    sc.lut = lut.data();

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> sweep = {0.f, -0.f, 1.f, std::nextafter(1.f, 0.f), std::nextafter(1.f, 2.f), 0.5f, 0.25f, 0.999f,
                                -0.25f, -1.f, -1e-30f, -1e-8f, 1e-30f, 2.f, 7.75f, -3.5f, 16777216.f, 1e9f, -1e9f, 3e38f,
                                -3e38f, 1e-45f, -1e-45f, inf, -inf, nan};
    uint32_t seed = 12345u;
    for (int k = 0; k < 24; ++k) sweep.push_back((float)(lcg(seed) >> 8) * (1.f / 16777216.f) * 3.f - 1.f);
    size_t taps = 0, values = 0;
    for (size_t m = 0; m < n_meshes; ++m) {
        const uint32_t *r = &rec[32 * m];
        if (std::memcmp(r, &s.mesh_f[12 * m], 48) || std::memcmp(r + rtmat::kRecTex, &s.mesh_tex[4 * m], 16))
            fail(s, "record tables", m, -1, 0.f, 0.f);
        for (int slot = 0; slot < 4; ++slot) {
            const int t = s.mesh_tex[4 * m + slot];
            const uint32_t *d = r + rtmat::kRecDesc + 3 * slot;
            const uint32_t off = d[0];
            const int W = (int)d[1], H = (int)d[2];
            if (t < 0 && (off != 0u || W != 1 || H != 1)) fail(s, "absent slot's descriptor", m, slot, 0.f, 0.f);
            if (t >= 0 && (off != tinfo[4 * t] || d[1] != tinfo[4 * t + 1] || d[2] != tinfo[4 * t + 2]))
                fail(s, "slot descriptor", m, slot, 0.f, 0.f);
            // per-texture extra coordinates: every texel centre and edge of the first and last rows / columns
            std::vector<float> xs = sweep, ys = sweep;
            for (int k = 0; k <= 2 * W && k <= 12; ++k) xs.push_back((float)k / (float)(2 * W));
            for (int k = 0; k <= 2 * H && k <= 12; ++k) ys.push_back((float)k / (float)(2 * H));
            xs.push_back(((float)W - 0.5f) / (float)W);
            ys.push_back(((float)H - 0.5f) / (float)H);
            const size_t extent = (size_t)((W + 3) / 4) * (size_t)((H + 3) / 4) * 16;
            for (float x : xs)
                for (float y : ys) {
                    uint32_t idx[4];
                    float dx, dy;
                    rtd::tex_taps<true>(off, W, H, rtv::V2{x, y}, idx, dx, dy);
                    for (int k = 0; k < 4; ++k) {
                        ++taps;
                        if (idx[k] >= tiled.size()) { fail(s, "tap outside the texel array", m, slot, x, y); idx[k] = 0; }
                        if (idx[k] < off || idx[k] >= off + extent) fail(s, "tap outside its texture", m, slot, x, y);
                        if (t < 0 && idx[k] != 0u) fail(s, "absent slot's tap is not texel 0", m, slot, x, y);
                    }
                    if (t < 0 || !std::isfinite(x) || !std::isfinite(y)) continue;
                    const uint32_t texel[4] = {tiled[idx[0]], tiled[idx[1]], tiled[idx[2]], tiled[idx[3]]};
                    const uint4 ti{s.tex_info[4 * t], s.tex_info[4 * t + 1], s.tex_info[4 * t + 2], 4u};
                    for (int srgb = 0; srgb < 2; ++srgb) {
                        ++values;
                        const rtv::V4 g = rtd::tex_decode(lut.data(), texel, dx, dy, srgb != 0);
                        if (!same(g, rtd::tex_sample_ti(sc, ti, rtv::V2{x, y}, srgb != 0)))
                            fail(s, "tex_taps + tex_decode differs from tex_sample_ti", m, slot, x, y);
                        if (!same(g, plain_sample(s, lut.data(), t, x, y, srgb != 0)))
                            fail(s, "tex_taps + tex_decode differs from the plain bilinear sample", m, slot, x, y);
                    }
                }
        }
    }
    std::printf("%s: %zu meshes, %zu textures, %zu taps in bounds, %zu samples bit-equal\n", s.name.c_str(), n_meshes, n_tex,
                taps, values);
}

}  // namespace

int main(int argc, char **argv) {
    uint32_t seed = 20261020u;
    {   // no textures at all
        SceneTables s;
        s.name = "zero-texture";
        for (int k = 0; k < 3; ++k) add_mesh(s, -1, -1, -1, -1);
        check(s);
    }
    {   // the only texture is 1x1, in every subset of the slots
        SceneTables s;
        s.name = "single 1x1";
        add_texture(s, 1, 1, seed);
        for (int k = 0; k < 16; ++k) add_mesh(s, k & 1 ? 0 : -1, k & 2 ? 0 : -1, k & 4 ? 0 : -1, k & 8 ? 0 : -1);
        check(s);
    }
    {   // odd sizes (partial tiles, 1-texel sides); the last texture in every slot of a mesh
        SceneTables s;
        s.name = "last texture in every slot";
        const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {5, 1}, {5, 3}, {3, 5}, {13, 6}, {2, 2}, {7, 9}, {6, 13}, {4, 4}, {9, 4}, {4, 10}};
        for (auto &wh : sizes) add_texture(s, wh[0], wh[1], seed);
        const int last = (int)(s.tex_info.size() / 4) - 1;
        add_mesh(s, last, last, last, last);
        for (int t = 0; t <= last; ++t) add_mesh(s, t, (t + 1) % (last + 1), -1, last - t);
        for (int k = 0; k < 16; ++k) add_mesh(s, k & 1 ? k % (last + 1) : -1, k & 2 ? last : -1, k & 4 ? 0 : -1, k & 8 ? last : -1);
        check(s);
    }
    {   // a texture index past the table is refused by the builder
        SceneTables s;
        add_texture(s, 2, 2, seed);
        add_mesh(s, 1, -1, -1, -1);
        std::vector<uint32_t> rec;
        if (rtmat::build_records(s.mesh_f.data(), s.mesh_tex.data(), 1, s.tex_info.data(), 1, rec)) {
            std::fprintf(stderr, "FAIL: build_records accepted a texture index out of range\n");
            ++g_fail;
        }
    }
    for (int a = 1; a < argc; ++a) {
        SceneTables s;
        if (!load(argv[a], s)) {
            std::fprintf(stderr, "FAIL: cannot read %s\n", argv[a]);
            ++g_fail;
            continue;
        }
        check(s);
    }
    if (g_fail) std::fprintf(stderr, "%d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
