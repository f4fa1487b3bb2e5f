// Per-mesh material records and the device texture layout: plain C++, shared by the scene
// upload (rt_device.hip ensure_blob) and by host programs that check the shading pass's
// addressing (tests/native/shade_gather_host.cpp).
//
// A record is 128 B (32 dwords), 128-B aligned in the scene blob, so a shaded hit reads all
// of its mesh's material data in one round trip (rt_path.h shade_pre, RT_SHADE_GATHER):
//   dwords  0..11  the mesh's 12 mesh_f floats (base rgb, emission rgb, metallic, roughness^2,
//                  alpha, 3 unused), bit for bit
//   dwords 12..15  its 4 mesh_tex indices (base, normal, metallic-roughness, emission; < 0: absent)
//   dwords 16..27  the four slots' texture descriptors inline, 3 dwords each: offset of the
//                  texture in the (tiled) texel array, width, height
//   dwords 28..31  zero
// An absent slot gets the descriptor (0, 1, 1): every address computed from it is texel 0,
// which exists (the device texel array is never empty), so a lane may load through it and
// ignore the value; its mesh_tex index < 0 is what marks it absent.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rtmat {

constexpr int kRecDwords = 32;
constexpr int kRecTex = 12;    // dword of mesh_tex[0]
constexpr int kRecDesc = 16;   // dword of slot 0's descriptor

// Device texture layout: texture t's texels in 4x4 tiles, tile (tx, ty) at tile index
// ty * ceil(w/4) + tx, texel (x & 3, y & 3) at 4 * (y & 3) + (x & 3) inside it; info_out keeps
// (offset in texels, width, height, channels).  `out` is never empty: a scene without
// textures gets one zero tile, the target of the absent slots' descriptors.
inline void tile_textures(const std::vector<uint32_t> &info, const std::vector<uint8_t> &texels,
                          std::vector<uint32_t> &info_out, std::vector<uint32_t> &out) {
    const size_t n = info.size() / 4;
    info_out = info;
    out.clear();
    for (size_t t = 0; t < n; ++t) {
        const uint32_t off = info[4 * t], w = info[4 * t + 1], h = info[4 * t + 2];
        const uint32_t tw = (w + 3) / 4, th = (h + 3) / 4;
        const size_t base = out.size();
        info_out[4 * t] = (uint32_t)base;
        out.resize(base + (size_t)tw * th * 16, 0u);
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x) {
                uint32_t v;
                std::memcpy(&v, &texels[4 * ((size_t)off + (size_t)y * w + x)], 4);
                out[base + ((size_t)(y >> 2) * tw + (x >> 2)) * 16 + (y & 3) * 4 + (x & 3)] = v;
            }
    }
    if (out.empty()) out.resize(16, 0u);
}

// The records of `n_meshes` meshes from the scene tables; tex_info is the layout the reader
// addresses (4 dwords per texture: offset, width, height, channels).  False where a mesh
// names a texture that does not exist.
inline bool build_records(const float *mesh_f, const int32_t *mesh_tex, size_t n_meshes, const uint32_t *tex_info,
                          size_t n_textures, std::vector<uint32_t> &rec) {
    rec.assign(n_meshes * kRecDwords, 0u);
    for (size_t m = 0; m < n_meshes; ++m) {
        uint32_t *r = &rec[m * kRecDwords];
        std::memcpy(r, mesh_f + 12 * m, 12 * sizeof(float));
        std::memcpy(r + kRecTex, mesh_tex + 4 * m, 4 * sizeof(int32_t));
        for (int s = 0; s < 4; ++s) {
            const int32_t t = mesh_tex[4 * m + s];
            uint32_t *d = r + kRecDesc + 3 * s;
            if (t < 0) {
                d[0] = 0u; d[1] = 1u; d[2] = 1u;
                continue;
            }
            if ((size_t)t >= n_textures) return false;
            d[0] = tex_info[4 * (size_t)t]; d[1] = tex_info[4 * (size_t)t + 1]; d[2] = tex_info[4 * (size_t)t + 2];
        }
    }
    return true;
}

}  // namespace rtmat
