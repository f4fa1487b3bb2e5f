// rt_refit_plan.h — what a refit needs to know about a scene's tree, made once per scene on the
// host (no HIP): the level ranges of the device's breadth-first numbering, the maps between the
// host mirror's build order and that numbering, and which meshes are emissive (their triangles may
// not move: the light list and the light BVH are not remapped), and, for a scene that opted in to
// movable lights, the LightPlan below.
//
// The device refit (rt_refit_device.h) launches one kernel per level, deepest first; a level is the
// contiguous id range [level_first[l], level_first[l + 1]) and every child lies in the level after
// its parent's, so a launch reads only what the launch before it wrote.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rt_bvh_layout.h"

namespace rtrp {

struct Plan {
    std::vector<uint32_t> build_of_bfs;    // [bfs id] -> build-order id (rt_bvh_layout.h bfs_nodes' order)
    std::vector<uint32_t> bfs_of_build;    // [build-order id] -> bfs id
    std::vector<uint32_t> level_first;     // levels + 1 entries: level l = bfs ids [level_first[l], level_first[l + 1])
    std::vector<uint8_t> mesh_emissive;    // [mesh]: emission not all zero
    size_t levels() const { return level_first.empty() ? 0 : level_first.size() - 1; }
};

// `order`: bfs_nodes' order for `node` (build-order records, 8 words each); mesh_f: 12 words per mesh.
inline Plan make_plan(const std::vector<float> &node, const std::vector<uint32_t> &order, const std::vector<float> &mesh_f) {
    Plan p;
    const size_t n = node.size() / 8;
    p.build_of_bfs = order;
    p.bfs_of_build.assign(n, 0);
    for (size_t k = 0; k < order.size(); ++k) p.bfs_of_build[order[k]] = (uint32_t)k;
    // breadth-first ids are sorted by depth: a level ends where the depth steps up
    std::vector<uint32_t> depth(order.size(), 0);
    for (size_t k = 0; k < order.size(); ++k) {
        const uint32_t u = order[k];
        if (k == 0 || depth[k] != depth[k - 1]) p.level_first.push_back((uint32_t)k);
        if (rtd::node_word(node, u, 7) < 3u) {
            const uint32_t a = p.bfs_of_build[rtd::node_word(node, u, 6)];
            depth[a] = depth[a + 1] = depth[k] + 1;
        }
    }
    if (!order.empty()) p.level_first.push_back((uint32_t)order.size());
    const size_t nm = mesh_f.size() / 12;
    p.mesh_emissive.assign(nm, 0);
    for (size_t m = 0; m < nm; ++m)
        p.mesh_emissive[m] = mesh_f[12 * m + 3] != 0.f || mesh_f[12 * m + 4] != 0.f || mesh_f[12 * m + 5] != 0.f;
    return p;
}

inline Plan make_plan(const std::vector<float> &node, const std::vector<float> &mesh_f) {
    std::vector<uint32_t> order;
    (void)rtd::bfs_nodes(node, &order);
    return make_plan(node, order, mesh_f);
}

// Movable lights (rt_scene_enable_light_updates): which triangle each light record restates, and the
// light tree's levels.  light_node is in build order on the device too, so a level is not an id range:
// node_by_depth holds the ids sorted by depth (ties in id order) and level l is
// node_by_depth[level_first[l] .. level_first[l + 1]).
struct LightPlan {
    std::vector<uint32_t> tri_of_light;    // [light] -> triangle
    std::vector<uint32_t> light_of_tri;    // [triangle] -> light, or kNone
    std::vector<uint32_t> node_by_depth;
    std::vector<uint32_t> level_first;     // levels + 1 entries
    static constexpr uint32_t kNone = 0xFFFFFFFFu;
    size_t levels() const { return level_first.empty() ? 0 : level_first.size() - 1; }
    bool touches(uint32_t first, uint32_t count) const {   // a light triangle in [first, first + count)
        for (uint32_t k = first; k < first + count; ++k)
            if (light_of_tri[k] != kNone) return true;
        return false;
    }
};

// The map rule: the lights in ascending index; light k takes the lowest-numbered triangle of an
// emissive mesh that is not yet taken and whose 12 words equal the light's words 0..11 bit for bit.
// Every light must find one and no emissive triangle may be left over.  The tree must be what the
// sweep and the level launches rely on: leaf ranges within the lights, children above their parents.
// Returns "" and fills `out`, or says what is wrong and leaves `out` alone.
inline std::string make_light_plan(const std::vector<float> &tri, const std::vector<float> &tri_attr,
                                   const std::vector<uint8_t> &mesh_emissive, const std::vector<float> &light,
                                   const std::vector<float> &light_node, LightPlan *out) {
    const size_t nt = tri.size() / 12, nl = light.size() / 16, nn = light_node.size() / 8;
    using Key = std::array<uint32_t, 12>;
    auto key_of = [](const float *w) {
        Key k;
        std::memcpy(k.data(), w, sizeof k);
        return k;
    };
    std::map<Key, std::pair<std::vector<uint32_t>, size_t>> free_tris;   // ids ascending, and how many are taken
    std::vector<uint8_t> emissive(nt, 0);
    for (size_t t = 0; t < nt; ++t) {
        uint32_t m;
        std::memcpy(&m, &tri_attr[16 * t + 15], 4);
        if (m < mesh_emissive.size() && mesh_emissive[m]) {
            emissive[t] = 1;
            free_tris[key_of(&tri[12 * t])].first.push_back((uint32_t)t);
        }
    }
    LightPlan p;
    p.tri_of_light.assign(nl, LightPlan::kNone);
    p.light_of_tri.assign(nt, LightPlan::kNone);
    for (size_t k = 0; k < nl; ++k) {
        auto it = free_tris.find(key_of(&light[16 * k]));
        if (it == free_tris.end() || it->second.second == it->second.first.size())
            return "light " + std::to_string(k) + " restates no free triangle of an emissive mesh";
        const uint32_t t = it->second.first[it->second.second++];
        p.tri_of_light[k] = t;
        p.light_of_tri[t] = (uint32_t)k;
    }
    for (size_t t = 0; t < nt; ++t)
        if (emissive[t] && p.light_of_tri[t] == LightPlan::kNone)
            return "triangle " + std::to_string(t) + " belongs to an emissive mesh and has no light";
    if (nl && !nn) return "lights without a light BVH";
    std::vector<uint32_t> depth(nn, 0);
    uint32_t deepest = 0;
    for (size_t i = 0; i < nn; ++i) {
        const uint32_t a = rtd::node_word(light_node, i, 6), b = rtd::node_word(light_node, i, 7);
        if ((b & 3u) == 3u) {
            if ((uint64_t)a + (b >> 2) > nl) return "light node " + std::to_string(i) + ": leaf range beyond the lights";
        } else {
            if (b > 2 || a <= i || (size_t)a + 1 >= nn) return "light node " + std::to_string(i) + ": bad internal node";
            depth[a] = depth[a + 1] = depth[i] + 1;
        }
        if (depth[i] > deepest) deepest = depth[i];
    }
    p.level_first.assign(nn ? deepest + 2 : 0, 0);
    for (size_t i = 0; i < nn; ++i) ++p.level_first[depth[i] + 1];
    for (size_t l = 1; l < p.level_first.size(); ++l) p.level_first[l] += p.level_first[l - 1];
    p.node_by_depth.assign(nn, 0);
    std::vector<uint32_t> at(p.level_first.begin(), p.level_first.end());
    for (size_t i = 0; i < nn; ++i) p.node_by_depth[at[depth[i]]++] = (uint32_t)i;
    *out = std::move(p);
    return "";
}

}  // namespace rtrp
