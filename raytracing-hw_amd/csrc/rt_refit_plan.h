// rt_refit_plan.h — what a refit needs to know about a scene's tree, made once per scene on the
// host (no HIP): the level ranges of the device's breadth-first numbering, the maps between the
// host mirror's build order and that numbering, and which meshes are emissive (their triangles may
// not move: the light list and the light BVH are not remapped).
//
// The device refit (rt_refit_device.h) launches one kernel per level, deepest first; a level is the
// contiguous id range [level_first[l], level_first[l + 1]) and every child lies in the level after
// its parent's, so a launch reads only what the launch before it wrote.
#pragma once
#include <cstdint>
#include <cstring>
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

}  // namespace rtrp
