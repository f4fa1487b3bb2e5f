// refit_plan_host.cpp — the refit's host-only plan (raytracing-hw_amd/csrc/rt_refit_plan.h) and the
// device's breadth-first node array (rt_bvh_layout.h) behind plain C entries, for
// tests/test_refit.py.  No HIP.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../raytracing-hw_amd/csrc/rt_refit_plan.h"

extern "C" {

// node: n_nodes x 8 (build order); mesh_f: n_meshes x 12.  Outputs (caller's buffers):
// build_of_bfs, bfs_of_build: n_nodes each; level_first: up to n_nodes + 1 entries, *n_levels the
// level count; mesh_emissive: n_meshes bytes; bfs_node: n_nodes x 8, the renumbered records.
int rp_plan(const float *node, uint32_t n_nodes, const float *mesh_f, uint32_t n_meshes, uint32_t *build_of_bfs,
            uint32_t *bfs_of_build, uint32_t *level_first, uint32_t *n_levels, uint8_t *mesh_emissive, float *bfs_node) {
    const std::vector<float> nodes(node, node + 8 * (size_t)n_nodes), mf(mesh_f, mesh_f + 12 * (size_t)n_meshes);
    std::vector<uint32_t> order;
    const std::vector<float> bfs = rtd::bfs_nodes(nodes, &order);
    const rtrp::Plan p = rtrp::make_plan(nodes, order, mf);
    const rtrp::Plan q = rtrp::make_plan(nodes, mf);   // (the form that computes the order itself)
    if (q.build_of_bfs != p.build_of_bfs || q.level_first != p.level_first) return -1;
    if (p.build_of_bfs.size() != n_nodes || p.bfs_of_build.size() != n_nodes || p.mesh_emissive.size() != n_meshes) return -2;
    std::memcpy(build_of_bfs, p.build_of_bfs.data(), 4 * (size_t)n_nodes);
    std::memcpy(bfs_of_build, p.bfs_of_build.data(), 4 * (size_t)n_nodes);
    std::memcpy(level_first, p.level_first.data(), 4 * p.level_first.size());
    *n_levels = (uint32_t)p.levels();
    std::memcpy(mesh_emissive, p.mesh_emissive.data(), n_meshes);
    std::memcpy(bfs_node, bfs.data(), 4 * bfs.size());
    return 0;
}

}  // extern "C"
