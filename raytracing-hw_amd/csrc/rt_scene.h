// rt_scene.h — host-side scene object behind the opaque rt_scene handle (include/rt_hw.h).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_hw.h"

struct rt_device_scene;  // owned by rt_device.hip: one per device the scene is uploaded to
struct rt_device_blob;   // owned by rt_device.hip: the device image of the scene, built once
namespace rtrp {
struct Plan;             // rt_refit_plan.h: owned by rt_host.cpp
struct LightPlan;        // rt_refit_plan.h: owned by rt_host.cpp
}

constexpr int kRtMaxDevices = 64;

struct rt_scene {
    int32_t width = 0, height = 0, samples = 0, ray_depth = 6;
    float max_distance = 1e9f;
    float cam_pos[3] = {0, 0, 0};
    float cam_axes[9] = {0};
    float cam_fov[2] = {0, 0};
    float tan_half_fov[2] = {0, 0};
    uint32_t view_epoch = 0;   // rt_scene_set_camera and rt_scene_update_tris* calls so far (an accumulator remembers the one it renders)
    uint32_t geom_epoch = 0;   // rt_scene_update_tris* calls alone (a history that carries motion remembers the one it saw)

    std::vector<float> tri, tri_attr, tri_tan, node;
    uint32_t bvh_depth = 0;
    std::vector<float> light, light_node;
    uint32_t light_bvh_depth = 0;
    std::vector<float> mesh_f;
    std::vector<int32_t> mesh_tex;
    std::vector<double> mesh_nt;
    std::vector<uint32_t> tex_info;
    std::vector<uint8_t> texels;

    rt_device_scene *dev[kRtMaxDevices] = {};   // [HIP device id]
    rt_device_blob *blob = nullptr;
    rtrp::Plan *refit_plan = nullptr;           // made by the first rt_scene_update_tris* (rt_refit_plan.h)
    rtrp::LightPlan *light_plan = nullptr;      // made by rt_scene_enable_light_updates; non-NULL: lights may move
    std::vector<uint32_t> bfs_order;            // build-order ids in the device's numbering, kept by the blob's builder

    // posable meshes (rt_pose.h): what the loader keeps, or rt_scene_set_rest hands in; empty: no rest data
    std::vector<float> rest;                    // n_tris x 18: object-space q0 q1 q2, n0 n1 n2 (post-build order)
    std::vector<uint32_t> tri_source;           // n_tris: the triangle's index in load order
    std::vector<double> mesh_matrix;            // n_meshes x 16: the mesh's current node matrix
    bool poses_on = false;                      // rt_scene_enable_poses succeeded
    std::vector<uint32_t> mesh_first, mesh_last;   // [mesh]: its first and last triangle (first > last: none); with poses_on
};

// error plumbing shared by rt_host.cpp and rt_device.hip
void rt_set_error(const std::string &msg);
int rt_fail(int code, const std::string &msg);

// implemented in rt_device.hip: frees every device copy and the device image
void rt_device_scene_release(rt_scene *s);
// implemented in rt_device.hip: the scene's camera into the launch arguments of every device copy
void rt_device_scene_set_camera(rt_scene *s);

// movable geometry (include/rt_hw.h rt_scene_update_tris*), rt_host.cpp:
// the scene's refit plan, made on first use
const rtrp::Plan &rt_scene_refit_plan(rt_scene *s);
// every refusal both entries share (NULL tri, the range, an emissive mesh's triangle unless the scene
// opted in with rt_scene_enable_light_updates); nothing is changed
int rt_update_tris_check(rt_scene *s, const char *who, uint32_t first, uint32_t count, const float *tri);
// implemented in rt_device.hip: after the host arrays took the new records and the refit boxes, the
// cached device image is patched and every device copy takes the range and refits its own boxes; waits.
// `lights`: the range holds a light's triangle (the host light arrays are already the new ones): the
// image's light arrays are patched and every copy restates its light records and light boxes too
int rt_device_scene_update_tris(rt_scene *s, uint32_t first, uint32_t count, bool attr, bool tan, bool lights);

// posable meshes (include/rt_hw.h rt_scene_pose_meshes), implemented in rt_device.hip (rt_pose_device.h):
// the rest records onto every device copy that exists (later copies take them when they are made)
int rt_device_scene_enable_poses(rt_scene *s);
// after the host twin brought the host arrays up to date: the cached image is patched, and every device
// copy takes the table (per posed mesh: id, M, NT; `table`: 32 doubles each), rewrites those meshes'
// mesh_nt, recomputes the records of their triangles within [first, first + count) from its own rest
// records and refits its boxes (and, with `lights`, its light records and light boxes); waits
int rt_device_scene_pose(rt_scene *s, uint32_t n, const uint32_t *mesh, const double *table, uint32_t first, uint32_t count,
                         bool lights);

// argument checks of rt_denoise / rt_denoise_device (rt_host.cpp): RT_OK and the resolved
// parameters (rt_denoise.h), or the failure as `who` reports it
namespace rtdn {
struct Params;
}
int rt_denoise_check(const char *who, const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                     const float *gbuffer, const rt_denoise_params *params, const float *out_mean, rtdn::Params *resolved);
// the same for rt_denoise_guided and its kin (rt_denoise_guided.h)
namespace rtdg {
struct Params;
}
int rt_denoise_guided_check(const char *who, const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                            const float *gbuffer, const rt_denoise_guided_params *params, const float *out_mean,
                            rtdg::Params *resolved);
// the same for rt_variance_from_moments and its device form (rt_moments.h), which have no parameters
int rt_variance_check(const char *who, const float *sums, const float *moments, const int32_t *counts, int32_t spp, int32_t width,
                      int32_t height, const float *gbuffer, const float *out);

// the same for rt_temporal and its kin (rt_temporal.h); history_prev given: cam_prev and gbuffer_prev must be
namespace rttm {
struct Params;
}
int rt_temporal_check(const char *who, const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                      const float *gbuffer, const rt_camera *cam_prev, const float *gbuffer_prev, const float *history_prev,
                      const rt_temporal_params *params, const float *history_out, rttm::Params *resolved);

// the same for rt_motion and its device form (rt_motion.h), which have no parameters; with n_tris == 0
// the two triangle arrays may be NULL (every record is then a miss's)
int rt_motion_check(const char *who, const float *gbuffer, int32_t width, int32_t height, const float *tri, const float *tri_prev,
                    uint32_t n_tris, const float *out_motion);

// row partition helper (rt_host.cpp)
int64_t rt_shard_rows_impl(int32_t height, int32_t rank, int32_t world, int32_t row_block, int32_t *rows_out);
