// rt_refit_device.h — movable geometry on the device: the scatter of new triangle records into a
// scene copy's arrays and the refit of its node boxes (include/rt_hw.h rt_scene_update_tris*), with
// rt_scene_read_device; and movable lights: the light records and the light BVH's boxes of a scene
// that opted in (rt_relight.h), with rt_scene_read_device_lights.  Included by rt_device.hip (one
// translation unit): it uses HIP_TRY, DeviceGuard, grow and the blob's offsets from there, the rules
// of rt_refit.h and rt_relight.h and the plans of rt_refit_plan.h.  The render kernels and DevScene are untouched: their pointers stay const, and
// these kernels write through pointers of their own into the same allocation.
//
// Ordering.  The refit is one launch per tree level, deepest first (the plan's level ranges of the
// breadth-first numbering): a launch reads only the triangles and the level the launch before it
// wrote, and the kernel boundary on the stream is the only ordering.  No atomics, no fences, no
// flags: the result does not depend on scheduling, and nothing can spin.

// New records from `src` (count records, packed) into the scene's arrays at triangle `first`:
// 16-byte quads, one thread per quad.  tri and tri_tan are 3 quads per record, tri_attr 4; the last
// word of a tri_attr record (the mesh id) is kept from the record in place.
__global__ void __launch_bounds__(256) rt_tris_scatter_kernel(float4 *__restrict__ tri, float4 *__restrict__ attr,
                                                              float4 *__restrict__ tan, const float4 *__restrict__ src_tri,
                                                              const float4 *__restrict__ src_attr,
                                                              const float4 *__restrict__ src_tan, long long first,
                                                              long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 3 * count) {
        tri[3 * first + i] = src_tri[i];
        if (src_tan) tan[3 * first + i] = src_tan[i];
    }
    if (src_attr && i < 4 * count) {
        float4 v = src_attr[i];
        if ((i & 3) == 3) v.w = attr[4 * first + i].w;
        attr[4 * first + i] = v;
    }
}

// One tree level: node ids [id0, id0 + n), one thread per node.  A node record is two quads:
// (min.xyz, max.x), (max.y, max.z, a, b).  A leaf folds its triangles' boxes in order; an internal
// node reads its children's 64-byte line (quads 2a .. 2a + 3).  Six words are written: the first
// quad and the first half of the second; a and b never are.
__global__ void __launch_bounds__(256) rt_refit_level_kernel(const float4 *__restrict__ tri, float4 *node, unsigned id0,
                                                             unsigned n) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t id = (size_t)id0 + k;
    const float4 q1 = node[2 * id + 1];
    const uint32_t a = __float_as_uint(q1.z), b = __float_as_uint(q1.w);
    rtrf::Box bx;
    if (rtrf::is_leaf(b)) {
        bx = rtrf::empty_box();
        const uint32_t cnt = b >> 2;
        for (uint32_t t = 0; t < cnt; ++t) {
            const float4 *r = tri + 3 * (size_t)(a + t);
            const float4 t0 = r[0], t1 = r[1];
            const float t2x = r[2].x;   // v0.xyz U.x | U.yz V.xy | V.z ...
            rtrf::grow_box(bx, rtrf::tri_box(t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2x));
        }
    } else {
        const float4 l0 = node[2 * (size_t)a], l1 = node[2 * (size_t)a + 1];
        const float4 r0 = node[2 * (size_t)a + 2], r1 = node[2 * (size_t)a + 3];
        const float lw[6] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y}, rw[6] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y};
        bx = rtrf::pair_box(lw, rw);
    }
    node[2 * id] = make_float4(bx.lo[0], bx.lo[1], bx.lo[2], bx.hi[0]);
    *(float2 *)&node[2 * id + 1] = make_float2(bx.hi[1], bx.hi[2]);
}

// Movable lights (rt_relight.h): the light records of the range's light triangles.  Launched after
// the triangle scatter (the kernel boundary orders them), one thread per triangle of the range: where
// light_of_tri names a light, the triangle's three quads as the scene's own `tri` array now holds
// them go into the light's first three quads and the area into word 12; words 13..15 stay.
__global__ void __launch_bounds__(256) rt_lights_scatter_kernel(const float4 *__restrict__ tri, float4 *__restrict__ light,
                                                                const uint32_t *__restrict__ light_of_tri, long long first,
                                                                long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t k = light_of_tri[first + i];
    if (k == rtrl::kNoLight) return;
    // (native vectors: a float4 whose .x alone is computed with is otherwise loaded and stored in pieces)
    typedef float quad __attribute__((ext_vector_type(4)));
    const quad *r = (const quad *)(tri + 3 * (first + i));
    const quad t0 = r[0], t1 = r[1], t2 = r[2];   // v0.xyz U.x | U.yz V.xy | V.z n.xyz
    quad *l = (quad *)(light + 4 * (size_t)k);
    l[0] = t0, l[1] = t1, l[2] = t2;
    *(float *)&l[3] = rtrl::light_area(t0.w, t1.x, t1.y, t1.z, t1.w, t2.x);
}

// One level of the light tree: the nodes ids[0 .. n), one thread per node (light_node is in build
// order, so a level is a list of ids, LightPlan::node_by_depth).  A light record is four quads; the
// rest is rt_refit_level_kernel's: a leaf folds its lights' boxes in order, an internal node reads
// its two children (adjacent records), six words are written and a and b never are.
__global__ void __launch_bounds__(256) rt_refit_light_level_kernel(const float4 *__restrict__ light, float4 *node,
                                                                   const uint32_t *__restrict__ ids, unsigned n) {
    const unsigned k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t id = ids[k];
    const float4 q1 = node[2 * id + 1];
    const uint32_t a = __float_as_uint(q1.z), b = __float_as_uint(q1.w);
    rtrf::Box bx;
    if (rtrf::is_leaf(b)) {
        bx = rtrf::empty_box();
        const uint32_t cnt = b >> 2;
        for (uint32_t t = 0; t < cnt; ++t) {
            const float4 *r = light + 4 * (size_t)(a + t);
            const float4 t0 = r[0], t1 = r[1];
            const float t2x = r[2].x;
            rtrf::grow_box(bx, rtrf::tri_box(t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2x));
        }
    } else {
        const float4 l0 = node[2 * (size_t)a], l1 = node[2 * (size_t)a + 1];
        const float4 r0 = node[2 * (size_t)a + 2], r1 = node[2 * (size_t)a + 3];
        const float lw[6] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y}, rw[6] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y};
        bx = rtrf::pair_box(lw, rw);
    }
    node[2 * id] = make_float4(bx.lo[0], bx.lo[1], bx.lo[2], bx.hi[0]);
    *(float2 *)&node[2 * id + 1] = make_float2(bx.hi[1], bx.hi[2]);
}

namespace {

// The writable views of a device copy's triangle, node and light arrays (the blob's offsets).
struct RefitArrays {
    float4 *tri, *attr, *tan, *node, *light, *lnode;
};
RefitArrays refit_arrays(rt_scene *s, rt_device_scene *d) {
    const rt_device_blob &b = *s->blob;
    uint8_t *base = (uint8_t *)d->buf;
    return {(float4 *)(base + b.o_tri),  (float4 *)(base + b.o_attr),  (float4 *)(base + b.o_tan),
            (float4 *)(base + b.o_node), (float4 *)(base + b.o_light), (float4 *)(base + b.o_lnode)};
}

// Movable lights: light_of_tri (n_tris words) and then the light node ids sorted by depth
// (n_light_nodes words) in a small allocation of the device copy, outside the blob; made by the
// copy's first update after the opt-in.  The current device is d's.
int relight_ensure(rt_scene *s, rt_device_scene *d) {
    if (d->relight_buf) return RT_OK;
    const rtrp::LightPlan &lp = *s->light_plan;
    const size_t nt = lp.light_of_tri.size(), nn = lp.node_by_depth.size();
    HIP_TRY(hipMalloc(&d->relight_buf, (nt + nn + 1) * sizeof(uint32_t)));
    uint32_t *p = (uint32_t *)d->relight_buf;
    if (nt) HIP_TRY(hipMemcpy(p, lp.light_of_tri.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (nn) HIP_TRY(hipMemcpy(p + nt, lp.node_by_depth.data(), nn * sizeof(uint32_t), hipMemcpyHostToDevice));
    return RT_OK;
}

// Scatter, then the refit's launches (one per level), on `stream`; the current device is d's.  The
// sources are device pointers (16-byte aligned); d_attr and d_tan may be NULL (kept).  `lights`: the
// range holds a light's triangle; then the light scatter and one launch per level of the light tree
// follow (a range without one launches none of them).
int refit_levels_enqueue(rt_scene *s, rt_device_scene *d, uint32_t first, uint32_t count, bool lights, hipStream_t stream);

int refit_enqueue(rt_scene *s, rt_device_scene *d, uint32_t first, uint32_t count, const float *d_tri, const float *d_attr,
                  const float *d_tan, bool lights, hipStream_t stream) {
    if (s->light_plan)
        if (int rc = relight_ensure(s, d)) return rc;
    const RefitArrays A = refit_arrays(s, d);
    const long long quads = (long long)count * (d_attr ? 4 : 3);
    hipLaunchKernelGGL(rt_tris_scatter_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, A.tri, A.attr, A.tan,
                       (const float4 *)d_tri, (const float4 *)d_attr, (const float4 *)d_tan, (long long)first, (long long)count);
    HIP_TRY(hipGetLastError());
    return refit_levels_enqueue(s, d, first, count, lights, stream);
}

// What follows new triangle records in a device copy's arrays, however they got there (the scatter
// above, or the pose kernel of rt_pose_device.h): the refit's launches, and with `lights` the light
// scatter over [first, first + count) and the light tree's launches (relight_ensure has run).
int refit_levels_enqueue(rt_scene *s, rt_device_scene *d, uint32_t first, uint32_t count, bool lights, hipStream_t stream) {
    const rtrp::Plan &plan = rt_scene_refit_plan(s);
    const RefitArrays A = refit_arrays(s, d);
    for (size_t l = plan.levels(); l-- > 0;) {
        const unsigned id0 = plan.level_first[l], n = plan.level_first[l + 1] - id0;
        hipLaunchKernelGGL(rt_refit_level_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const float4 *)A.tri, A.node,
                           id0, n);
        HIP_TRY(hipGetLastError());
    }
    if (lights) {
        const rtrp::LightPlan &lp = *s->light_plan;
        const uint32_t *light_of_tri = (const uint32_t *)d->relight_buf, *ids = light_of_tri + lp.light_of_tri.size();
        hipLaunchKernelGGL(rt_lights_scatter_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, (const float4 *)A.tri, A.light,
                           light_of_tri, (long long)first, (long long)count);
        HIP_TRY(hipGetLastError());
        for (size_t l = lp.levels(); l-- > 0;) {
            const unsigned i0 = lp.level_first[l], n = lp.level_first[l + 1] - i0;
            hipLaunchKernelGGL(rt_refit_light_level_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const float4 *)A.light,
                               A.lnode, ids + i0, n);
            HIP_TRY(hipGetLastError());
        }
    }
    return RT_OK;
}

// The host light arrays into the cached image (both are small: whole arrays).
void relight_patch_image(rt_scene *s) {
    rt_device_blob &b = *s->blob;
    if (!s->light.empty()) std::memcpy(b.bytes.data() + b.o_light, s->light.data(), s->light.size() * sizeof(float));
    if (!s->light_node.empty()) std::memcpy(b.bytes.data() + b.o_lnode, s->light_node.data(), s->light_node.size() * sizeof(float));
}

// The first six words of every node record of the device numbering (`bfs`, 8 words per node) into
// the host mirror's records (build order) and the cached image's.
void refit_adopt_nodes(rt_scene *s, const float *bfs) {
    const rtrp::Plan &plan = rt_scene_refit_plan(s);
    float *img = (float *)(s->blob->bytes.data() + s->blob->o_node);
    for (size_t k = 0; k < plan.build_of_bfs.size(); ++k) {
        std::memcpy(&s->node[8 * (size_t)plan.build_of_bfs[k]], bfs + 8 * k, 6 * sizeof(float));
        std::memcpy(img + 8 * k, bfs + 8 * k, 6 * sizeof(float));
    }
}

// The image's boxes: the host's, in the device numbering (what the device kernels give too).
void refit_patch_image_nodes(rt_scene *s) {
    const rtrp::Plan &plan = rt_scene_refit_plan(s);
    float *img = (float *)(s->blob->bytes.data() + s->blob->o_node);
    for (size_t k = 0; k < plan.build_of_bfs.size(); ++k)
        std::memcpy(img + 8 * k, &s->node[8 * (size_t)plan.build_of_bfs[k]], 6 * sizeof(float));
}

// The host arrays' triangle range into the cached image.
void refit_patch_image(rt_scene *s, uint32_t first, uint32_t count) {
    rt_device_blob &b = *s->blob;
    std::memcpy(b.bytes.data() + b.o_tri + 48 * (size_t)first, &s->tri[12 * (size_t)first], 48 * (size_t)count);
    std::memcpy(b.bytes.data() + b.o_attr + 64 * (size_t)first, &s->tri_attr[16 * (size_t)first], 64 * (size_t)count);
    std::memcpy(b.bytes.data() + b.o_tan + 48 * (size_t)first, &s->tri_tan[12 * (size_t)first], 48 * (size_t)count);
}

}  // namespace

// rt_scene_update_tris' device half (rt_scene.h): the host arrays already hold the new records and
// the host refit's boxes.
int rt_device_scene_update_tris(rt_scene *s, uint32_t first, uint32_t count, bool attr, bool tan, bool lights) {
    if (!s->blob) return RT_OK;   // on no device yet: the image is built from the host arrays when one is needed
    refit_patch_image(s, first, count);
    if (lights) relight_patch_image(s);
    refit_patch_image_nodes(s);
    const size_t bt = 48 * (size_t)count, ba = attr ? 64 * (size_t)count : 0, bn = tan ? 48 * (size_t)count : 0;
    for (rt_device_scene *d : s->dev) {
        if (!d) continue;
        DeviceGuard guard(d->device);
        if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "rt_scene_update_tris: hipSetDevice failed");
        HIP_TRY(grow(&d->refit_stage, &d->refit_stage_bytes, bt + ba + bn));
        uint8_t *st = (uint8_t *)d->refit_stage;
        HIP_TRY(hipMemcpy(st, &s->tri[12 * (size_t)first], bt, hipMemcpyHostToDevice));
        if (attr) HIP_TRY(hipMemcpy(st + bt, &s->tri_attr[16 * (size_t)first], ba, hipMemcpyHostToDevice));
        if (tan) HIP_TRY(hipMemcpy(st + bt + ba, &s->tri_tan[12 * (size_t)first], bn, hipMemcpyHostToDevice));
        if (int rc = refit_enqueue(s, d, first, count, (const float *)st, attr ? (const float *)(st + bt) : nullptr,
                                   tan ? (const float *)(st + bt + ba) : nullptr, lights, nullptr))
            return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return RT_OK;
}

extern "C" {

int rt_scene_update_tris_device(rt_scene *s, int32_t device, uint32_t first, uint32_t count, const float *d_tri,
                                const float *d_tri_attr, const float *d_tri_tan, void *stream) {
    const char *who = "rt_scene_update_tris_device";
    if (int rc = rt_update_tris_check(s, who, first, count, d_tri)) return rc;
    if (device < 0 || device >= kRtMaxDevices || !s->dev[device])
        return rt_fail(RT_ERR_ARG, std::string(who) + ": the scene is not uploaded to device " + std::to_string(device));
    for (int k = 0; k < kRtMaxDevices; ++k)
        if (k != device && s->dev[k])
            return rt_fail(RT_ERR_ARG, std::string(who) + ": the scene is also on device " + std::to_string(k) +
                                           " (the device entry updates one copy; use rt_scene_update_tris)");
    for (const float *p : {d_tri, d_tri_attr, d_tri_tan})
        if ((uintptr_t)p & 15u) return rt_fail(RT_ERR_ARG, std::string(who) + ": device pointers must be 16-byte aligned");
    if (count == 0) return RT_OK;
    rt_device_scene *d = s->dev[device];
    DeviceGuard guard(device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, std::string(who) + ": hipSetDevice failed");
    hipStream_t q = (hipStream_t)stream;
    const size_t nn = s->node.size() / 8;
    std::vector<float> bfs(8 * nn);
    ++s->view_epoch;
    ++s->geom_epoch;
    const bool lights = s->light_plan && s->light_plan->touches(first, count);
    if (int rc = refit_enqueue(s, d, first, count, d_tri, d_tri_attr, d_tri_tan, lights, q)) return rc;
    // the host mirror and the cached image follow the device: the changed range and every box
    const RefitArrays A = refit_arrays(s, d);
    HIP_TRY(hipMemcpyAsync(&s->tri[12 * (size_t)first], (const float *)A.tri + 12 * (size_t)first, 48 * (size_t)count,
                           hipMemcpyDeviceToHost, q));
    if (d_tri_attr)
        HIP_TRY(hipMemcpyAsync(&s->tri_attr[16 * (size_t)first], (const float *)A.attr + 16 * (size_t)first, 64 * (size_t)count,
                               hipMemcpyDeviceToHost, q));
    if (d_tri_tan)
        HIP_TRY(hipMemcpyAsync(&s->tri_tan[12 * (size_t)first], (const float *)A.tan + 12 * (size_t)first, 48 * (size_t)count,
                               hipMemcpyDeviceToHost, q));
    HIP_TRY(hipMemcpyAsync(bfs.data(), A.node, bfs.size() * sizeof(float), hipMemcpyDeviceToHost, q));
    if (lights) {   // the light arrays follow the device too (both are small: whole arrays)
        if (!s->light.empty())
            HIP_TRY(hipMemcpyAsync(s->light.data(), A.light, s->light.size() * sizeof(float), hipMemcpyDeviceToHost, q));
        if (!s->light_node.empty())
            HIP_TRY(hipMemcpyAsync(s->light_node.data(), A.lnode, s->light_node.size() * sizeof(float), hipMemcpyDeviceToHost, q));
    }
    HIP_TRY(hipStreamSynchronize(q));
    refit_patch_image(s, first, count);
    refit_adopt_nodes(s, bfs.data());
    if (lights) relight_patch_image(s);
    return RT_OK;
}

int rt_scene_read_device_lights(rt_scene *s, int32_t device, float *light, float *light_node) {
    const char *who = "rt_scene_read_device_lights";
    if (!s) return rt_fail(RT_ERR_ARG, std::string(who) + ": NULL scene");
    if (device < 0 || device >= kRtMaxDevices || !s->dev[device])
        return rt_fail(RT_ERR_ARG, std::string(who) + ": the scene is not uploaded to device " + std::to_string(device));
    rt_device_scene *d = s->dev[device];
    DeviceGuard guard(device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, std::string(who) + ": hipSetDevice failed");
    const RefitArrays A = refit_arrays(s, d);
    if (light && !s->light.empty()) HIP_TRY(hipMemcpy(light, A.light, s->light.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (light_node && !s->light_node.empty())
        HIP_TRY(hipMemcpy(light_node, A.lnode, s->light_node.size() * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_scene_read_device(rt_scene *s, int32_t device, float *tri, float *tri_attr, float *tri_tan, float *node) {
    const char *who = "rt_scene_read_device";
    if (!s) return rt_fail(RT_ERR_ARG, std::string(who) + ": NULL scene");
    if (device < 0 || device >= kRtMaxDevices || !s->dev[device])
        return rt_fail(RT_ERR_ARG, std::string(who) + ": the scene is not uploaded to device " + std::to_string(device));
    rt_device_scene *d = s->dev[device];
    DeviceGuard guard(device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, std::string(who) + ": hipSetDevice failed");
    const RefitArrays A = refit_arrays(s, d);
    const size_t nt = s->tri.size() / 12, nn = s->node.size() / 8;
    if (tri && nt) HIP_TRY(hipMemcpy(tri, A.tri, 48 * nt, hipMemcpyDeviceToHost));
    if (tri_attr && nt) HIP_TRY(hipMemcpy(tri_attr, A.attr, 64 * nt, hipMemcpyDeviceToHost));
    if (tri_tan && nt) HIP_TRY(hipMemcpy(tri_tan, A.tan, 48 * nt, hipMemcpyDeviceToHost));
    if (node && nn) {
        const rtrp::Plan &plan = rt_scene_refit_plan(s);
        std::vector<float> bfs(8 * nn);
        HIP_TRY(hipMemcpy(bfs.data(), A.node, bfs.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < nn; ++k) {   // back to build order: the record's place and an internal node's child id
            float *o = node + 8 * (size_t)plan.build_of_bfs[k];
            std::memcpy(o, &bfs[8 * k], 8 * sizeof(float));
            uint32_t a, b;
            std::memcpy(&a, &bfs[8 * k + 6], 4);
            std::memcpy(&b, &bfs[8 * k + 7], 4);
            if (!rtrf::is_leaf(b)) {
                const uint32_t ba = plan.build_of_bfs[a];
                std::memcpy(o + 6, &ba, 4);
            }
        }
    }
    return RT_OK;
}

}  // extern "C"
