// rt_pose_device.h — posable meshes on the device: the rest records of a scene copy and the kernel
// that recomputes a posed mesh's triangle records from them (include/rt_hw.h rt_scene_pose_meshes;
// the rule is rt_pose.h).  Included by rt_device.hip after rt_refit_device.h: it uses HIP_TRY,
// DeviceGuard, grow, the writable views and the refit launches from there.  The render kernels and
// DevScene are untouched.
//
// One call, per device copy: the table goes up (one copy), rt_pose_nt_kernel rewrites the posed
// meshes' mesh_nt, rt_pose_kernel rewrites their triangles, then the refit's launches (and the light
// launches) of rt_refit_device.h follow on the same stream.  The kernel boundary is the only
// ordering: no atomics, no LDS, no flags.  No record crosses the bus in either direction.

// The table buffer: slot_of_mesh (n_meshes x int32: the mesh's place in the call, or -1), then ids
// (n x uint32: the mesh of each place), padded to 16 bytes, then per place M and NT (32 doubles).
namespace {
struct PoseTableLayout {
    size_t o_ids, o_tab, bytes;
};
PoseTableLayout pose_table_layout(size_t n_meshes, size_t n) {
    PoseTableLayout L;
    L.o_ids = 4 * n_meshes;
    L.o_tab = (L.o_ids + 4 * n + 15) & ~(size_t)15;
    L.bytes = L.o_tab + 256 * n;
    return L;
}
}  // namespace

// mesh_nt of the posed meshes: one thread per (place, word).
__global__ void __launch_bounds__(256) rt_pose_nt_kernel(double *__restrict__ mesh_nt, const uint32_t *__restrict__ ids,
                                                         const double *__restrict__ table, unsigned n) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 16u * n) return;
    const unsigned slot = i >> 4, w = i & 15u;
    mesh_nt[16 * (size_t)ids[slot] + w] = table[32 * (size_t)slot + 16 + w];
}

// Triangles [first, first + count), one thread each.  The thread reads the last quad of its tri_attr
// record (word 15: the mesh) and returns if the mesh has no place in the table; otherwise it reads its
// rest record (five quads, 18 words used), computes the record as rt_pose.h says (fp64 products and
// adds for the transforms, fp32 for the differences, cross, length and normal) and writes tri as three
// quads and words 0..8 of tri_attr as two quads and one word.  Words 9..15 and tri_tan are never written.
__global__ void __launch_bounds__(256) rt_pose_kernel(float4 *tri, float4 *attr, const float4 *__restrict__ rest,
                                                      const int32_t *__restrict__ slot_of_mesh,
                                                      const double *__restrict__ table, unsigned n_meshes, long long first,
                                                      long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t k = (size_t)(first + i);
    // (native vectors: a float4 whose members are used one by one is otherwise loaded and stored in pieces)
    typedef float quad __attribute__((ext_vector_type(4)));
    quad *a = (quad *)(attr + 4 * k);
    const uint32_t mesh = __float_as_uint(a[3].w);
    if (mesh >= n_meshes) return;
    const int32_t slot = slot_of_mesh[mesh];
    if (slot < 0) return;
    const double *M = table + 32 * (size_t)slot;
    const quad *r = (const quad *)(rest + 5 * k);
    const quad r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3], r4 = r[4];
    const float rw[rtps::kRestWords] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x,
                                        r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w, r4.x, r4.y};
    float t[12], n[9];
    rtps::pose_record(M, M + 16, rw, t, n);
    quad *o = (quad *)(tri + 3 * k);
    o[0] = quad{t[0], t[1], t[2], t[3]};
    o[1] = quad{t[4], t[5], t[6], t[7]};
    o[2] = quad{t[8], t[9], t[10], t[11]};
    a[0] = quad{n[0], n[1], n[2], n[3]};
    a[1] = quad{n[4], n[5], n[6], n[7]};
    *(float *)&a[2] = n[8];
}

namespace {

// The scene's rest records onto device copy d (the current device is d's): 18 words padded to 20.
int pose_rest_upload(rt_scene *s, rt_device_scene *d) {
    if (d->pose_rest) return RT_OK;
    const size_t nt = s->tri.size() / 12;
    std::vector<float> padded(rtps::kRestDevWords * nt, 0.f);
    for (size_t k = 0; k < nt; ++k)
        std::memcpy(&padded[rtps::kRestDevWords * k], &s->rest[rtps::kRestWords * k], rtps::kRestWords * sizeof(float));
    HIP_TRY(hipMalloc(&d->pose_rest, padded.size() * sizeof(float) + 256));
    if (nt) HIP_TRY(hipMemcpy(d->pose_rest, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice));
    return RT_OK;
}

}  // namespace

int rt_device_scene_enable_poses(rt_scene *s) {
    for (rt_device_scene *d : s->dev) {
        if (!d) continue;
        DeviceGuard guard(d->device);
        if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "rt_scene_enable_poses: hipSetDevice failed");
        if (int rc = pose_rest_upload(s, d)) return rc;
    }
    return RT_OK;
}

// rt_scene_pose_meshes' device half (rt_scene.h): the host arrays already hold the posed records, the
// new mesh_nt, the refit's boxes and, with `lights`, the light arrays.
int rt_device_scene_pose(rt_scene *s, uint32_t n, const uint32_t *mesh, const double *table, uint32_t first, uint32_t count,
                         bool lights) {
    if (!s->blob) return RT_OK;   // on no device yet: the image is built from the host arrays when one is needed
    rt_device_blob &b = *s->blob;
    if (count) {
        refit_patch_image(s, first, count);
        refit_patch_image_nodes(s);
    }
    if (lights) relight_patch_image(s);
    for (uint32_t k = 0; k < n; ++k)
        std::memcpy(b.bytes.data() + b.o_nt + 128 * (size_t)mesh[k], table + 32 * (size_t)k + 16, 128);
    const size_t nm = s->mesh_f.size() / 12;
    const PoseTableLayout L = pose_table_layout(nm, n);
    std::vector<uint8_t> stage(L.bytes, 0);
    {
        int32_t *slot = (int32_t *)stage.data();
        for (size_t m = 0; m < nm; ++m) slot[m] = -1;
        for (uint32_t k = 0; k < n; ++k) slot[mesh[k]] = (int32_t)k;
        std::memcpy(stage.data() + L.o_ids, mesh, 4 * (size_t)n);
        std::memcpy(stage.data() + L.o_tab, table, 256 * (size_t)n);
    }
    for (rt_device_scene *d : s->dev) {
        if (!d) continue;
        DeviceGuard guard(d->device);
        if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "rt_scene_pose_meshes: hipSetDevice failed");
        if (int rc = pose_rest_upload(s, d)) return rc;
        if (s->light_plan)
            if (int rc = relight_ensure(s, d)) return rc;
        HIP_TRY(grow(&d->pose_table, &d->pose_table_bytes, L.bytes));
        HIP_TRY(hipMemcpy(d->pose_table, stage.data(), L.bytes, hipMemcpyHostToDevice));
        const uint8_t *tb = (const uint8_t *)d->pose_table;
        const RefitArrays A = refit_arrays(s, d);
        hipLaunchKernelGGL(rt_pose_nt_kernel, dim3((16 * n + 255) / 256), dim3(256), 0, nullptr,
                           (double *)((uint8_t *)d->buf + b.o_nt), (const uint32_t *)(tb + L.o_ids), (const double *)(tb + L.o_tab), n);
        HIP_TRY(hipGetLastError());
        if (count) {
            hipLaunchKernelGGL(rt_pose_kernel, dim3((count + 255) / 256), dim3(256), 0, nullptr, A.tri, A.attr,
                               (const float4 *)d->pose_rest, (const int32_t *)tb, (const double *)(tb + L.o_tab), (unsigned)nm,
                               (long long)first, (long long)count);
            HIP_TRY(hipGetLastError());
            if (int rc = refit_levels_enqueue(s, d, first, count, lights, nullptr)) return rc;
        }
        HIP_TRY(hipStreamSynchronize(nullptr));
    }
    return RT_OK;
}
