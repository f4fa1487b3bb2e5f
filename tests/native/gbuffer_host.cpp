// gbuffer_host.cpp — TEST ONLY: the first-hit feature record (raytracing-hw_amd/csrc/rt_gbuffer.h
// over rt_path.h) compiled for the host, the way kernel_host.cpp compiles the render kernels'
// source, so its arithmetic can be checked without a GPU and the device kernel against it.  Not
// part of the product.
#include "mega_emu.h"
#include "../../raytracing-hw_amd/csrc/rt_gbuffer.h"

using namespace emu;

// The records of a (rank, world, row_block) shard in shard-pixel order (16 floats each), and the
// rays they were cast with: origin and the direction before Ray::Ray normalises it (what
// BVH-level checkers take).  *ray_mismatch counts pixels whose exported ray, put through make_ray,
// is not bit for bit the ray gbuffer_pixel cast (0: the exported rays are the cast ones).
// Returns the shard's pixel count.
extern "C" long long gh_gbuffer(const rt_scene_view *v, int rank, int world, int row_block, float *rec, float *org,
                                float *dir, long long *ray_mismatch) {
    const rtd::DevScene sc = make(v);
    const Shard sh = shard_of(v, rank, world, row_block);
    long long bad = 0;
    for (long long p = 0; p < sh.n; ++p) {
        int px, py;
        rtd::shard_xy(sh.g, p, px, py);
        rtd::Ray cast;
        const rtd::GRecord g = rtd::gbuffer_pixel(sc, px, py, &cast);
        std::memcpy(rec + 16 * p, g.q, 64);
        // Camera::cast_in_pixel (camera.cpp:49-62) at the pixel centre, up to the normalisation
        rtv::V3 t;
        t.x = (2.f * ((float)px + 0.5f + 0.f) / sc.fwidth - 1) * sc.tan_fov[0];
        t.y = -(2.f * ((float)py + 0.5f + 0.f) / sc.fheight - 1) * sc.tan_fov[1];
        t.z = 1;
        rtv::V3 d{0.f, 0.f, 0.f};
        const float tv[3] = {t.x, t.y, t.z};
        for (int i = 0; i < 3; ++i)
            d = rtv::add(d, rtv::mul(rtv::V3{sc.cam_axes[3 * i], sc.cam_axes[3 * i + 1], sc.cam_axes[3 * i + 2]}, tv[i]));
        const rtd::Ray again = rtd::make_ray(rtv::V3{sc.cam_pos[0], sc.cam_pos[1], sc.cam_pos[2]}, d);
        bad += std::memcmp(&again.o, &cast.o, sizeof again.o) != 0 || std::memcmp(&again.d, &cast.d, sizeof again.d) != 0;
        org[3 * p] = sc.cam_pos[0]; org[3 * p + 1] = sc.cam_pos[1]; org[3 * p + 2] = sc.cam_pos[2];
        dir[3 * p] = d.x; dir[3 * p + 1] = d.y; dir[3 * p + 2] = d.z;
    }
    if (ray_mismatch) *ray_mismatch = bad;
    return sh.n;
}
