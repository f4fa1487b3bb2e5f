// rt_motion_device.h — the device half of the per-pixel motion records: the kernel, its launch
// function and rt_motion_device (include/rt_hw.h).  Included by rt_device.hip after
// rt_denoise_device.h (dn_lane) and before rt_temporal_device.h, whose history launches it, so the
// build stays one translation unit.  The per-pixel text is rt_motion.h.

// One thread per pixel over the denoiser's tiles (dn_lane: kDnTileW x kDnTileH pixels per 256-thread
// block), so neighbouring pixels, which mostly see the same or adjacent triangles, gather the same
// lines of the two triangle arrays.  Per pixel: quads 0, 1 and 3 of its record, three quads of its
// triangle from each array (none for a miss), two quads stored.  Every access is a whole 16-byte
// quad; no LDS, no atomics.  The id is tested against n_tris before it indexes (rt_motion.h).
__global__ void __launch_bounds__(256) rt_motion_kernel(const rtdn::Q *__restrict__ g, const rtdn::Q *__restrict__ tri,
                                                         const rtdn::Q *__restrict__ tri_prev, unsigned n_tris, int W, int H,
                                                         int tiles_x, rtdn::Q *__restrict__ out) {
    const DnLane l = dn_lane(tiles_x);
    if (l.x >= W || l.y >= H) return;
    const long long p = (long long)l.y * W + l.x;
    const rtmo::Motion m = rtmo::carry_pixel(g[4 * p], g[4 * p + 1], g[4 * p + 3], tri, tri_prev, n_tris);
    out[2 * p] = m.p;
    out[2 * p + 1] = m.n;
}

namespace {

// The records of a W x H frame on the current device.
int motion_launch(const float *d_g, int W, int H, const float *d_tri, const float *d_tri_prev, uint32_t n_tris, float *d_out,
                  hipStream_t stream) {
    const int tiles_x = (W + kDnTileW - 1) / kDnTileW;
    const dim3 tiles((unsigned)((long long)tiles_x * ((H + kDnTileH - 1) / kDnTileH)));
    hipLaunchKernelGGL(rt_motion_kernel, tiles, dim3(256), 0, stream, (const rtdn::Q *)d_g, (const rtdn::Q *)d_tri,
                       (const rtdn::Q *)d_tri_prev, n_tris, W, H, tiles_x, (rtdn::Q *)d_out);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

bool quad_aligned(const void *p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int rt_motion_device(const float *d_gbuffer, int32_t width, int32_t height, const float *d_tri, const float *d_tri_prev,
                                uint32_t n_tris, float *d_out_motion, void *stream) {
    if (int rc = rt_motion_check("rt_motion_device", d_gbuffer, width, height, d_tri, d_tri_prev, n_tris, d_out_motion)) return rc;
    if (!quad_aligned(d_gbuffer) || !quad_aligned(d_tri) || !quad_aligned(d_tri_prev) || !quad_aligned(d_out_motion))
        return rt_fail(RT_ERR_ARG, "rt_motion_device: device pointers must be 16-byte aligned");
    return motion_launch(d_gbuffer, width, height, d_tri, d_tri_prev, n_tris, d_out_motion, (hipStream_t)stream);
}
