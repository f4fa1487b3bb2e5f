// rt_temporal_device.h — the device half of the reprojected temporal history: the kernel, its launch
// function, rt_temporal_device and the rt_history_* entries of include/rt_hw.h.  Included by
// rt_device.hip after rt_denoise_device.h (dn_lane, gbuffer_launch) so the build stays one
// translation unit.  The per-pixel text is rt_temporal.h.

// One thread per pixel over the denoiser's tiles (dn_lane: kDnTileW x kDnTileH pixels per 256-thread
// block), so the four taps of neighbouring pixels fall into the same few rows of the previous frame
// and share cache lines (16 x 16 tiles measured 6% slower on the 1080p headline frame, DESIGN.md
// §5.18).  Every history and record access is a whole 16-byte quad (of a previous
// record only quads 0, 2 and 3 are read); the three history planes, the mean and the variance are
// plain vector stores.  No LDS, no atomics.  prev_h == nullptr: a first frame.
// kMotion: the pixel's two motion quads (rt_motion.h) are read as well and give the look-up its
// centre; without it `motion` is not read and the code is the one this kernel had before it took
// the argument (DESIGN.md §5.24 has the comparison of the two listings).
template <bool kMotion>
__global__ void __launch_bounds__(256) rt_temporal_kernel(const float *__restrict__ sums, const int32_t *__restrict__ counts, int spp,
                                                           const rtdn::Q *__restrict__ g, const rtdn::Q *__restrict__ prev_h,
                                                           const rtdn::Q *__restrict__ prev_g, rttm::Camera cam, rttm::Params tp,
                                                           int W, int H, int tiles_x, rtdn::Q *__restrict__ hist_out,
                                                           float *__restrict__ out_mean, float *__restrict__ out_var,
                                                           const rtdn::Q *__restrict__ motion) {
    const DnLane l = dn_lane(tiles_x);
    if (l.x >= W || l.y >= H) return;
    const long long n = (long long)W * H, p = (long long)l.y * W + l.x;
    const rtdn::Q rec[4] = {g[4 * p], g[4 * p + 1], g[4 * p + 2], g[4 * p + 3]};
    const float S[3] = {sums[3 * p], sums[3 * p + 1], sums[3 * p + 2]};
    rttm::Pixel r;
    if constexpr (kMotion) {
        const rtdn::Q mo[2] = {motion[2 * p], motion[2 * p + 1]};
        r = rttm::temporal_pixel(rttm::PlainSrc{prev_h, prev_g, W, n}, prev_h != nullptr, cam, S, counts ? counts[p] : spp, rec, W, H,
                                 tp, mo);
    } else {
        r = rttm::temporal_pixel(rttm::PlainSrc{prev_h, prev_g, W, n}, prev_h != nullptr, cam, S, counts ? counts[p] : spp, rec, W, H,
                                 tp);
    }
#pragma unroll
    for (int k = 0; k < rttm::kHistoryQuads; ++k) hist_out[k * n + p] = r.h[k];
    if (out_mean) {
        out_mean[3 * p] = r.mean[0];
        out_mean[3 * p + 1] = r.mean[1];
        out_mean[3 * p + 2] = r.mean[2];
    }
    if (out_var) out_var[p] = r.variance;
}

namespace {

// The step on the current device (d_hist_prev == nullptr: a first frame; d_motion == nullptr: the
// kernel without motion records).
int temporal_launch(const float *d_sums, const int32_t *d_counts, int spp, int W, int H, const float *d_g, const rt_camera *cam_prev,
                    const float *d_g_prev, const float *d_hist_prev, const rttm::Params &tp, float *d_hist_out, float *d_out_mean,
                    float *d_out_var, hipStream_t stream, const float *d_motion = nullptr) {
    rttm::Camera cam{};
    if (d_hist_prev) std::memcpy(&cam, cam_prev, sizeof cam);
    const int tiles_x = (W + kDnTileW - 1) / kDnTileW;
    const dim3 tiles((unsigned)((long long)tiles_x * ((H + kDnTileH - 1) / kDnTileH)));
    if (d_motion)
        hipLaunchKernelGGL(rt_temporal_kernel<true>, tiles, dim3(256), 0, stream, d_sums, d_counts, spp, (const rtdn::Q *)d_g,
                           (const rtdn::Q *)d_hist_prev, (const rtdn::Q *)(d_hist_prev ? d_g_prev : nullptr), cam, tp, W, H, tiles_x,
                           (rtdn::Q *)d_hist_out, d_out_mean, d_out_var, (const rtdn::Q *)d_motion);
    else
        hipLaunchKernelGGL(rt_temporal_kernel<false>, tiles, dim3(256), 0, stream, d_sums, d_counts, spp, (const rtdn::Q *)d_g,
                           (const rtdn::Q *)d_hist_prev, (const rtdn::Q *)(d_hist_prev ? d_g_prev : nullptr), cam, tp, W, H, tiles_x,
                           (rtdn::Q *)d_hist_out, d_out_mean, d_out_var, (const rtdn::Q *)nullptr);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

}  // namespace

// Two histories and two G-buffers of a scene's frame on one device; `cur` is the slot the next push
// writes, the other one holds the last push's frame once has_prev is set.
struct rt_history {
    rt_scene *scene = nullptr;
    int device = 0, W = 0, H = 0;
    long long n = 0;
    ShardGeom geom{};   // the whole frame
    float *hist[2] = {nullptr, nullptr};
    float4 *gbuf[2] = {nullptr, nullptr};
    int cur = 0;
    bool has_prev = false;
    rt_camera cam_prev{};
    hipStream_t stream = nullptr;   // the last push's (host reads wait for it)
    // motion records (rt_history_enable_motion): the scene's triangles as they stood at the last push,
    // the geometry counter they were copied at, and the last push's records
    bool motion_on = false, has_snapshot = false, motion_valid = false;
    uint32_t geom_seen = 0;
    float *tri_prev = nullptr, *motion = nullptr;
};

extern "C" {

int rt_temporal_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                       const float *d_gbuffer, const rt_camera *cam_prev, const float *d_gbuffer_prev, const float *d_history_prev,
                       const rt_temporal_params *params, float *d_history_out, float *d_out_mean, float *d_out_variance,
                       void *stream) {
    rttm::Params tp;
    if (int rc = rt_temporal_check("rt_temporal_device", d_sums, d_counts, spp, width, height, d_gbuffer, cam_prev, d_gbuffer_prev,
                                   d_history_prev, params, d_history_out, &tp))
        return rc;
    return temporal_launch(d_sums, d_counts, spp, width, height, d_gbuffer, cam_prev, d_gbuffer_prev, d_history_prev, tp,
                           d_history_out, d_out_mean, d_out_variance, (hipStream_t)stream);
}

int rt_temporal_motion_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                              const float *d_gbuffer, const rt_camera *cam_prev, const float *d_gbuffer_prev,
                              const float *d_history_prev, const rt_temporal_params *params, float *d_history_out, float *d_out_mean,
                              float *d_out_variance, const float *d_motion, void *stream) {
    rttm::Params tp;
    if (int rc = rt_temporal_check("rt_temporal_motion_device", d_sums, d_counts, spp, width, height, d_gbuffer, cam_prev,
                                   d_gbuffer_prev, d_history_prev, params, d_history_out, &tp))
        return rc;
    if (d_motion && !d_history_prev) return rt_fail(RT_ERR_ARG, "rt_temporal_motion_device: motion records need a previous history");
    if (!quad_aligned(d_motion)) return rt_fail(RT_ERR_ARG, "rt_temporal_motion_device: device pointers must be 16-byte aligned");
    return temporal_launch(d_sums, d_counts, spp, width, height, d_gbuffer, cam_prev, d_gbuffer_prev, d_history_prev, tp,
                           d_history_out, d_out_mean, d_out_variance, (hipStream_t)stream, d_motion);
}

void rt_history_free(rt_history *h) {
    if (!h) return;
    DeviceGuard guard(h->device);
    for (void *b : {(void *)h->hist[0], (void *)h->hist[1], (void *)h->gbuf[0], (void *)h->gbuf[1], (void *)h->tri_prev, (void *)h->motion})
        if (b) (void)hipFree(b);
    delete h;
}

int rt_history_create(rt_scene *s, int32_t device, rt_history **out) {
    if (!s || !out) return rt_fail(RT_ERR_ARG, "rt_history_create: NULL argument");
    *out = nullptr;
    if (device < 0 || device >= kRtMaxDevices || !s->dev[device])
        return rt_fail(RT_ERR_ARG, "rt_history_create: scene not uploaded to device " + std::to_string(device));
    rt_params p{};
    p.device = device;
    Shard sh;
    if (int rc = shard_of(s, &p, "rt_history_create", sh)) return rc;
    DeviceGuard guard(device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    rt_history *h = new rt_history();
    h->scene = s, h->device = device, h->W = s->width, h->H = s->height, h->n = sh.n_pixels, h->geom = sh.g;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = hipMalloc((void **)&h->hist[i], (size_t)h->n * RT_HISTORY_WORDS * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void **)&h->gbuf[i], (size_t)h->n * RT_GBUFFER_WORDS * sizeof(float));
    }
    if (e != hipSuccess) {
        rt_history_free(h);
        return rt_fail(RT_ERR_DEVICE, std::string("rt_history_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return RT_OK;
}

int rt_history_push(rt_history *h, const float *d_sums, const int32_t *d_counts, int32_t spp, const rt_temporal_params *params,
                    float *d_out_mean, float *d_out_variance, void *stream) {
    if (!h) return rt_fail(RT_ERR_ARG, "rt_history_push: NULL history");
    // every refusal before the first launch: a refused push leaves both slots as they were
    rttm::Params tp;
    const int c = h->cur, o = c ^ 1;
    const float *g_prev = h->has_prev ? (const float *)h->gbuf[o] : nullptr, *h_prev = h->has_prev ? h->hist[o] : nullptr;
    if (int rc = rt_temporal_check("rt_history_push", d_sums, d_counts, spp, h->W, h->H, (const float *)h->gbuf[c], &h->cam_prev,
                                   g_prev, h_prev, params, h->hist[c], &tp))
        return rc;
    rt_device_scene *d = h->scene->dev[h->device];
    if (!d) return rt_fail(RT_ERR_ARG, "rt_history_push: scene not uploaded to device " + std::to_string(h->device));
    DeviceGuard guard(h->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    h->stream = (hipStream_t)stream;
    if (int rc = gbuffer_launch(d, h->geom, h->gbuf[c], h->stream)) return rc;
    // with motion records: the triangles moved since the snapshot was taken (several updates between
    // two pushes are one motion); an unmoved scene runs exactly the launch below
    const bool moved = h->motion_on && h->has_prev && h->has_snapshot && h->geom_seen != h->scene->geom_epoch;
    h->motion_valid = false;
    if (moved) {
        if (int rc = motion_launch((const float *)h->gbuf[c], h->W, h->H, (const float *)d->ds.tri, h->tri_prev, (uint32_t)d->ds.n_tris,
                                   h->motion, h->stream))
            return rc;
        h->motion_valid = true;
    }
    if (int rc = temporal_launch(d_sums, d_counts, spp, h->W, h->H, (const float *)h->gbuf[c], &h->cam_prev, g_prev, h_prev, tp,
                                 h->hist[c], d_out_mean, d_out_variance, h->stream, moved ? h->motion : nullptr))
        return rc;
    if (h->motion_on && (!h->has_snapshot || h->geom_seen != h->scene->geom_epoch)) {
        if (d->ds.n_tris)
            HIP_TRY(hipMemcpyAsync(h->tri_prev, d->ds.tri, (size_t)d->ds.n_tris * 12 * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        h->geom_seen = h->scene->geom_epoch;
        h->has_snapshot = true;
    }
    (void)rt_scene_get_camera(h->scene, &h->cam_prev);
    h->cur = o;
    h->has_prev = true;
    return RT_OK;
}

// rt_history_push and what follows it for a caller that holds host arrays and no HIP (the CLI):
// the sums (and counts) go to the history's device, are pushed, the integrated mean optionally
// passes through one of the two filters at spp = 1 with the history's records (the guided one with
// the step's variance), and is finished to bytes; it waits.
int rt_history_push_frame_u8(rt_history *h, const float *sums, const int32_t *counts, int32_t spp, const rt_temporal_params *tparams,
                             const rt_denoise_params *dparams, const rt_denoise_guided_params *gparams, uint8_t *out_rgb) {
    const std::string who = "rt_history_push_frame_u8";
    if (!h || !sums || !out_rgb) return rt_fail(RT_ERR_ARG, who + ": NULL argument");
    if (dparams && gparams) return rt_fail(RT_ERR_ARG, who + ": two filters given; choose one");
    rtdn::Params dp;
    rtdg::Params gp;
    if (dparams)
        if (int rc = rt_denoise_check(who.c_str(), sums, counts, spp, h->W, h->H, sums, dparams, sums, &dp)) return rc;
    if (gparams)
        if (int rc = rt_denoise_guided_check(who.c_str(), sums, counts, spp, h->W, h->H, sums, gparams, sums, &gp)) return rc;
    DeviceGuard guard(h->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    // one staging allocation: sums, mean, filtered mean, counts, variance, bytes (each part 256-byte aligned)
    const size_t n = (size_t)h->n;
    const size_t o_mean = rtp::align_up(n * 12), o_filt = o_mean + rtp::align_up(n * 12), o_cnt = o_filt + rtp::align_up(n * 12),
                 o_var = o_cnt + rtp::align_up(n * 4), o_rgb = o_var + rtp::align_up(n * 4), total = o_rgb + n * 3;
    uint8_t *buf = nullptr;
    HIP_TRY(hipMalloc((void **)&buf, total));
    int32_t *d_counts = counts ? (int32_t *)(buf + o_cnt) : nullptr;
    float *d_mean = (float *)(buf + o_mean), *d_filt = (float *)(buf + o_filt), *d_var = (float *)(buf + o_var);
    hipError_t e = hipMemcpy(buf, sums, n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess && counts) e = hipMemcpy(d_counts, counts, n * 4, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? RT_OK : rt_fail(RT_ERR_DEVICE, who + " copy: " + hipGetErrorString(e));
    if (rc == RT_OK) rc = rt_history_push(h, (const float *)buf, d_counts, spp, tparams, d_mean, d_var, nullptr);
    const float *d_final = d_mean;
    if (rc == RT_OK && (dparams || gparams)) {
        std::lock_guard<std::mutex> lock(g_dn_mu);
        const float *d_g = rt_history_gbuffer_device(h);
        rc = dparams ? denoise_launch(&g_dn_ws[h->device], &g_dn_ws_bytes[h->device], d_mean, nullptr, 1, h->W, h->H, d_g, dp, d_filt, nullptr)
                     : denoise_guided_launch(&g_dn_ws[h->device], &g_dn_ws_bytes[h->device], d_mean, nullptr, 1, h->W, h->H, d_g, d_var, gp,
                                             d_filt, nullptr, nullptr);
        d_final = d_filt;
    }
    if (rc == RT_OK) rc = rt_tonemap_u8_device(d_final, h->W, h->H, 1, buf + o_rgb, nullptr);
    if (rc == RT_OK) {
        e = hipMemcpy(out_rgb, buf + o_rgb, n * 3, hipMemcpyDeviceToHost);   // (waits for the default stream)
        if (e != hipSuccess) rc = rt_fail(RT_ERR_DEVICE, who + " copy: " + hipGetErrorString(e));
    } else {
        (void)hipDeviceSynchronize();   // (nothing of the staging buffer may be in flight when it is freed)
    }
    (void)hipFree(buf);
    return rc;
}

const float *rt_history_gbuffer_device(rt_history *h) { return h && h->has_prev ? (const float *)h->gbuf[h->cur ^ 1] : nullptr; }

int rt_history_enable_motion(rt_history *h) {
    if (!h) return rt_fail(RT_ERR_ARG, "rt_history_enable_motion: NULL history");
    if (h->has_prev) return rt_fail(RT_ERR_ARG, "rt_history_enable_motion: only before the first push or directly after rt_history_reset");
    if (h->motion_on) return RT_OK;
    rt_device_scene *d = h->scene->dev[h->device];
    if (!d) return rt_fail(RT_ERR_ARG, "rt_history_enable_motion: scene not uploaded to device " + std::to_string(h->device));
    DeviceGuard guard(h->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    float *tri_prev = nullptr, *motion = nullptr;
    const size_t tri_bytes = (size_t)d->ds.n_tris * 12 * sizeof(float);
    hipError_t e = hipMalloc((void **)&tri_prev, tri_bytes ? tri_bytes : 16);
    if (e == hipSuccess) e = hipMalloc((void **)&motion, (size_t)(h->n ? h->n : 1) * RT_MOTION_WORDS * sizeof(float));
    if (e != hipSuccess) {   // the history stays as it was
        if (tri_prev) (void)hipFree(tri_prev);
        return rt_fail(RT_ERR_DEVICE, std::string("rt_history_enable_motion: ") + hipGetErrorString(e));
    }
    h->tri_prev = tri_prev, h->motion = motion, h->motion_on = true, h->has_snapshot = false, h->motion_valid = false;
    return RT_OK;
}

const float *rt_history_motion_device(rt_history *h) { return h && h->has_prev && h->motion_valid ? h->motion : nullptr; }

int rt_history_motion(rt_history *h, float *out) {
    if (!h || !out) return rt_fail(RT_ERR_ARG, "rt_history_motion: NULL argument");
    if (!rt_history_motion_device(h)) return rt_fail(RT_ERR_ARG, "rt_history_motion: the last push ran without motion records");
    DeviceGuard guard(h->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->n) HIP_TRY(hipMemcpy(out, h->motion, (size_t)h->n * RT_MOTION_WORDS * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_history_lengths(rt_history *h, float *out) {
    if (!h || !out) return rt_fail(RT_ERR_ARG, "rt_history_lengths: NULL argument");
    if (!h->has_prev) {
        std::fill(out, out + h->n, 0.f);
        return RT_OK;
    }
    DeviceGuard guard(h->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    HIP_TRY(hipStreamSynchronize(h->stream));
    std::vector<float> plane((size_t)h->n * 4);   // plane 0: (L, N)
    if (h->n) HIP_TRY(hipMemcpy(plane.data(), h->hist[h->cur ^ 1], plane.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (long long p = 0; p < h->n; ++p) out[p] = plane[(size_t)(4 * p + 3)];
    return RT_OK;
}

int rt_history_reset(rt_history *h) {
    if (!h) return rt_fail(RT_ERR_ARG, "rt_history_reset: NULL history");
    h->has_prev = false;   // (the slots' contents are never read before the next push has written one)
    h->has_snapshot = false, h->motion_valid = false;   // (the next push takes a new snapshot of the triangles)
    return RT_OK;
}

}  // extern "C"
