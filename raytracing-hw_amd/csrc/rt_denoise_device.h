// rt_denoise_device.h — the device half of the feature buffer and the frame denoiser: the kernels,
// their launch functions, the per-device scratch cache and the entries of include/rt_hw.h that
// call them (rt_gbuffer*, rt_denoise_*, rt_variance_from_moments_device).  Included by
// rt_device.hip after the scene, grow, HIP_TRY, shard_of, ensure_device_scene and the tonemap
// entries, which it uses, so the build stays one translation unit.  The per-pixel text is
// rt_gbuffer.h, rt_denoise.h and rt_denoise_guided.h; the accumulator's frames are
// rt_accum_device.h's.

// rt_gbuffer* (include/rt_hw.h, rt_gbuffer.h): one lane per shard pixel, in the shape of
// rt_rays_kernel; the pixel-centre ray, its closest hit and the hit's attributes, written as four
// 16-byte stores per record.
__global__ void __launch_bounds__(256) rt_gbuffer_kernel(DevScene sc, ShardGeom g, float4 *out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.n_pixels) return;
    int px, py;
    rtd::shard_xy(g, p, px, py);
    const rtd::GRecord r = rtd::gbuffer_pixel(sc, px, py);
#pragma unroll
    for (int k = 0; k < rtd::kGbufferQuads; ++k) out[rtd::kGbufferQuads * p + k] = r.q[k];
}

// rt_denoise_device and rt_denoise_guided_device (include/rt_hw.h, rt_denoise.h,
// rt_denoise_guided.h): prepare packs what a tap needs into three 16-byte words per pixel, (L, kind),
// (N, t) and (P, 0); each level reads one (L, kind) buffer and writes the other; resolve
// remodulates.  In the variance-guided mode the variance is a float of its own per pixel; the clamp
// writes the other (L, kind) buffer, the variance kernel the first V buffer, and each level reads
// one (L, kind) and V buffer and writes the other pair.  Every kernel maps consecutive lanes to
// consecutive x.
template <bool GUIDED>
__global__ void __launch_bounds__(256) rt_denoise_prepare_kernel(const float *__restrict__ sums, const int32_t *__restrict__ counts,
                                                                  int spp, long long n, const rtdn::Q *__restrict__ g,
                                                                  rtdn::Q *__restrict__ a, rtdn::Q *__restrict__ nt,
                                                                  rtdn::Q *__restrict__ pp) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const rtdn::Q rec[4] = {g[4 * p], g[4 * p + 1], g[4 * p + 2], g[4 * p + 3]};
    const float S[3] = {sums[3 * p], sums[3 * p + 1], sums[3 * p + 2]};
    rtdn::Q qa, qn, qp;
    if constexpr (GUIDED)
        rtdg::prepare_pixel(S, counts ? counts[p] : spp, rec, qa, qn, qp);
    else
        rtdn::prepare_pixel(S, counts ? counts[p] : spp, rec, qa, qn, qp);
    a[p] = qa;
    nt[p] = qn;
    pp[p] = qp;
}

// The windowed kernels' tile: kDnTileW x kDnTileH pixels per 256-thread block, tiles numbered
// row-major in a one-dimensional grid.  Wherever a window's halo of REACH pixels is smaller than the
// tile, the tile and its halo are staged in LDS first, 3 x 16 B per pixel and 4 more where the
// variance is a tap word: the plain levels at strides 1 and 2 (reach 2 and 4: 36 x 12 pixels, 20.3 KB,
// and 40 x 16, 30 KB), the clamp (2: 20.3 KB), the variance estimate (3: 38 x 14 pixels, 24.9 KB),
// the guided levels at strides 1 and 2 (52 B per pixel: 21.9 and 32.5 KB).  At stride >= 4 the halo
// outgrows the tile and the taps read through L2 (STAGE = 0: plain loads, any stride).
// Measured against plain loads on the 1080p headline frame, two alternating runs each: the plain
// mode at strides 1 and 2 (profiles/denoise_passes.jsonl), 5 iterations
// 0.753-0.759 ms staged against 0.833-0.836 ms plain; the guided mode in every staged kernel
// (profiles/denoise_guided_passes.jsonl), 5 iterations 1.19 ms staged against
// 1.60 ms plain.
constexpr int kDnTileW = 32, kDnTileH = 8;
constexpr int dn_tile_slots(int reach) { return (kDnTileW + 2 * reach) * (kDnTileH + 2 * reach); }

struct DnTileSrc {
    const rtdn::Q *A, *NT, *PP;   // LDS
    const float *V;               // LDS (the guided level kernel only)
    int x0, y0, tw;               // frame coordinates of the staged tile's corner, its width
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * tw + (x - x0); }
    __device__ __forceinline__ rtdn::Q a(int x, int y) const { return A[at(x, y)]; }
    __device__ __forceinline__ rtdn::Q nt(int x, int y) const { return NT[at(x, y)]; }
    __device__ __forceinline__ rtdn::Q pp(int x, int y) const { return PP[at(x, y)]; }
    __device__ __forceinline__ float v(int x, int y) const { return V[at(x, y)]; }
};

// The block's tile (tx, ty) and the lane's pixel (x, y), which may lie outside the frame.
struct DnLane {
    int tx, ty, x, y;
};
__device__ __forceinline__ DnLane dn_lane(int tiles_x) {
    const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
    const int lx = (int)threadIdx.x % kDnTileW, ly = (int)threadIdx.x / kDnTileW;
    return DnLane{tx, ty, tx * kDnTileW + lx, ty * kDnTileH + ly};
}

// Stages the block's tile with a halo of REACH pixels: slot k of tile[0..2] (and tv, where v_in is
// given) is frame pixel (x0 + k % tw, y0 + k / tw).  A slot outside the frame is never read: every
// window skips such a tap.
template <int REACH>
__device__ __forceinline__ DnTileSrc dn_stage(const DnLane &l, rtdn::Q (*tile)[dn_tile_slots(REACH)], float *tv,
                                              const rtdn::Q *__restrict__ a_in, const rtdn::Q *__restrict__ nt,
                                              const rtdn::Q *__restrict__ pp, const float *__restrict__ v_in, int W, int H) {
    constexpr int tw = kDnTileW + 2 * REACH;
    const int x0 = l.tx * kDnTileW - REACH, y0 = l.ty * kDnTileH - REACH;
    for (int k = (int)threadIdx.x; k < dn_tile_slots(REACH); k += 256) {
        const int gy = y0 + k / tw, gx = x0 + k % tw;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const long long q = (long long)gy * W + gx;
            tile[0][k] = a_in[q];
            tile[1][k] = nt[q];
            tile[2][k] = pp[q];
            if (tv) tv[k] = v_in[q];
        }
    }
    __syncthreads();
    return DnTileSrc{tile[0], tile[1], tile[2], tv, x0, y0, tw};
}

template <int STAGE>
__global__ void __launch_bounds__(256) rt_denoise_level_kernel(const rtdn::Q *__restrict__ a_in, const rtdn::Q *__restrict__ nt,
                                                                const rtdn::Q *__restrict__ pp, rtdn::Q *__restrict__ a_out,
                                                                int W, int H, int tiles_x, rtdn::Level lv) {
    const DnLane l = dn_lane(tiles_x);
    if constexpr (STAGE > 0) {
        __shared__ rtdn::Q tile[3][dn_tile_slots(2 * STAGE)];
        const DnTileSrc src = dn_stage<2 * STAGE>(l, tile, nullptr, a_in, nt, pp, nullptr, W, H);
        if (l.x < W && l.y < H) a_out[(long long)l.y * W + l.x] = rtdn::level_pixel(src, l.x, l.y, W, H, lv);
    } else {
        if (l.x < W && l.y < H)
            a_out[(long long)l.y * W + l.x] = rtdn::level_pixel(rtdn::PlainSrc{a_in, nt, pp, W}, l.x, l.y, W, H, lv);
    }
}

// a == nullptr (iterations = 0): every pixel's own mean.
__global__ void __launch_bounds__(256) rt_denoise_resolve_kernel(const float *__restrict__ sums, const int32_t *__restrict__ counts,
                                                                  int spp, long long n, const rtdn::Q *__restrict__ g,
                                                                  const rtdn::Q *__restrict__ a, float *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float S[3] = {sums[3 * p], sums[3 * p + 1], sums[3 * p + 2]};
    const int cnt = counts ? counts[p] : spp;
    float m[3];
    if (a) {
        const rtdn::Q rec[4] = {g[4 * p], g[4 * p + 1], g[4 * p + 2], g[4 * p + 3]};
        rtdn::resolve_pixel(S, cnt, rec, a[p], m);
    } else {
        const rtdn::Q none{0.f, 0.f, 0.f, rtm::u2f(rtdn::kPass)};
        rtdn::resolve_pixel(S, cnt, nullptr, none, m);
    }
    out[3 * p] = m[0];
    out[3 * p + 1] = m[1];
    out[3 * p + 2] = m[2];
}

// The guided mode's two windows in front of the levels: the firefly clamp ((L, kind) out) and the
// spatial variance estimate (V out).
template <bool VARIANCE>
__global__ void __launch_bounds__(256)
rt_denoise_guided_window_kernel(const rtdn::Q *__restrict__ a_in, const rtdn::Q *__restrict__ nt, const rtdn::Q *__restrict__ pp,
                                std::conditional_t<VARIANCE, float, rtdn::Q> *__restrict__ out, int W, int H, int tiles_x,
                                rtdg::Params dp) {
    constexpr int reach = VARIANCE ? rtdg::kVarianceReach : rtdg::kClampReach;
    const DnLane l = dn_lane(tiles_x);
    __shared__ rtdn::Q tile[3][dn_tile_slots(reach)];
    const DnTileSrc src = dn_stage<reach>(l, tile, nullptr, a_in, nt, pp, nullptr, W, H);
    if (l.x >= W || l.y >= H) return;
    if constexpr (VARIANCE)
        out[(long long)l.y * W + l.x] = rtdg::variance_pixel(src, l.x, l.y, W, H, dp);
    else
        out[(long long)l.y * W + l.x] = rtdg::clamp_pixel(src, l.x, l.y, W, H, dp);
}

// The caller's variance in place of the estimate.
__global__ void __launch_bounds__(256) rt_denoise_guided_given_kernel(const rtdn::Q *__restrict__ a, const float *__restrict__ variance,
                                                                       long long n, float *__restrict__ v_out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) v_out[p] = rtdg::given_variance(rtm::f2u(a[p].w), variance[p]);
}

template <int STAGE>
__global__ void __launch_bounds__(256) rt_denoise_guided_level_kernel(const rtdn::Q *__restrict__ a_in, const float *__restrict__ v_in,
                                                                       const rtdn::Q *__restrict__ nt, const rtdn::Q *__restrict__ pp,
                                                                       rtdn::Q *__restrict__ a_out, float *__restrict__ v_out, int W,
                                                                       int H, int tiles_x, rtdg::Level lv) {
    const DnLane l = dn_lane(tiles_x);
    rtdg::Pixel r;
    if constexpr (STAGE > 0) {
        __shared__ rtdn::Q tile[3][dn_tile_slots(2 * STAGE)];
        __shared__ float tv[dn_tile_slots(2 * STAGE)];
        const DnTileSrc src = dn_stage<2 * STAGE>(l, tile, tv, a_in, nt, pp, v_in, W, H);
        if (l.x >= W || l.y >= H) return;
        r = rtdg::level_pixel(src, l.x, l.y, W, H, lv);
    } else {
        if (l.x >= W || l.y >= H) return;
        r = rtdg::level_pixel(rtdg::PlainSrc{a_in, nt, pp, v_in, W}, l.x, l.y, W, H, lv);
    }
    a_out[(long long)l.y * W + l.x] = r.a;
    v_out[(long long)l.y * W + l.x] = r.v;
}

// a == nullptr (iterations = 0): zeros.
__global__ void __launch_bounds__(256) rt_denoise_guided_varout_kernel(const rtdn::Q *__restrict__ a, const float *__restrict__ v,
                                                                        long long n, float *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) out[p] = a ? rtdg::resolve_variance(a[p], v[p]) : 0.f;
}

// A level kernel's instantiation for a stride: staged at 1 and 2, plain loads above.
#define DN_LEVEL_KERNEL(kernel, stride) ((stride) == 1 ? kernel<1> : (stride) == 2 ? kernel<2> : kernel<0>)

namespace {

// The G-buffer of a shard into device memory (the current device is the scene copy's).
int gbuffer_launch(rt_device_scene *d, const ShardGeom &g, float4 *d_out, hipStream_t stream) {
    if (g.n_pixels == 0) return RT_OK;
    hipLaunchKernelGGL(rt_gbuffer_kernel, dim3((unsigned)((g.n_pixels + 255) / 256)), dim3(256), 0, stream, d->ds, g, d_out);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// What the two modes' launch functions share.  `ws` / `ws_bytes`: the scratch of the call's owner
// (an accumulator, or the device's cache g_dn_ws below), grown on first use; 64 B per pixel: the
// two (L, kind) buffers, (N, t) and (P, 0); 72 B in the guided mode, with its two variance buffers.
struct DnFrame {
    const float *sums;
    const int32_t *counts;
    int spp, W, H;
    const rtdn::Q *g;
    hipStream_t stream;
    long long n;
    int tiles_x;
    dim3 flat, tiles;   // one lane per pixel; one block per tile (below 2^31 tiles: the frame is)
    rtdn::Q *a[2] = {}, *nt = nullptr, *pp = nullptr;
    float *v[2] = {};

    DnFrame(const float *d_sums, const int32_t *d_counts, int spp, int W, int H, const float *d_g, hipStream_t stream)
        : sums(d_sums), counts(d_counts), spp(spp), W(W), H(H), g((const rtdn::Q *)d_g), stream(stream), n((long long)W * H),
          tiles_x((W + kDnTileW - 1) / kDnTileW), flat((unsigned)((n + 255) / 256)),
          tiles((unsigned)((long long)tiles_x * ((H + kDnTileH - 1) / kDnTileH))) {}
    hipError_t scratch(void **ws, size_t *ws_bytes, bool guided) {
        const hipError_t e = grow(ws, ws_bytes, (size_t)n * (4 * sizeof(rtdn::Q) + (guided ? 2 * sizeof(float) : 0)));
        if (e != hipSuccess) return e;
        rtdn::Q *q = (rtdn::Q *)*ws;
        a[0] = q, a[1] = q + n, nt = q + 2 * n, pp = q + 3 * n;
        if (guided) v[0] = (float *)(q + 4 * n), v[1] = v[0] + n;
        return e;
    }
    // The last step of both modes, and with fa == nullptr all of iterations = 0: the means from the
    // filtered (L, kind) buffer fa, and the filtered variance fv where the caller asks for it.
    int resolve(const rtdn::Q *fa, const float *fv, float *d_out, float *d_out_var) const {
        hipLaunchKernelGGL(rt_denoise_resolve_kernel, flat, dim3(256), 0, stream, sums, counts, spp, n, g, fa, d_out);
        if (d_out_var) hipLaunchKernelGGL(rt_denoise_guided_varout_kernel, flat, dim3(256), 0, stream, fa, fv, n, d_out_var);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
};

// The filter on the current device.
int denoise_launch(void **ws, size_t *ws_bytes, const float *d_sums, const int32_t *d_counts, int spp, int W, int H,
                   const float *d_g, const rtdn::Params &dp, float *d_out, hipStream_t stream) {
    DnFrame f(d_sums, d_counts, spp, W, H, d_g, stream);
    if (dp.iterations == 0) return f.resolve(nullptr, nullptr, d_out, nullptr);
    HIP_TRY(f.scratch(ws, ws_bytes, false));
    hipLaunchKernelGGL(rt_denoise_prepare_kernel<false>, f.flat, dim3(256), 0, stream, d_sums, d_counts, spp, f.n, f.g, f.a[0], f.nt,
                       f.pp);
    for (int k = 0; k < dp.iterations; ++k) {
        const rtdn::Level lv = rtdn::level_of(dp, k);
        hipLaunchKernelGGL(DN_LEVEL_KERNEL(rt_denoise_level_kernel, lv.stride), f.tiles, dim3(256), 0, stream,
                           (const rtdn::Q *)f.a[k & 1], (const rtdn::Q *)f.nt, (const rtdn::Q *)f.pp, f.a[(k + 1) & 1], W, H, f.tiles_x,
                           lv);
    }
    return f.resolve(f.a[dp.iterations & 1], nullptr, d_out, nullptr);
}

// The variance-guided mode on the current device, on the same scratch rules (d_var / d_out_var: the
// caller's variance, the filtered variance out, or NULL).
int denoise_guided_launch(void **ws, size_t *ws_bytes, const float *d_sums, const int32_t *d_counts, int spp, int W, int H,
                          const float *d_g, const float *d_var, const rtdg::Params &dp, float *d_out, float *d_out_var,
                          hipStream_t stream) {
    DnFrame f(d_sums, d_counts, spp, W, H, d_g, stream);
    if (dp.iterations == 0) return f.resolve(nullptr, nullptr, d_out, d_out_var);
    HIP_TRY(f.scratch(ws, ws_bytes, true));
    hipLaunchKernelGGL(rt_denoise_prepare_kernel<true>, f.flat, dim3(256), 0, stream, d_sums, d_counts, spp, f.n, f.g, f.a[0], f.nt,
                       f.pp);
    const rtdn::Q *nt = f.nt, *pp = f.pp;
    int cur = 0;   // the buffers that hold (L, kind) and V
    if (!(dp.firefly < 0.f)) {
        hipLaunchKernelGGL(rt_denoise_guided_window_kernel<false>, f.tiles, dim3(256), 0, stream, (const rtdn::Q *)f.a[0], nt, pp, f.a[1],
                           W, H, f.tiles_x, dp);
        cur = 1;
    }
    if (d_var)
        hipLaunchKernelGGL(rt_denoise_guided_given_kernel, f.flat, dim3(256), 0, stream, (const rtdn::Q *)f.a[cur], d_var, f.n, f.v[cur]);
    else
        hipLaunchKernelGGL(rt_denoise_guided_window_kernel<true>, f.tiles, dim3(256), 0, stream, (const rtdn::Q *)f.a[cur], nt, pp,
                           f.v[cur], W, H, f.tiles_x, dp);
    for (int k = 0; k < dp.iterations; ++k, cur ^= 1) {
        const rtdg::Level lv = rtdg::level_of(dp, k);
        hipLaunchKernelGGL(DN_LEVEL_KERNEL(rt_denoise_guided_level_kernel, lv.stride), f.tiles, dim3(256), 0, stream,
                           (const rtdn::Q *)f.a[cur], (const float *)f.v[cur], nt, pp, f.a[cur ^ 1], f.v[cur ^ 1], W, H, f.tiles_x, lv);
    }
    return f.resolve(f.a[cur], f.v[cur], d_out, d_out_var);
}

}  // namespace

// The measured variance (rt_moments.h variance_of_pixel): one thread per pixel, consecutive lanes
// on consecutive pixels; counts or, when null, `spp` for every pixel.
__global__ void __launch_bounds__(256) rt_variance_kernel(const float *__restrict__ sums, const float *__restrict__ moments,
                                                           const int32_t *__restrict__ counts, int spp, long long n,
                                                           const float4 *__restrict__ g, float *__restrict__ out) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float4 g1 = g[rtd::kGbufferQuads * p + 1];
    const float S[3] = {sums[3 * p], sums[3 * p + 1], sums[3 * p + 2]};
    const float Q[3] = {moments[3 * p], moments[3 * p + 1], moments[3 * p + 2]};
    const float al[3] = {g1.x, g1.y, g1.z};
    out[p] = rtmo::variance_of_mean(counts ? counts[p] : spp, S, Q, al, __float_as_int(g1.w) >= 0);
}

namespace {

// rt_variance_kernel on the current device.
int variance_launch(const float *d_sums, const float *d_moments, const int32_t *d_counts, int spp, long long n, const float *d_g,
                    float *d_out, hipStream_t stream) {
    if (n == 0) return RT_OK;
    hipLaunchKernelGGL(rt_variance_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_sums, d_moments, d_counts,
                       spp, n, (const float4 *)d_g, d_out);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// rt_denoise_device's and rt_denoise_guided_device's scratch, per device, from the first call on
// (only grows).
std::mutex g_dn_mu;
void *g_dn_ws[kRtMaxDevices] = {};
size_t g_dn_ws_bytes[kRtMaxDevices] = {};

// rt_denoise_frame_u8 / rt_denoise_guided_frame_u8: host arrays to `device`, filtered there by
// launch(d_sums, d_counts, d_gbuffer, d_variance, d_mean) under the device cache's lock, finished
// at spp = 1, the bytes copied back.  variance may be NULL.
template <class Launch>
int denoise_frame_bytes(const std::string &who, const float *sums, const int32_t *counts, int32_t width, int32_t height,
                        const float *gbuffer, const float *variance, int32_t device, uint8_t *out_rgb, Launch launch) {
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev || device >= kRtMaxDevices)
        return rt_fail(RT_ERR_DEVICE, "no HIP device " + std::to_string(device));
    DeviceGuard guard(device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    // one staging allocation: sums, mean, G-buffer, counts, variance, bytes (each part 256-byte aligned)
    const size_t n = (size_t)width * height;
    const size_t o_mean = rtp::align_up(n * 12), o_g = o_mean + rtp::align_up(n * 12), o_cnt = o_g + n * 64,
                 o_var = o_cnt + rtp::align_up(n * 4), o_rgb = o_var + (variance ? rtp::align_up(n * 4) : 0), total = o_rgb + n * 3;
    uint8_t *buf = nullptr;
    HIP_TRY(hipMalloc((void **)&buf, total));
    int32_t *d_counts = counts ? (int32_t *)(buf + o_cnt) : nullptr;
    float *d_var = variance ? (float *)(buf + o_var) : nullptr;
    hipError_t e = hipMemcpy(buf, sums, n * 12, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + o_g, gbuffer, n * 64, hipMemcpyHostToDevice);
    if (e == hipSuccess && counts) e = hipMemcpy(d_counts, counts, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && variance) e = hipMemcpy(d_var, variance, n * 4, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? RT_OK : rt_fail(RT_ERR_DEVICE, who + " copy: " + hipGetErrorString(e));
    if (rc == RT_OK) {
        std::lock_guard<std::mutex> lock(g_dn_mu);
        rc = launch((const float *)buf, (const int32_t *)d_counts, (const float *)(buf + o_g), (const float *)d_var,
                    (float *)(buf + o_mean));
    }
    if (rc == RT_OK) rc = rt_tonemap_u8_device((const float *)(buf + o_mean), width, height, 1, buf + o_rgb, nullptr);
    if (rc == RT_OK) {
        e = hipMemcpy(out_rgb, buf + o_rgb, n * 3, hipMemcpyDeviceToHost);   // (waits for the default stream)
        if (e != hipSuccess) rc = rt_fail(RT_ERR_DEVICE, who + " copy: " + hipGetErrorString(e));
    }
    (void)hipFree(buf);
    return rc;
}

}  // namespace

extern "C" {

int rt_gbuffer_device(rt_scene *s, const rt_params *p, float *d_out, void *stream) {
    if (!s || !p || !d_out) return rt_fail(RT_ERR_ARG, "rt_gbuffer_device: NULL argument");
    Shard sh;
    if (int rc = shard_of(s, p, "rt_gbuffer_device", sh)) return rc;
    if (p->device < 0 || p->device >= kRtMaxDevices || !s->dev[p->device])
        return rt_fail(RT_ERR_ARG, "rt_gbuffer_device: scene not uploaded to device " + std::to_string(p->device));
    rt_device_scene *d = s->dev[p->device];
    DeviceGuard guard(d->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    return gbuffer_launch(d, sh.g, (float4 *)d_out, (hipStream_t)stream);
}

int rt_gbuffer(rt_scene *s, const rt_params *p, float *out) {
    if (!s || !p || !out) return rt_fail(RT_ERR_ARG, "rt_gbuffer: NULL argument");
    Shard sh;
    if (int rc = shard_of(s, p, "rt_gbuffer", sh)) return rc;
    if (int rc = ensure_device_scene(s, p->device)) return rc;
    rt_device_scene *d = s->dev[p->device];
    DeviceGuard guard(d->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const size_t bytes = (size_t)sh.n_pixels * RT_GBUFFER_WORDS * sizeof(float);
    float4 *d_out = nullptr;
    HIP_TRY(hipMalloc((void **)&d_out, bytes ? bytes : 64));
    int rc = gbuffer_launch(d, sh.g, d_out, nullptr);
    if (rc == RT_OK && bytes) {
        const hipError_t e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = rt_fail(RT_ERR_DEVICE, std::string("rt_gbuffer copy: ") + hipGetErrorString(e));
    }
    (void)hipFree(d_out);
    return rc;
}

int rt_denoise_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                      const float *d_gbuffer, const rt_denoise_params *params, float *d_out_mean, void *stream) {
    rtdn::Params dp;
    if (int rc = rt_denoise_check("rt_denoise_device", d_sums, d_counts, spp, width, height, d_gbuffer, params, d_out_mean, &dp))
        return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kRtMaxDevices) return rt_fail(RT_ERR_DEVICE, "rt_denoise_device: device id");
    std::lock_guard<std::mutex> lock(g_dn_mu);
    return denoise_launch(&g_dn_ws[dev], &g_dn_ws_bytes[dev], d_sums, d_counts, spp, width, height, d_gbuffer, dp, d_out_mean,
                          (hipStream_t)stream);
}

int rt_denoise_frame_u8(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height, const float *gbuffer,
                        const rt_denoise_params *params, int32_t device, uint8_t *out_rgb) {
    if (!out_rgb) return rt_fail(RT_ERR_ARG, "rt_denoise_frame_u8: NULL argument");
    rtdn::Params dp;
    if (int rc = rt_denoise_check("rt_denoise_frame_u8", sums, counts, spp, width, height, gbuffer, params, sums, &dp)) return rc;
    return denoise_frame_bytes("rt_denoise_frame_u8", sums, counts, width, height, gbuffer, nullptr, device, out_rgb,
                               [&](const float *d_sums, const int32_t *d_counts, const float *d_g, const float *, float *d_mean) {
                                   return denoise_launch(&g_dn_ws[device], &g_dn_ws_bytes[device], d_sums, d_counts, spp, width, height,
                                                         d_g, dp, d_mean, nullptr);
                               });
}

int rt_denoise_guided_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                             const float *d_gbuffer, const float *d_variance, const rt_denoise_guided_params *params,
                             float *d_out_mean, float *d_out_variance, void *stream) {
    rtdg::Params dp;
    if (int rc = rt_denoise_guided_check("rt_denoise_guided_device", d_sums, d_counts, spp, width, height, d_gbuffer, params,
                                         d_out_mean, &dp))
        return rc;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kRtMaxDevices) return rt_fail(RT_ERR_DEVICE, "rt_denoise_guided_device: device id");
    std::lock_guard<std::mutex> lock(g_dn_mu);
    return denoise_guided_launch(&g_dn_ws[dev], &g_dn_ws_bytes[dev], d_sums, d_counts, spp, width, height, d_gbuffer, d_variance, dp,
                                 d_out_mean, d_out_variance, (hipStream_t)stream);
}

int rt_denoise_guided_frame_u8(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                               const float *gbuffer, const float *variance, const rt_denoise_guided_params *params, int32_t device,
                               uint8_t *out_rgb) {
    if (!out_rgb) return rt_fail(RT_ERR_ARG, "rt_denoise_guided_frame_u8: NULL argument");
    rtdg::Params dp;
    if (int rc = rt_denoise_guided_check("rt_denoise_guided_frame_u8", sums, counts, spp, width, height, gbuffer, params, sums, &dp))
        return rc;
    return denoise_frame_bytes("rt_denoise_guided_frame_u8", sums, counts, width, height, gbuffer, variance, device, out_rgb,
                               [&](const float *d_sums, const int32_t *d_counts, const float *d_g, const float *d_var, float *d_mean) {
                                   return denoise_guided_launch(&g_dn_ws[device], &g_dn_ws_bytes[device], d_sums, d_counts, spp, width,
                                                                height, d_g, d_var, dp, d_mean, nullptr, nullptr);
                               });
}

int rt_variance_from_moments_device(const float *d_sums, const float *d_moments, const int32_t *d_counts, int32_t spp,
                                    int32_t width, int32_t height, const float *d_gbuffer, float *d_out, void *stream) {
    if (int rc = rt_variance_check("rt_variance_from_moments_device", d_sums, d_moments, d_counts, spp, width, height, d_gbuffer, d_out))
        return rc;
    return variance_launch(d_sums, d_moments, d_counts, spp, (long long)width * height, d_gbuffer, d_out, (hipStream_t)stream);
}

}  // extern "C"
