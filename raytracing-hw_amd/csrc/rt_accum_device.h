// rt_accum_device.h — the device half of the accumulator: rt_accum, its kernels, helpers and every
// rt_accum_* entry of include/rt_hw.h.  Included by rt_device.hip after launch() / render_host and
// after rt_denoise_device.h (the frames call both), so the build stays one translation unit.
//
// An accumulator is the per-pixel chain state of one shard on one device, kept between passes
// (rt_mega.h, chain buffer).  It owns the chain buffer (one 32-byte record per shard pixel,
// rt_records.h) and the float sums its passes write; a pass is launch() with a ChainPass (both, and
// the fold kernels launch() runs, in rt_device.hip).  Host only, tested without a device: the
// kinds, parameter checks, host state (rtap::State) and passes in rt_accum_plan.h, the checkpoint
// file in rt_accum_file.h.
struct rt_accum : rtap::State {
    rt_scene *scene = nullptr;
    uint32_t epoch = 0;       // the scene's camera epoch its samples were rendered at (create, load, reset)
    rt_params p{};            // rank, world, row_block, device, flags (normalised)
    long long n_pixels = 0;
    int rows = 0;
    ShardGeom geom{};         // the shard (shard_of)
    rtap::Kind kind = rtap::Kind::Parity;   // a fast kind's chain buffer holds fast records (rt_records.h)
    uint4 *chain = nullptr;   // n_pixels records of the kind
    float *sums = nullptr;    // n_pixels x 3
    uint8_t *rgb = nullptr;   // n_pixels x 3, made by the first rt_accum_frame_u8
    hipStream_t stream = nullptr;   // the last pass's stream (host reads wait for it)
    // rt_accum_mark's copy of the sums and counts (made on first use)
    float *mark_sums = nullptr;
    int32_t *mark_counts = nullptr;
    // rt_accum_select's pending list (shard pixels, ascending; made on first use) and its kernel's buffers
    int *sel_list = nullptr;
    unsigned *sel_blocks = nullptr;        // per block of rt_select_kernel: selected count, then list offset
    unsigned long long *sel_out = nullptr; // SelectOut
    uint8_t *sel_mask = nullptr;           // device copy of rt_select.mask
    int32_t *counts = nullptr;             // n_pixels, for the count-aware finish
    // A moments accumulator (rt_moments.h) also keeps per pixel the moment record (32 bytes,
    // rt_records.h) and the reported moment (n_pixels x 3); both made at creation.
    // `var`: the measured variance, made on first use.
    bool has_moments() const { return kind == rtap::Kind::Moments; }
    uint4 *mom = nullptr;
    float *moments = nullptr;
    float *var = nullptr;
    // rt_accum_frame_u8_denoised's, made on first use and kept: the shard's first-hit records
    // (rendered once: they depend on the scene alone), the filter's scratch and its mean frame
    float4 *gbuf = nullptr;
    bool gbuf_ready = false;   // the records have been rendered into gbuf
    void *dn_ws = nullptr;
    size_t dn_ws_bytes = 0;
    float *dn_mean = nullptr;
};

// What rt_select_kernel reduces besides the list (device words, zeroed / set before the launch).
struct SelectOut {
    unsigned long long n_selected, samples;   // samples: sum of (target - next) over the selected
    int next_min, next_max;                   // of `next` as it will be after the pass
    int from_min, reserved;                   // the smallest `next` among the selected, as it stands (a fast
                                              // pass's units per item come from it); INT32_MAX for an empty list
};

// The selection (rt_accum_select, rt_select.h): one thread per shard pixel applies the rule.
// WRITE = false counts: per wave a ballot, per block the four wave counts, block b's count to
// blocks[b], and the reductions of SelectOut per wave (shuffles), per block (LDS), one atomic
// per block and value.  rt_select_scan_kernel then turns the block counts into list offsets,
// and WRITE = true evaluates the same rule again and writes pixel p to
// list[blocks[b] + selected in the block's earlier waves + selected lanes below (mbcnt)]: the
// list is in ascending shard-pixel order, holds each pixel at most once, and no atomic orders it.
// VAR (rt_accum_select_variance, a moments accumulator): steps 1 and 2 of the rule, then the
// relative standard error of the mean from the moments (rt_moments.h relative_error) in place of
// steps 3 and 4; `mark_sums` then carries the reported moments and `mark_counts` is null (no
// mark is read).  The scan and the list order are the same.
template <bool WRITE, bool VAR = false>
__global__ void __launch_bounds__(256) rt_select_kernel(ShardGeom g, rtsel::Rule rule, const uint4 *chain, const float *sums,
                                                         const float *mark_sums, const int32_t *mark_counts,
                                                         const uint8_t *mask, unsigned *blocks, int *list, SelectOut *out) {
    __shared__ unsigned wave_n[4];
    __shared__ unsigned long long wave_s[4];
    __shared__ int wave_lo[4], wave_hi[4], wave_from[4];
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool sel = false;
    int n_b = 0;
    if (p < g.n_pixels) {
        n_b = (int)rtrec::next_of((const uint32_t *)chain, p);
        int x, y;
        rtd::shard_xy(g, p, x, y);
        const float S_b[3] = {sums[3 * p], sums[3 * p + 1], sums[3 * p + 2]};
        if constexpr (VAR) {
            const float Q_b[3] = {mark_sums[3 * p], mark_sums[3 * p + 1], mark_sums[3 * p + 2]};
            sel = rtmo::selected(rule, x, y, mask ? mask[p] : 1u, n_b, S_b, Q_b);
        } else {
            const int n_a = mark_counts ? mark_counts[p] : 0;
            float S_a[3] = {0.f, 0.f, 0.f};
            if (mark_sums) {
                S_a[0] = mark_sums[3 * p];
                S_a[1] = mark_sums[3 * p + 1];
                S_a[2] = mark_sums[3 * p + 2];
            }
            sel = rtsel::selected(rule, x, y, mask ? mask[p] : 1u, n_b, S_b, n_a, S_a);
        }
    }
    const unsigned long long m = __ballot(sel);
    if (lane == 0) wave_n[wave] = (unsigned)__popcll(m);
    if constexpr (!WRITE) {
        unsigned long long s = sel ? (unsigned long long)(rule.target - n_b) : 0ull;
        const int after = sel ? rule.target : n_b;
        int lo = p < g.n_pixels ? after : 0x7fffffff, hi = p < g.n_pixels ? after : 0;
        int from = sel ? n_b : 0x7fffffff;
        for (int k = 32; k > 0; k >>= 1) {
            s += __shfl_xor(s, k, 64);
            lo = min(lo, __shfl_xor(lo, k, 64));
            hi = max(hi, __shfl_xor(hi, k, 64));
            from = min(from, __shfl_xor(from, k, 64));
        }
        if (lane == 0) {
            wave_s[wave] = s;
            wave_lo[wave] = lo;
            wave_hi[wave] = hi;
            wave_from[wave] = from;
        }
    }
    __syncthreads();
    if constexpr (WRITE) {
        unsigned base = blocks[blockIdx.x];
        for (int w = 0; w < wave; ++w) base += wave_n[w];
        const unsigned below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (sel) list[base + below] = (int)p;
    } else if (threadIdx.x == 0) {
        const unsigned n = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        blocks[blockIdx.x] = n;
        atomicAdd(&out->n_selected, (unsigned long long)n);
        atomicAdd(&out->samples, wave_s[0] + wave_s[1] + wave_s[2] + wave_s[3]);
        atomicMin(&out->next_min, min(min(wave_lo[0], wave_lo[1]), min(wave_lo[2], wave_lo[3])));
        atomicMax(&out->next_max, max(max(wave_hi[0], wave_hi[1]), max(wave_hi[2], wave_hi[3])));
        atomicMin(&out->from_min, min(min(wave_from[0], wave_from[1]), min(wave_from[2], wave_from[3])));
    }
}

// Exclusive prefix sum of the selection's block counts, in place, by one block: thread t sums
// its run of ceil(n / 256) counts, thread 0 scans the 256 run sums, thread t writes its run.
__global__ void __launch_bounds__(256) rt_select_scan_kernel(unsigned *blocks, long long n) {
    __shared__ unsigned run[256];
    const long long per = (n + 255) / 256, b0 = (long long)threadIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
    unsigned s = 0;
    for (long long b = b0; b < b1; ++b) s += blocks[b];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned acc = 0;
        for (int t = 0; t < 256; ++t) {
            const unsigned v = run[t];
            run[t] = acc;
            acc += v;
        }
    }
    __syncthreads();
    unsigned acc = run[threadIdx.x];
    for (long long b = b0; b < b1; ++b) {
        const unsigned v = blocks[b];
        blocks[b] = acc;
        acc += v;
    }
}

// rt_accum_mark: the sums and counts as they stand, for the selection rule's "before" half.
__global__ void __launch_bounds__(256) rt_mark_kernel(const uint4 *chain, const float *sums, long long n, float *mark_sums,
                                                       int32_t *mark_counts) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    mark_sums[3 * p + 0] = sums[3 * p + 0];
    mark_sums[3 * p + 1] = sums[3 * p + 1];
    mark_sums[3 * p + 2] = sums[3 * p + 2];
    mark_counts[p] = (int32_t)rtrec::next_of((const uint32_t *)chain, p);
}

// The sample-count map: every record's next sample.
__global__ void __launch_bounds__(256) rt_counts_kernel(const uint4 *chain, long long n, int32_t *counts) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) counts[p] = (int32_t)rtrec::next_of((const uint32_t *)chain, p);
}

__global__ void __launch_bounds__(256) rt_chain_init_kernel(DevScene sc, ShardGeom g, uint4 *chain, float *sums) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.n_pixels) return;
    rtd::chain_init(chain, sc, g, (int)p);
    sums[3 * p + 0] = 0.f;
    sums[3 * p + 1] = 0.f;
    sums[3 * p + 2] = 0.f;
}

// A fresh fast record: no samples, total and open +0.
__global__ void __launch_bounds__(256) rt_fast_chain_init_kernel(long long n, uint4 *chain, float *sums) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    rtd::fast_rec_store(chain, p, rtfu::Rec{0, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}});
    sums[3 * p + 0] = 0.f;
    sums[3 * p + 1] = 0.f;
    sums[3 * p + 2] = 0.f;
}

namespace {

void accum_release(rt_accum *a) {
    if (!a) return;
    if (a->chain || a->sums || a->rgb) {
        DeviceGuard guard(a->p.device);
        for (void *b : {(void *)a->chain, (void *)a->sums, (void *)a->rgb, (void *)a->mark_sums, (void *)a->mark_counts,
                        (void *)a->sel_list, (void *)a->sel_blocks, (void *)a->sel_out, (void *)a->sel_mask, (void *)a->counts,
                        (void *)a->gbuf, a->dn_ws, (void *)a->dn_mean, (void *)a->mom, (void *)a->moments, (void *)a->var})
            if (b) (void)hipFree(b);
    }
    delete a;
}

// Host-side part of create / load: parameters and shard, no device call (a fast kind's p->fast_chunk: 0 = 2).
int accum_new(rt_scene *s, const rt_params *p, const char *who, rt_accum **out, rtap::Kind kind) {
    if (int rc = check_flags(p, who)) return rc;
    if (const rtp::Refusal r = rtap::check_params(kind, p->flags, p->count, p->kernel, p->fast_chunk, who)) return rt_fail(r.code, r.msg);
    if (p->device < 0 || p->device >= kRtMaxDevices) return rt_fail(RT_ERR_ARG, std::string(who) + ": bad device " + std::to_string(p->device));
    Shard sh;
    if (int rc = shard_of(s, p, who, sh)) return rc;
    rt_accum *a = new rt_accum();
    a->scene = s, a->kind = kind, a->epoch = s->view_epoch;
    a->p = *p;
    a->p.spp = 0, a->p.world = sh.world, a->p.row_block = sh.row_block;
    a->rows = sh.rows, a->n_pixels = sh.n_pixels, a->geom = sh.g;
    if (rtap::info(kind).fast) {   // (what its passes render with: fast units, no order, the chunk size as it is)
        a->fast_c = p->fast_chunk > 0 ? p->fast_chunk : 2;
        a->p.flags = RT_FLAG_FAST;
        a->p.fast_chunk = a->fast_c;
    }
    *out = a;
    return RT_OK;
}

// Device buffers of a new accumulator (the scene is on the device).
int accum_alloc(rt_accum *a) {
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const size_t n = (size_t)std::max<long long>(a->n_pixels, 1);
    HIP_TRY(hipMalloc((void **)&a->chain, n * 32));
    HIP_TRY(hipMalloc((void **)&a->sums, n * 3 * sizeof(float)));
    if (a->has_moments()) {   // (zero words: no samples, total2 and open2 +0.f)
        HIP_TRY(hipMalloc((void **)&a->mom, n * 32));
        HIP_TRY(hipMalloc((void **)&a->moments, n * 3 * sizeof(float)));
        HIP_TRY(hipMemset(a->mom, 0, n * 32));
        HIP_TRY(hipMemset(a->moments, 0, n * 3 * sizeof(float)));
    }
    return RT_OK;
}

int accum_wait(rt_accum *a) {
    HIP_TRY(hipStreamSynchronize(a->stream));
    return RT_OK;
}

// The scene's camera or triangles have moved since the accumulator's samples were rendered
// (rt_scene_set_camera, rt_scene_update_tris*): only the read-outs of the old view still work;
// everything else asks for rt_accum_reset.
int accum_stale(const rt_accum *a, const std::string &who) {
    if (a->epoch == a->scene->view_epoch) return RT_OK;
    return rt_fail(RT_ERR_ARG, who + ": the scene's camera or geometry has changed since this accumulator's samples were rendered; "
                                     "call rt_accum_reset (its sums, counts and moments still read out the old view)");
}

// Fresh records and zero sums on `stream` (create and reset; the current device is the accumulator's).
void accum_init_launch(rt_accum *a, hipStream_t stream) {
    const dim3 blocks((unsigned)((a->n_pixels + 255) / 256));
    if (a->fast_c)
        hipLaunchKernelGGL(rt_fast_chain_init_kernel, blocks, dim3(256), 0, stream, a->n_pixels, a->chain, a->sums);
    else
        hipLaunchKernelGGL(rt_chain_init_kernel, blocks, dim3(256), 0, stream, a->scene->dev[a->p.device]->ds, a->geom, a->chain,
                           a->sums);
}

// A device buffer of an accumulator made on first use (the current device is the accumulator's).
template <class T>
int accum_buffer(T *&p, size_t count) {
    if (!p) HIP_TRY(hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T)));
    return RT_OK;
}

// The sample-count map into a->counts, on the accumulator's stream.
int accum_counts_launch(rt_accum *a, int32_t *d_counts, hipStream_t stream) {
    if (a->n_pixels == 0) return RT_OK;
    hipLaunchKernelGGL(rt_counts_kernel, dim3((unsigned)((a->n_pixels + 255) / 256)), dim3(256), 0, stream,
                       (const uint4 *)a->chain, a->n_pixels, d_counts);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The counts a frame divides by: null while every pixel holds a->samples, else the map in a->counts, on a->stream.
int accum_counts_if_mixed(rt_accum *a, const int32_t **counts) {
    *counts = nullptr;
    if (a->uniform()) return RT_OK;
    if (int rc = accum_buffer(a->counts, (size_t)a->n_pixels)) return rc;
    if (int rc = accum_counts_launch(a, a->counts, a->stream)) return rc;
    *counts = a->counts;
    return RT_OK;
}

// The host-copy entries: on the accumulator's device, prepare() (what the entry queues first; it
// may make the buffer), the wait for the stream, then `bytes` of the buffer `src` to `out`.
template <class T, class Prepare = int (*)()>
int accum_read_back(rt_accum *a, T *rt_accum::*src, size_t bytes, void *out, Prepare prepare = [] { return (int)RT_OK; }) {
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = prepare()) return rc;
    if (int rc = accum_wait(a)) return rc;
    if (bytes) HIP_TRY(hipMemcpy(out, a->*src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

// rt_accum_create and its fast forms (`who` names the entry in messages).
int accum_create(rt_scene *s, const rt_params *p, rt_accum **out, const std::string &who, rtap::Kind kind) {
    if (!s || !p || !out) return rt_fail(RT_ERR_ARG, who + ": NULL argument");
    *out = nullptr;
    rt_accum *a = nullptr;
    if (int rc = accum_new(s, p, who.c_str(), &a, kind)) return rc;
    if (!s->dev[a->p.device]) {
        accum_release(a);
        return rt_fail(RT_ERR_ARG, who + ": scene not uploaded to device " + std::to_string(p->device));
    }
    int rc = accum_alloc(a);
    if (rc == RT_OK && a->n_pixels > 0) {
        DeviceGuard guard(a->p.device);
        accum_init_launch(a, nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) rc = rt_fail(RT_ERR_DEVICE, who + ": " + hipGetErrorString(e));
    }
    if (rc) {
        accum_release(a);
        return rc;
    }
    *out = a;
    return RT_OK;
}

// A planned pass (rt_accum_plan.h) on `stream`: the one place that makes an accumulator's ChainPass.
// A parity pass is one launch to the target, and `st` is that launch's.  A fast pass runs as the
// launches next_launch cuts it into; `st` sums their times, with the pass's pixel and sample totals.
int accum_pass(rt_accum *a, const rtap::Pass &ps, hipStream_t stream, rt_stats *st) {
    a->stream = stream;
    rt_params p = a->p;
    p.spp = ps.target;
    ChainPass cp{a->chain, ps.n};
    cp.items = ps.items ? a->sel_list : nullptr, cp.n_items = ps.n_items, cp.samples = ps.items ? ps.samples : 0;
    if (!a->fast_c) return launch(a->scene, &p, a->sums, stream, st, &cp);
    cp.fast_c = a->fast_c, cp.mom = a->mom, cp.moments = a->moments;
    rt_stats total{};
    for (int from = ps.from; from < ps.target;) {
        const int to = rtap::next_launch(from, ps.target, a->fast_c);
        p.spp = to, cp.n = to - from;
        cp.fast_units = rtfu::units_of(from, to, a->fast_c);   // (of the item furthest behind)
        rt_stats one{};
        if (int rc = launch(a->scene, &p, a->sums, stream, st ? &one : nullptr, &cp)) return rc;
        total.render_ms += one.render_ms, total.schedule |= one.schedule;
        total.pixels = one.pixels, total.devices = one.devices;
        from = to;   // (items that stood at or past `to` were not touched and stay ahead of it)
    }
    if (st) {
        *st = total;
        if (ps.items) st->pixels = (uint64_t)ps.n_items;
        st->samples = ps.samples;
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_accum_create(rt_scene *s, const rt_params *p, rt_accum **out) {
    return accum_create(s, p, out, "rt_accum_create", rtap::Kind::Parity);
}

int rt_accum_create_fast(rt_scene *s, const rt_params *p, rt_accum **out) {
    return accum_create(s, p, out, "rt_accum_create_fast", rtap::Kind::Fast);
}

int32_t rt_accum_fast_chunk(const rt_accum *a) { return a ? a->fast_c : 0; }

int rt_accum_create_fast_moments(rt_scene *s, const rt_params *p, rt_accum **out) {
    return accum_create(s, p, out, "rt_accum_create_fast_moments", rtap::Kind::Moments);
}

int32_t rt_accum_has_moments(const rt_accum *a) { return a && a->has_moments() ? 1 : 0; }

int rt_accum_moments(rt_accum *a, float *out) {
    if (!a || !out) return rt_fail(RT_ERR_ARG, "rt_accum_moments: NULL argument");
    if (!a->has_moments()) return rt_fail(RT_ERR_ARG, "rt_accum_moments: the accumulator keeps no moments (rt_accum_create_fast_moments)");
    return accum_read_back(a, &rt_accum::moments, (size_t)a->n_pixels * 3 * sizeof(float), out);
}

const float *rt_accum_device_moments(rt_accum *a) { return a && a->has_moments() ? a->moments : nullptr; }

int rt_accum_add(rt_accum *a, int32_t n_samples, void *stream, rt_stats *st) {
    if (!a) return rt_fail(RT_ERR_ARG, "rt_accum_add: NULL accumulator");
    if (int rc = accum_stale(a, "rt_accum_add")) return rc;
    const rtap::Pass ps = rtap::plan_add(*a, n_samples, a->n_pixels);
    if (ps.refused) return rt_fail(ps.refused.code, ps.refused.msg);
    if (int rc = accum_pass(a, ps, (hipStream_t)stream, st)) return rc;
    rtap::commit_add(*a, ps);
    return RT_OK;
}

int rt_accum_mark(rt_accum *a, void *stream) {
    if (!a) return rt_fail(RT_ERR_ARG, "rt_accum_mark: NULL accumulator");
    if (int rc = accum_stale(a, "rt_accum_mark")) return rc;
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    // (a pending selection stays: the mark changes no record, so the list is as safe as it was)
    if (int rc = accum_buffer(a->mark_sums, (size_t)a->n_pixels * 3)) return rc;
    if (int rc = accum_buffer(a->mark_counts, (size_t)a->n_pixels)) return rc;
    a->stream = (hipStream_t)stream;
    if (a->n_pixels > 0) {
        hipLaunchKernelGGL(rt_mark_kernel, dim3((unsigned)((a->n_pixels + 255) / 256)), dim3(256), 0, a->stream,
                           (const uint4 *)a->chain, (const float *)a->sums, a->n_pixels, a->mark_sums, a->mark_counts);
        HIP_TRY(hipGetLastError());
    }
    a->has_mark = true;
    return RT_OK;
}

// rt_accum_select and, with `variance`, rt_accum_select_variance (`who` names the entry in messages).
static int accum_select(rt_accum *a, const rt_select *sel, void *stream, int64_t *n_selected, const std::string &who,
                        bool variance) {
    // every argument check comes before any device call
    if (!sel) return rt_fail(RT_ERR_ARG, who + ": NULL selection");
    const rtsel::Rule rule{sel->target, sel->x0, sel->y0, sel->x1, sel->y1, sel->threshold};
    const int bad = rtsel::check_rule(rule, a ? a->scene->width : INT32_MAX, a ? a->scene->height : INT32_MAX);
    if (bad == 2) return rt_fail(RT_ERR_LIMIT, who + ": target must be < 2^20");
    if (bad == 1)
        return rt_fail(RT_ERR_ARG, rule.target < 1 ? who + ": target must be >= 1"
                                                   : who + ": bad window [" + std::to_string(rule.x0) + ", " +
                                                         std::to_string(rule.x1) + ") x [" + std::to_string(rule.y0) + ", " +
                                                         std::to_string(rule.y1) + ")");
    if (!a) return rt_fail(RT_ERR_ARG, who + ": NULL accumulator");
    if (int rc = accum_stale(a, who)) return rc;
    if (variance && !a->has_moments())
        return rt_fail(RT_ERR_ARG, who + ": the accumulator keeps no moments (rt_accum_create_fast_moments)");
    a->sel_pending = false;
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const long long n = a->n_pixels, nb = (n + 255) / 256;
    if (int rc = accum_buffer(a->sel_list, (size_t)n)) return rc;
    if (int rc = accum_buffer(a->sel_blocks, (size_t)nb)) return rc;
    if (int rc = accum_buffer(a->sel_out, sizeof(SelectOut) / sizeof(unsigned long long))) return rc;
    if (sel->mask) {   // (the last launch that read the mask buffer has been waited for: select waits)
        if (int rc = accum_buffer(a->sel_mask, (size_t)n)) return rc;
        if (int rc = accum_wait(a)) return rc;
        if (n) HIP_TRY(hipMemcpy(a->sel_mask, sel->mask, (size_t)n, hipMemcpyHostToDevice));
    }
    a->stream = (hipStream_t)stream;
    SelectOut so{0ull, 0ull, INT32_MAX, 0, INT32_MAX, 0};
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(a->sel_out, &so, sizeof so, hipMemcpyHostToDevice, a->stream));
        const uint8_t *mask = sel->mask ? a->sel_mask : nullptr;
        // (the variance form reads the reported moments through the mark sums' argument, and no mark)
        const float *ms = variance ? a->moments : a->has_mark ? a->mark_sums : nullptr;
        const int32_t *mc = !variance && a->has_mark ? a->mark_counts : nullptr;
        const auto count_kernel = variance ? &rt_select_kernel<false, true> : &rt_select_kernel<false>;
        const auto write_kernel = variance ? &rt_select_kernel<true, true> : &rt_select_kernel<true>;
        hipLaunchKernelGGL(count_kernel, dim3((unsigned)nb), dim3(256), 0, a->stream, a->geom, rule, (const uint4 *)a->chain,
                           (const float *)a->sums, ms, mc, mask, a->sel_blocks, a->sel_list, (SelectOut *)a->sel_out);
        hipLaunchKernelGGL(rt_select_scan_kernel, dim3(1), dim3(256), 0, a->stream, a->sel_blocks, nb);
        hipLaunchKernelGGL(write_kernel, dim3((unsigned)nb), dim3(256), 0, a->stream, a->geom, rule, (const uint4 *)a->chain,
                           (const float *)a->sums, ms, mc, mask, a->sel_blocks, a->sel_list, (SelectOut *)a->sel_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&so, a->sel_out, sizeof so, hipMemcpyDeviceToHost, a->stream));
        if (int rc = accum_wait(a)) return rc;
    } else {
        so.next_min = so.next_max = a->samples;
    }
    a->sel_n = (long long)so.n_selected;
    a->sel_samples = so.samples;
    a->sel_target = rule.target;
    a->sel_min = so.next_min;
    a->sel_max = so.next_max;
    a->sel_from = so.from_min;
    a->sel_pending = true;
    if (n_selected) *n_selected = a->sel_n;
    return RT_OK;
}

int rt_accum_select(rt_accum *a, const rt_select *sel, void *stream, int64_t *n_selected) {
    return accum_select(a, sel, stream, n_selected, "rt_accum_select", false);
}

int rt_accum_select_variance(rt_accum *a, const rt_select *sel, void *stream, int64_t *n_selected) {
    return accum_select(a, sel, stream, n_selected, "rt_accum_select_variance", true);
}

int rt_accum_selection(rt_accum *a, int32_t *out_pixels) {
    if (!a || !out_pixels) return rt_fail(RT_ERR_ARG, "rt_accum_selection: NULL argument");
    if (int rc = accum_stale(a, "rt_accum_selection")) return rc;
    if (!a->sel_pending) return rt_fail(RT_ERR_ARG, "rt_accum_selection: no pending selection (rt_accum_select first)");
    return accum_read_back(a, &rt_accum::sel_list, (size_t)a->sel_n * sizeof(int32_t), out_pixels);
}

int rt_accum_add_selected(rt_accum *a, void *stream, rt_stats *st) {
    if (!a) return rt_fail(RT_ERR_ARG, "rt_accum_add_selected: NULL accumulator");
    if (int rc = accum_stale(a, "rt_accum_add_selected")) return rc;
    const rtap::Pass ps = rtap::plan_add_selected(*a);
    if (ps.refused) return rt_fail(ps.refused.code, ps.refused.msg);
    if (!ps.launch) {   // nothing to raise
        if (st) {
            std::memset(st, 0, sizeof *st);
            st->devices = 1;
        }
        return RT_OK;
    }
    if (int rc = accum_pass(a, ps, (hipStream_t)stream, st)) return rc;
    rtap::commit_selected(*a);
    return RT_OK;
}

int rt_accum_counts(rt_accum *a, int32_t *out) {
    if (!a || !out) return rt_fail(RT_ERR_ARG, "rt_accum_counts: NULL argument");
    return accum_read_back(a, &rt_accum::counts, (size_t)a->n_pixels * sizeof(int32_t), out, [&] {
        if (int rc = accum_buffer(a->counts, (size_t)a->n_pixels)) return rc;
        return accum_counts_launch(a, a->counts, a->stream);
    });
}

int rt_accum_counts_device(rt_accum *a, int32_t *d_out, void *stream) {
    if (!a || !d_out) return rt_fail(RT_ERR_ARG, "rt_accum_counts_device: NULL argument");
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    return accum_counts_launch(a, d_out, (hipStream_t)stream);
}

int rt_accum_sample_range(rt_accum *a, int32_t *min_out, int32_t *max_out) {
    if (!a) return rt_fail(RT_ERR_ARG, "rt_accum_sample_range: NULL accumulator");
    if (min_out) *min_out = a->min_samples;
    if (max_out) *max_out = a->samples;
    return RT_OK;
}

int32_t rt_accum_samples(const rt_accum *a) { return a ? a->samples : 0; }

int rt_accum_sums(rt_accum *a, float *out_sum) {
    if (!a || !out_sum) return rt_fail(RT_ERR_ARG, "rt_accum_sums: NULL argument");
    return accum_read_back(a, &rt_accum::sums, (size_t)a->n_pixels * 3 * sizeof(float), out_sum);
}

const float *rt_accum_device_sums(rt_accum *a) { return a ? a->sums : nullptr; }

int rt_accum_frame_u8(rt_accum *a, uint8_t *out_rgb) {
    if (!a || !out_rgb) return rt_fail(RT_ERR_ARG, "rt_accum_frame_u8: NULL argument");
    if (int rc = accum_stale(a, "rt_accum_frame_u8")) return rc;
    if (a->samples < 1) return rt_fail(RT_ERR_ARG, "rt_accum_frame_u8: no samples yet");
    if (a->n_pixels == 0) return RT_OK;
    return accum_read_back(a, &rt_accum::rgb, (size_t)a->n_pixels * 3, out_rgb, [&] {
        if (int rc = accum_buffer(a->rgb, (size_t)a->n_pixels * 3)) return rc;
        const int32_t *counts = nullptr;   // (mixed counts: every pixel divided by its own)
        if (int rc = accum_counts_if_mixed(a, &counts)) return rc;
        return counts ? rt_tonemap_u8_counts_device(a->sums, counts, a->scene->width, a->rows, a->rgb, a->stream)
                      : rt_tonemap_u8_device(a->sums, a->scene->width, a->rows, a->samples, a->rgb, a->stream);
    });
}

// Host copy of the chain buffer (after the last pass).
static int accum_records(rt_accum *a, std::vector<uint32_t> &rec) {
    rec.resize((size_t)a->n_pixels * 8);
    return accum_read_back(a, &rt_accum::chain, rec.size() * 4, rec.data());
}

int rt_accum_state(rt_accum *a, uint32_t *out) {
    if (!a || !out) return rt_fail(RT_ERR_ARG, "rt_accum_state: NULL argument");
    std::vector<uint32_t> rec;
    if (int rc = accum_records(a, rec)) return rc;
    for (long long k = 0; k < a->n_pixels; ++k) {
        const uint32_t *w = &rec[rtrec::kWords * k];
        if (a->fast_c) {   // (next sample, the open partial's three words)
            const rtfu::Rec r = rtrec::fast_unpack(w).r;
            out[4 * k + 0] = (uint32_t)r.next;
            rtrec::put3(out + 4 * k + 1, r.open);
            continue;
        }
        const rtrec::Parity q = rtrec::parity_unpack(w);
        out[4 * k + 0] = q.next;
        out[4 * k + 1] = q.state;
        out[4 * k + 2] = q.cached_avail;
        out[4 * k + 3] = rtm::f2u(q.cached);
    }
    return RT_OK;
}

// What a checkpoint header records of the scene (rt_accum_file.h).
static rtaf::SceneFacts accum_scene_facts(const rt_scene *s) {
    rtaf::SceneFacts f{s->width, s->height, s->ray_depth, (uint32_t)(s->tri.size() / 12), (uint32_t)(s->node.size() / 8),
                       (uint32_t)(s->light.size() / 16), {}};
    std::memcpy(f.cam, s->cam_pos, 12), std::memcpy(f.cam + 3, s->cam_axes, 36), std::memcpy(f.cam + 12, s->tan_half_fov, 8);
    return f;
}

int rt_accum_save(rt_accum *a, const char *path) {
    if (!a || !path) return rt_fail(RT_ERR_ARG, "rt_accum_save: NULL argument");
    if (int rc = accum_stale(a, "rt_accum_save")) return rc;   // (the header holds the camera: old sums, new camera)
    std::vector<uint32_t> rec, mom;
    if (int rc = accum_records(a, rec)) return rc;
    if (a->has_moments()) {
        mom.resize((size_t)a->n_pixels * 8);
        if (int rc = accum_read_back(a, &rt_accum::mom, mom.size() * 4, mom.data())) return rc;
    }
    auto h = rtaf::header_of(accum_scene_facts(a->scene), a->kind);
    h.rank = a->p.rank, h.world = a->p.world, h.row_block = a->p.row_block;
    h.n_pixels = a->n_pixels, h.samples = a->samples, h.pad[0] = (uint32_t)a->fast_c;
    h.reserved = a->uniform() ? 0 : 1;   // 1: per-pixel counts, `samples` is the largest
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return rt_fail(RT_ERR_IO, std::string("rt_accum_save: cannot write ") + path);
    bool ok = rtaf::write(f, h, rec, mom);
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return rt_fail(RT_ERR_IO, std::string("rt_accum_save: short write to ") + path);
    return RT_OK;
}

int rt_accum_load(rt_scene *s, int32_t device, const char *path, rt_accum **out) {
    if (!s || !path || !out) return rt_fail(RT_ERR_ARG, "rt_accum_load: NULL argument");
    *out = nullptr;
    // the file is read and checked whole before any device call; between its header and its
    // records, the shard the header names must be one of this scene with as many pixels
    const std::string who = std::string("rt_accum_load: ") + path;
    rt_accum *a = nullptr;
    const rtaf::File f = rtaf::read(path, accum_scene_facts(s), who, [&](const rtaf::File &file) -> rtp::Refusal {
        rt_params p{};
        p.rank = file.h.rank, p.world = file.h.world, p.row_block = file.h.row_block;
        p.device = device, p.fast_chunk = file.fast_c();
        if (int rc = accum_new(s, &p, "rt_accum_load", &a, file.kind)) return {rc, rt_last_error()};
        if (a->n_pixels != file.h.n_pixels)
            return {RT_ERR_ARG, who + ": " + std::to_string(file.h.n_pixels) + " pixels, the shard (rank " + std::to_string(file.h.rank) +
                                    ", world " + std::to_string(file.h.world) + ") of this scene has " + std::to_string(a->n_pixels)};
        return {};
    });
    int rc = f.refused ? rt_fail(f.refused.code, f.refused.msg) : RT_OK;
    if (rc == RT_OK) rc = ensure_device_scene(s, device);   // (the file fits the scene: first device call)
    if (rc == RT_OK) rc = accum_alloc(a);
    if (rc == RT_OK && a->n_pixels > 0) {   // the records, and their reported values as the fold kernels write them
        DeviceGuard guard(device);
        hipError_t e = hipMemcpy(a->chain, f.rec.data(), f.rec.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(a->sums, f.sums.data(), f.sums.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && a->has_moments()) {
            e = hipMemcpy(a->mom, f.mom.data(), f.mom.size() * 4, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(a->moments, f.moments.data(), f.moments.size() * 4, hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) rc = rt_fail(RT_ERR_DEVICE, std::string("rt_accum_load: ") + hipGetErrorString(e));
    }
    if (rc) {
        accum_release(a);
        return rc;
    }
    a->samples = f.hi;   // (no mark, no pending selection)
    a->min_samples = f.lo;
    *out = a;
    return RT_OK;
}

void rt_accum_free(rt_accum *a) { accum_release(a); }

// Back to what accum_create left: fresh records, zero sums and moments, no samples, no mark, no
// pending selection, no cached G-buffer; the scene's camera epoch adopted.  Kind, chunk size,
// partition, flags and buffers stay.
int rt_accum_reset(rt_accum *a, void *stream) {
    if (!a) return rt_fail(RT_ERR_ARG, "rt_accum_reset: NULL accumulator");
    if (!a->scene->dev[a->p.device]) return rt_fail(RT_ERR_ARG, "rt_accum_reset: scene not uploaded to device " + std::to_string(a->p.device));
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    if (int rc = accum_wait(a)) return rc;   // (the last pass may be on another stream)
    a->stream = (hipStream_t)stream;
    if (a->n_pixels > 0) {
        accum_init_launch(a, a->stream);
        HIP_TRY(hipGetLastError());
        if (a->has_moments()) {
            HIP_TRY(hipMemsetAsync(a->mom, 0, (size_t)a->n_pixels * 32, a->stream));
            HIP_TRY(hipMemsetAsync(a->moments, 0, (size_t)a->n_pixels * 3 * sizeof(float), a->stream));
        }
        if (int rc = accum_wait(a)) return rc;
    }
    const int fast_c = a->fast_c;
    static_cast<rtap::State &>(*a) = rtap::State{};
    a->fast_c = fast_c;
    a->gbuf_ready = false;
    a->epoch = a->scene->view_epoch;
    return RT_OK;
}

}  // extern "C"

namespace {

// The shard's first-hit records in a->gbuf on a->stream, rendered on first use (they depend on the
// scene alone; the current device is the accumulator's).
int accum_ensure_gbuffer(rt_accum *a) {
    if (int rc = accum_buffer(a->gbuf, (size_t)a->n_pixels * rtd::kGbufferQuads)) return rc;
    if (a->gbuf_ready) return RT_OK;
    if (int rc = gbuffer_launch(a->scene->dev[a->p.device], a->geom, a->gbuf, a->stream)) return rc;
    a->gbuf_ready = true;   // (set only once the records' launch was accepted: a call that fails before keeps it unset)
    return RT_OK;
}

// rt_accum_frame_u8_denoised / rt_accum_frame_u8_guided: the accumulator's frame through a filter
// in front of the finish.  check(spp, W, H) resolves the parameters before anything is allocated
// or launched; launch(counts, spp, W, H) filters a->sums into a->dn_mean on a->stream.
template <class Check, class Launch>
int accum_filtered_frame(rt_accum *a, const std::string &who, const char *frame_entry, uint8_t *out_rgb, Check check, Launch launch) {
    if (!a || !out_rgb) return rt_fail(RT_ERR_ARG, who + ": NULL argument");
    if (int rc = accum_stale(a, who)) return rc;
    if (a->p.world != 1)
        return rt_fail(RT_ERR_ARG, who + ": the filter needs the whole frame (world = 1); gather the shards' "
                                         "sums and G-buffers and use " + frame_entry);
    if (a->samples < 1) return rt_fail(RT_ERR_ARG, who + ": no samples yet");
    if (a->n_pixels == 0) return RT_OK;
    DeviceGuard guard(a->p.device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const int W = a->scene->width, H = a->rows;
    // the parameters first: a refused call allocates and launches nothing
    const int spp = a->samples;
    if (int rc = check(spp, W, H)) return rc;
    if (int rc = accum_buffer(a->dn_mean, (size_t)a->n_pixels * 3)) return rc;
    if (int rc = accum_buffer(a->rgb, (size_t)a->n_pixels * 3)) return rc;
    if (int rc = accum_ensure_gbuffer(a)) return rc;
    const int32_t *counts = nullptr;   // (mixed counts: every pixel divided by its own)
    if (int rc = accum_counts_if_mixed(a, &counts)) return rc;
    if (int rc = launch(counts, spp, W, H)) return rc;
    if (int rc = rt_tonemap_u8_device(a->dn_mean, W, H, 1, a->rgb, a->stream)) return rc;
    if (int rc = accum_wait(a)) return rc;
    HIP_TRY(hipMemcpy(out_rgb, a->rgb, (size_t)a->n_pixels * 3, hipMemcpyDeviceToHost));
    return RT_OK;
}

// A moments accumulator's measured variance into a->var on a->stream (the current device is the
// accumulator's): its own counts, and its shard's first-hit records, rendered on first use.
int accum_variance_launch(rt_accum *a) {
    if (int rc = accum_buffer(a->var, (size_t)a->n_pixels)) return rc;
    if (int rc = accum_ensure_gbuffer(a)) return rc;
    const int32_t *counts = nullptr;
    if (int rc = accum_counts_if_mixed(a, &counts)) return rc;
    return variance_launch(a->sums, a->moments, counts, a->samples, a->n_pixels, (const float *)a->gbuf, a->var, a->stream);
}

}  // namespace

extern "C" {

int rt_accum_frame_u8_denoised(rt_accum *a, const rt_denoise_params *params, uint8_t *out_rgb) {
    rtdn::Params dp;
    return accum_filtered_frame(
        a, "rt_accum_frame_u8_denoised", "rt_denoise_device", out_rgb,
        [&](int spp, int W, int H) {   // (the check only asks that its pointers are not NULL, and the sums exist)
            return rt_denoise_check("rt_accum_frame_u8_denoised", a->sums, nullptr, spp, W, H, a->sums, params, a->sums, &dp);
        },
        [&](const int32_t *counts, int spp, int W, int H) {
            return denoise_launch(&a->dn_ws, &a->dn_ws_bytes, a->sums, counts, spp, W, H, (const float *)a->gbuf, dp, a->dn_mean,
                                  a->stream);
        });
}

// rt_accum_frame_u8_guided and, with `measured`, rt_accum_frame_u8_guided_measured (`who` names the
// entry in messages): the measured form gives the filter the accumulator's own variance.
static int accum_guided_frame(rt_accum *a, const rt_denoise_guided_params *params, uint8_t *out_rgb, const char *who,
                              bool measured) {
    if (measured && a && !a->has_moments())
        return rt_fail(RT_ERR_ARG, std::string(who) + ": the accumulator keeps no moments (rt_accum_create_fast_moments)");
    rtdg::Params dp;
    return accum_filtered_frame(
        a, who, "rt_denoise_guided_device", out_rgb,
        [&](int spp, int W, int H) {
            return rt_denoise_guided_check(who, a->sums, nullptr, spp, W, H, a->sums, params, a->sums, &dp);
        },
        [&](const int32_t *counts, int spp, int W, int H) {   // (the G-buffer is rendered by now: the variance reuses it)
            if (measured)
                if (int rc = accum_variance_launch(a)) return rc;
            return denoise_guided_launch(&a->dn_ws, &a->dn_ws_bytes, a->sums, counts, spp, W, H, (const float *)a->gbuf,
                                         measured ? a->var : nullptr, dp, a->dn_mean, nullptr, a->stream);
        });
}

int rt_accum_frame_u8_guided(rt_accum *a, const rt_denoise_guided_params *params, uint8_t *out_rgb) {
    return accum_guided_frame(a, params, out_rgb, "rt_accum_frame_u8_guided", false);
}

int rt_accum_frame_u8_guided_measured(rt_accum *a, const rt_denoise_guided_params *params, uint8_t *out_rgb) {
    return accum_guided_frame(a, params, out_rgb, "rt_accum_frame_u8_guided_measured", true);
}

int rt_accum_variance(rt_accum *a, float *out) {
    if (!a || !out) return rt_fail(RT_ERR_ARG, "rt_accum_variance: NULL argument");
    if (int rc = accum_stale(a, "rt_accum_variance")) return rc;   // (it reads the cached G-buffer)
    if (!a->has_moments()) return rt_fail(RT_ERR_ARG, "rt_accum_variance: the accumulator keeps no moments (rt_accum_create_fast_moments)");
    if (a->n_pixels == 0) return RT_OK;
    return accum_read_back(a, &rt_accum::var, (size_t)a->n_pixels * sizeof(float), out, [&] { return accum_variance_launch(a); });
}

}  // extern "C"
