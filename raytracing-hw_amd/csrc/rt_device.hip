// rt_device.hip — MI355X (gfx950) render kernels and the device half of the C ABI.
//
// Kernels (the per-pixel sample loop of Scene::render, scene.cpp:31-52, and its finish):
//   rt_mega_kernel          lane-resident persistent path tracer (rt_mega.h), the default:
//                           every lane runs whole pixels, traversal one unit per iteration,
//                           shading batched per wave; also fast mode (RT_FLAG_FAST) and the
//                           counting pre-pass that orders pixels heaviest-first (rt_mega_device.h)
//   wf_{init,extend,shade}  wavefront schedule of the same arithmetic (kernel 4, rt_wavefront.h)
//   rt_finish_kernel        mean -> ACES -> gamma -> 8-bit (scene.cpp:54-64)
//   rt_finish_counts_kernel the same finish with a per-pixel sample count
//   rt_select_kernel        an accumulator's subset pass: the pixels the rule of rt_select.h
//                           chooses, as a compacted ascending list (with rt_select_scan_kernel),
//                           and rt_mark_kernel / rt_counts_kernel beside it (rt_accum_device.h)
//   rt_rays[_via]_kernel    BVH::intersect + light pdf for explicit rays, and the six *_check_kernel of
//                           rt_device_selfcheck: the test entries (rt_check_device.h)
//   rt_gbuffer_kernel       first-hit feature records from the pixel-centre rays (rt_gbuffer.h)
//   rt_denoise_{prepare,level,resolve}_kernel  the edge-avoiding a-trous filter of a frame,
//                           guided by those records (rt_denoise.h)
//   rt_denoise_guided_{window,given,level,varout}_kernel  its variance-guided mode with a
//                           firefly clamp (rt_denoise_guided.h)
//                           (these three groups, their launch functions and entries: rt_denoise_device.h)
// Every schedule writes the per-pixel float RGB sum (sample_canvas, scene.cpp:20,42) of the
// owned rows; the bits do not depend on the kernel, the launch shape, the pixel order or the
// partition.
//
// Host side of a render (launch(), below): rt_launch_plan.h decides what is launched (kernel
// instantiation, schedule, grid; host only, tested without a GPU), rt_mega_device.h holds the
// lane-resident kernel, its tuned constants and the kernel table generated from the plan's
// variant table, rt_mega.h QueueWord names the words of the queue block the host and the
// kernels share, and rt_mega_prof.h holds the diagnostics build's counters and report
// (included by rt_mega_device.h under RT_MEGA_PROF only).  The whole-frame render
// (rt_render_frame) takes its devices, row partition and buffer layout from rt_frame_plan.h
// (host only as well).  The accumulator (rt_accum_*, rt_accum_device.h) takes its kinds, parameter
// checks, host state and passes from rt_accum_plan.h, its checkpoint file from rt_accum_file.h
// (both host only) and the layout of its per-pixel records from rt_records.h.  The test entries
// (rt_device_selfcheck, rt_intersect_rays[_via], the debug build's rt_debug_*) are rt_check_device.h.
//
// Concurrency: one render per (scene, device) may be in flight at a time (the pixel queue,
// counters, vertex records and order buffers of a device copy are shared by its launches);
// renders of the same scene on different devices are independent (rt_render_multi).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rt_path.h"
#include "rt_wavefront.h"
#include <type_traits>
#include "rt_mega.h"
#include "rt_quant_lut.h"
#include "rt_scene.h"
#include "rt_material.h"
#include "rt_bvh_layout.h"
#include "rt_launch_plan.h"
#include "rt_select.h"
#include "rt_moments.h"
#include "rt_accum_plan.h"
#include "rt_accum_file.h"
#include "rt_frame_plan.h"
#include "rt_gbuffer.h"
#include "rt_denoise.h"
#include "rt_denoise_guided.h"
#include "rt_temporal.h"
#include "rt_motion.h"
#include "rt_refit.h"
#include "rt_refit_plan.h"
#include "rt_relight.h"
#include "rt_pose.h"

using rtd::Counters;
using rtd::DevScene;
using rtd::ShardGeom;
using rtd::shard_row;

// Pixel order pre-pass (launch_order).  Compile-time only, for A/B builds (make variant).
// Measured on sponza 1080p x256spp (tools/order_ab.py, profiles/r02_order_ab.jsonl): 1 spp and
// a 9 x 9 box filter (1399 ms, pre-pass 6.8 ms) against row-major order (1436 ms), 2 spp
// unfiltered (1470 ms: a noisy order loses the coherence of row-major order and gains
// nothing), 2 spp 5 x 5 (1407 ms), 8 spp 3 x 3 (1429 ms); 8-way shards, slowest of the 8:
// 346 ms against 478 ms in row-major order.  Ordering 64-pixel runs instead of pixels keeps
// rows coherent but loses the spread (8-way 476 ms).
#ifndef RT_ORDER_SPP
#define RT_ORDER_SPP 1
#endif
#ifndef RT_ORDER_RADIUS
#define RT_ORDER_RADIUS 4
#endif
constexpr int kOrderSpp = RT_ORDER_SPP;       // samples per pixel of the counting pre-pass
constexpr int kOrderRadius = RT_ORDER_RADIUS;  // box filter of the pre-pass costs ((2r+1)^2 pixels)
// The schedule rules' constants (order threshold, fast chunks, runahead and hand-off limits,
// claim stride) are rt_launch_plan.h's; the kernel itself reads the claim stride.
using rtp::kClaimStride;
constexpr int kWfRefill = 8;         // wavefront extend: idle lanes before a wave refills
constexpr unsigned kWfChunk = 64;    // wavefront extend: queue entries claimed per atomic
constexpr double kWfCompactBelow = 0.75;   // wavefront: dense queue until this active fraction

// The device image of a scene (built once on the host, copied to every device it renders on).
struct rt_device_blob {
    std::vector<uint8_t> bytes;
    size_t o_tri, o_attr, o_tan, o_node, o_light, o_lnode, o_mf, o_mt, o_nt, o_ti, o_tx, o_lut, o_mat;
    size_t n_texels;   // of the tiled texel array (rt_device_selfcheck 4)
};

struct rt_device_scene {
    int device = -1;
    void *buf = nullptr;               // one allocation holding every scene array
    DevScene ds{};
    size_t n_texels = 0;               // of ds.texels
    unsigned long long *counters = nullptr;  // rtd::kCounterWords x u64: the render's, then the order pre-pass's (kOrderCounters)
    unsigned long long *queue = nullptr;     // the queue block: rtd::kQueueWords x u64 (rt_mega.h QueueWord)
    int cu_count = 0;
    // vertex records (lane-resident) / path state and queues (wavefront)
    void *wf_buf = nullptr;
    long long wf_cap = 0;
    int wf_D = 0;
    rtd::WfState wf{};
    float4 *wf_queue[2] = {nullptr, nullptr};
    float4 *wf_hits = nullptr;
    unsigned *wf_count = nullptr;       // [0], [1]: queue counts (active rays)
    unsigned *wf_fetch = nullptr;       // extend claim counter
    unsigned *wf_host_count = nullptr;  // pinned
    float *fast_part = nullptr;         // fast mode / pre-pass: work-unit partial sums
    size_t fast_part_bytes = 0;
    // pixel order of the current render (heaviest first, spread; see launch_order)
    void *order_buf = nullptr;
    size_t order_bytes = 0;
    // rt_scene_update_tris: the new records on their way into the arrays (rt_refit_device.h)
    void *refit_stage = nullptr;
    size_t refit_stage_bytes = 0;
    void *relight_buf = nullptr;       // movable lights: light_of_tri, then the light node ids by depth
    // posable meshes (rt_pose_device.h): the rest records (five quads per triangle), and the last call's table
    void *pose_rest = nullptr;
    void *pose_table = nullptr;
    size_t pose_table_bytes = 0;
    // rt_render_frame's, kept between frames: the device's render and copy streams, two shard
    // buffers (float sums then 8-bit rows) and the events that order their reuse; on the root
    // device also the root buffer: staging, frame and row map (sizes and offsets: rt_frame_plan.h)
    struct Frame {
        hipStream_t stream = nullptr, cp_stream = nullptr;
        void *buf[2] = {nullptr, nullptr};
        size_t bytes[2] = {0, 0};
        hipEvent_t copied[2] = {nullptr, nullptr};   // copy of buffer b done (reuse after it)
        hipEvent_t finished = nullptr;               // shard finished to 8 bits (copy may start)
        hipEvent_t last = nullptr;                   // the device's last copy of the frame done
        void *root_buf = nullptr;
        size_t root_bytes = 0;
    } fr;
};

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return rt_fail(RT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

namespace {

// Restores the calling thread's current HIP device on every return path.
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// HIP events released on every return path.
struct EventSet {
    std::vector<hipEvent_t> ev;
    hipError_t make(hipEvent_t &e) {
        hipError_t r = hipEventCreate(&e);
        if (r == hipSuccess) ev.push_back(e);
        return r;
    }
    ~EventSet() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

// Device buffer that only grows (contents not kept).
hipError_t grow(void **p, size_t *cap, size_t need) {
    if (*p && *cap >= need) return hipSuccess;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(p, need ? need : 256);
    if (e == hipSuccess) *cap = need;
    return e;
}

}  // namespace

// ------------------------------------------------------------------------ kernels
// ------------------------------------------------------------------------ frame finish
// Scene::render's last loop (scene.cpp:54-64) on the device: mean, ACES (vector.h:400-407,
// same operation order as rt_tonemap_u8), saturate, then powf(v, 1/2.2) + round(clamp(*255))
// as the exact threshold count of rt_quant_lut.h (glibc powf quantizer, checked monotonic
// over every float in [0, 1] by tools/libm_check.cpp).  NaN gives 0, as on the host.
__constant__ uint32_t k_quant_thr[256];
__global__ void __launch_bounds__(256) rt_finish_kernel(const float *sum, long long n, float normalizer,
                                                         uint8_t *rgb) {
    __shared__ float thr[256];
    thr[threadIdx.x] = __uint_as_float(k_quant_thr[threadIdx.x]);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float x = sum[i];
        x *= normalizer;
        const float num = x * (x * 2.51f + 0.03f);
        const float den = x * (x * 2.43f + 0.59f) + 0.14f;
        const float v = rtv::smax(rtv::smin(num / den, 1.f), 0.f);
        int q = 0;
        if (!isnan(v)) {   // #{k in 1..255 : thr[k] <= v}, binary search (thr is non-decreasing)
            int lo = 0;    // invariant: thr[lo] <= v (thr[0] = 0 <= v for v >= 0)
#pragma unroll
            for (int step = 128; step > 0; step >>= 1)
                if (lo + step <= 255 && thr[lo + step] <= v) lo += step;
            q = lo;
        }
        rgb[i] = (uint8_t)q;
    }
}

// The same finish with a per-pixel sample count (rt_tonemap_u8_counts_device): value i belongs to
// pixel i / 3, whose sum is multiplied by 1.f / (float)count as above by 1.f / (float)spp; a pixel
// without samples gives 0, 0, 0.  Same thresholds, same NaN / inf behaviour.
__global__ void __launch_bounds__(256) rt_finish_counts_kernel(const float *sum, const int32_t *counts, long long n,
                                                                uint8_t *rgb) {
    __shared__ float thr[256];
    thr[threadIdx.x] = __uint_as_float(k_quant_thr[threadIdx.x]);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int32_t c = counts[i / 3];
        float x = sum[i];
        x *= rtsel::count_normalizer(c);
        const float num = x * (x * 2.51f + 0.03f);
        const float den = x * (x * 2.43f + 0.59f) + 0.14f;
        const float v = rtv::smax(rtv::smin(num / den, 1.f), 0.f);
        int q = 0;
        if (c > 0 && !isnan(v)) {
            int lo = 0;
#pragma unroll
            for (int step = 128; step > 0; step >>= 1)
                if (lo + step <= 255 && thr[lo + step] <= v) lo += step;
            q = lo;
        }
        rgb[i] = (uint8_t)q;
    }
}

#include "rt_mega_device.h"   // the lane-resident kernel, its tuned constants and its variant table

// Fast mode: pixel sum = partials of chunks 0, 1, ... added in order (deterministic; the
// oracle's rt_oracle_render_fast adds them the same way).  part is chunk-major: n3 floats
// per chunk.
__global__ void __launch_bounds__(256) rt_fast_reduce_kernel(const float *__restrict__ part, float *__restrict__ out,
                                                             long long n3, int chunks) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += part[(long long)c * n3 + i];
    out[i] = s;
}

// (The two fold kernels and ChainPass stay here, beside launch(), which launches them; the accumulator's rest: rt_accum_device.h.)
// A fast accumulator's pass, after its render launch: one thread per item of the pass (`items`
// lists their shard pixels, null = every pixel) folds the item's partials (unit-major: unit k of
// item i at k * n_list + i) into its record and writes the record and the pixel's reported sum
// (rt_fast_units.h fold, reported).  The only writer of fast records besides their init; pixels
// not listed, and items already at `target`, are not touched.  `units`: the launch's units per
// item (at least every item's own).
struct FastPartials {
    const float *part;
    long long n_list, i;
    RT_HD float operator()(int k, int ch) const { return part[3 * ((long long)k * n_list + i) + ch]; }
};
__global__ void __launch_bounds__(256) rt_fast_fold_chain_kernel(uint4 *chain, const int *items, long long n_list, int units,
                                                                  int c, int target, const float *__restrict__ part,
                                                                  float *sums) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_list) return;
    const long long p = items ? (long long)items[i] : i;
    rtd::FastRec q = rtd::fast_rec(chain, p);
    const int own = rtfu::units_of(q.r.next, target, c);
    if (own < 1 || own > units) return;   // (nothing rendered for it / never: the launch has the largest count)
    rtfu::fold(q.r, target, c, FastPartials{part, n_list, i});
    rtd::fast_rec_store(chain, p, q.r);
    float s[3];
    rtfu::reported(q.r, c, s);
    sums[3 * p + 0] = s[0];
    sums[3 * p + 1] = s[1];
    sums[3 * p + 2] = s[2];
}

// The fold of a moments accumulator's pass (rt_moments.h): the same fold on both partial sets, the
// sums' at `part` and the squares' at part + 3 * n_list * units, into the fast record and the
// moment record (mom: 32 bytes per pixel, rt_records.h), and both reported values.  The
// moment record's `next` is the fast record's, so both folds see the same units.  Pixels not
// listed, and items already at `target`, are not touched.
__global__ void __launch_bounds__(256) rt_fast_fold_moments_kernel(uint4 *chain, uint4 *mom, const int *items, long long n_list,
                                                                    int units, int c, int target, const float *__restrict__ part,
                                                                    float *sums, float *moments) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_list) return;
    const long long p = items ? (long long)items[i] : i;
    rtd::FastRec q = rtd::fast_rec(chain, p);
    const int own = rtfu::units_of(q.r.next, target, c);
    if (own < 1 || own > units) return;
    rtfu::Rec m;
    m.next = q.r.next;
    rtd::moment_rec(mom, p, m);
    rtfu::fold(q.r, target, c, FastPartials{part, n_list, i});
    rtfu::fold(m, target, c, FastPartials{part + 3 * n_list * (long long)units, n_list, i});
    rtd::fast_rec_store(chain, p, q.r);
    rtd::moment_rec_store(mom, p, m);
    float s[3], s2[3];
    rtfu::reported(q.r, c, s);
    rtfu::reported(m, c, s2);
    for (int ch = 0; ch < 3; ++ch) {
        sums[3 * p + ch] = s[ch];
        moments[3 * p + ch] = s2[ch];
    }
}

// Pixel order, step 1: the sort's values (shard pixel ids) and keys (pre-pass costs).
__global__ void __launch_bounds__(256) rt_order_iota_kernel(int *ids, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = (int)i;
}

// Pixel order, optional smoothing: box sums of the pre-pass costs over (2r+1) shard pixels
// along a row (dir 0) or down a column (dir 1) of the shard's rows x width grid.
__global__ void __launch_bounds__(256) rt_order_box_kernel(const unsigned *in, unsigned *out, long long n, int width,
                                                           int r, int dir) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const long long rows = n / width, k = p / width, i = p % width;
    unsigned s = 0;
    for (int d = -r; d <= r; ++d) {
        const long long kk = dir ? k + d : k, ii = dir ? i : i + d;
        if (kk >= 0 && kk < rows && ii >= 0 && ii < width) s += in[kk * width + ii];
    }
    out[p] = s;
}

// Pixel order, step 2: `sorted` holds the shard pixels heaviest first.  The first claims of
// the render (each of the `groups` waves takes `per` consecutive queue items at its start, one
// pixel per lane, all lanes at once) get the heaviest m = min(n, groups * per) pixels, spread
// so that every wave holds one pixel of every cost stratum: queue item gi * per + j gets rank
// r = j * a + min(j, b) + gi (m = a * per + b: the ranks in (lane j, wave gi) order of the
// items that exist).  A heavy pixel's wave-mates are then light and finish early, and its
// sequential sample chain runs in a sparse wave.  Later claims stay heaviest-first.
__global__ void __launch_bounds__(256) rt_order_spread_kernel(const int *sorted, int *order, long long n,
                                                              long long groups, long long per) {
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const long long m = n < groups * per ? n : groups * per;
    long long r = q;
    if (q < m) {
        const long long gi = q / per, j = q % per, a = m / per, b = m % per;
        r = j * a + (j < b ? j : b) + gi;
    }
    order[q] = sorted[r];
}

// Hand-off, between the two launches: the sort keys of the park list's slots, the work a
// parked pixel has left as (samples left) x (its pre-pass estimate + 1); 0 for an empty slot.
// The slots sorted by it, heaviest first, then go through rt_order_spread_kernel, so that the
// runahead launch deals the parked pixels with the most work left one per wave.
__global__ void __launch_bounds__(256) rt_park_keys_kernel(const uint4 *park, long long n, int spp, const unsigned *est,
                                                           unsigned *keys, int *ids) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rtd::Parked q = rtd::parked(park, i);
    unsigned long long k = 0;
    if (q.pix != rtd::kNoPark) k = (unsigned long long)(spp - (int)q.s) * ((unsigned long long)est[q.pix] + 1ull);
    keys[i] = k > 0xffffffffull ? 0xffffffffu : (unsigned)k;
    ids[i] = (int)i;
}
// One 64-bit word, in stream order (the resume map's address in the queue block).
__global__ void rt_set_u64_kernel(unsigned long long *dst, unsigned long long v) { *dst = v; }

// ------------------------------------------------------------------------ wavefront (kernel 4)
// (rt_wavefront.h) init -> { extend ; shade } until every slot has finished its samples.
// Queue modes.  Dense: entry p holds slot p's ray, or an inactive marker (slot -1) once that
// pixel has all its samples; the order never changes, so a wave's lanes keep neighbouring
// pixels (coherent camera rays, coalesced slot-state access) for the whole frame.  Compact:
// active rays only, appended with one atomic per wave; used for the tail of the frame, when
// most slots are finished.  In both modes *count is the number of active rays (the host's
// termination test).
__global__ void __launch_bounds__(256) wf_init_kernel(DevScene sc, ShardGeom g, rtd::WfState st, long long n,
                                                       float4 *qout, unsigned *cout) {
    for (long long base = (long long)blockIdx.x * blockDim.x; base < n; base += (long long)gridDim.x * blockDim.x) {
        const long long i = base + threadIdx.x;
        const bool valid = i < n;
        if (valid) rtd::store_qray(sc, qout, (unsigned)i, (int)i, rtd::wf_init_slot(sc, g, st, i));
        rtd::queue_slot(valid, cout);   // active count
    }
}

// Persistent traversal over the queue: each loop iteration advances every lane of a wave
// by one unit of its own ray's traversal (rt_wavefront.h trav_step).  Lanes whose ray is
// finished idle until kWfRefill of them are idle (or the wave has nothing else to do), then
// take the next rays of the wave's current chunk of the queue; a wave claims a new chunk of
// kWfChunk entries with one atomic when its chunk runs out.  Exit: the claim counter is
// monotonic, so every wave stops claiming once it passes the end and leaves when its lanes
// are done.
template <bool COUNT>
__global__ void __launch_bounds__(256) wf_extend_kernel(DevScene sc, const float4 *qin, const unsigned *count,
                                                         unsigned npos, float4 *hits, unsigned *fetch,
                                                         unsigned *next_count, unsigned long long *counters) {
    const unsigned n = npos ? npos : *count;   // queue positions (dense: all slots)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&counters[7], (unsigned long long)n);  // rays extended
        *next_count = 0;                                 // the shade kernel's output queue
    }
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    uint2 spill[rtd::kStack - rtd::kLdsStackWf];
    rtd::LdsStackT<rtd::kLdsStackWf> S{spill};
    const int lane = threadIdx.x & 63;
    const rtd::GlobalNodes nodes{sc.node};
    const rtd::NodeRec root = rtd::load_node(sc.node, 0);
    unsigned q = 0, lo = 0, hi = 0;   // [lo, hi): the wave's unclaimed part of its chunk
    bool busy = false, exhausted = false;
    rtd::Ray r;
    rtd::TravState T;
    for (;;) {
        const unsigned long long m = __ballot(!busy);
        const unsigned idle = (unsigned)__popcll(m);
        if (!exhausted && (idle >= (unsigned)kWfRefill || idle == 64)) {
            const unsigned rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            unsigned got = 0, mine = 0xffffffffu;
            while (got < idle) {
                if (lo >= hi) {
                    unsigned b = 0;
                    if (lane == 0) b = atomicAdd(fetch, kWfChunk);
                    b = __shfl(b, 0, 64);
                    if (b >= n) {
                        exhausted = true;
                        break;
                    }
                    lo = b;
                    hi = b + kWfChunk < n ? b + kWfChunk : n;
                }
                const unsigned k = hi - lo < idle - got ? hi - lo : idle - got;
                if (!busy && rank >= got && rank < got + k) mine = lo + (rank - got);
                lo += k;
                got += k;
            }
            if (mine != 0xffffffffu) {
                q = mine;
                uint32_t bits;
                int slot;
                r = rtd::load_qray_trav(qin, q, bits, slot);
                if (slot >= 0) {   // (dense queue: inactive entries are skipped)
                    busy = rtd::trav_start<COUNT>(bits, root.a, root.b, T, cnt);
                    if (!busy) rtd::store_hit(hits, q, T.best);   // misses the scene box
                }
            }
        }
        // (every best frame, as before RT_ACC_ELIDE: this kernel was not measured with it)
        if (busy && rtd::trav_step<COUNT, rtd::kFarDist2, false>(sc, r, T, S, nodes, cnt)) {
            rtd::store_hit(hits, q, T.best);
            busy = false;
        }
        if (exhausted && !__any(busy)) break;
    }
    rtd::counters_flush<COUNT>(cnt, counters);
}

// Per-block LDS copies of the small tables every shading hit reads with a lane-dependent
// index (texel decode LUT, materials): LDS reads instead of divergent vector-memory gathers.
constexpr int kMatLds = 64;
struct ShadeLds {
    float lut[512];
    float mf[kMatLds * 12];
    int mt[kMatLds * 4];
    double nt[kMatLds * 16];
};

template <bool COUNT, bool MAT_LDS>
__global__ void __launch_bounds__(256) wf_shade_kernel(DevScene sc_in, ShardGeom g, rtd::WfState st, int spp,
                                                        const float4 *qin, const unsigned *cin, unsigned npos,
                                                        const float4 *hits, float4 *qout, unsigned *cout,
                                                        int dense_out, unsigned *fetch, float *out,
                                                        unsigned long long *counters) {
    __shared__ ShadeLds L;
    for (int k = threadIdx.x; k < 512; k += blockDim.x) L.lut[k] = sc_in.lut[k];
    if (MAT_LDS) {
        for (int k = threadIdx.x; k < sc_in.n_meshes * 12; k += blockDim.x) L.mf[k] = sc_in.mesh_f[k];
        for (int k = threadIdx.x; k < sc_in.n_meshes * 4; k += blockDim.x) L.mt[k] = sc_in.mesh_tex[k];
        for (int k = threadIdx.x; k < sc_in.n_meshes * 16; k += blockDim.x) L.nt[k] = sc_in.mesh_nt[k];
    }
    __syncthreads();
    DevScene sc = sc_in;
    sc.lut = L.lut;
    if (MAT_LDS) {
        sc.mesh_f = L.mf;
        sc.mesh_tex = L.mt;
        sc.mesh_nt = L.nt;
    }
    const unsigned n = npos ? npos : *cin;   // input positions (dense: all slots)
    if (blockIdx.x == 0 && threadIdx.x == 0) *fetch = 0;   // the next extend launch's claim counter
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    for (unsigned base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {
        const unsigned q = base + threadIdx.x;
        int slot = -1;
        bool next = false;
        rtd::Ray r;
        if (q < n) {
            r = rtd::load_qray(qin, q, slot);
            if (slot >= 0) {
                const rtd::Hit h = rtd::load_hit(hits, q);
                next = rtd::wf_shade_slot<COUNT>(sc, g, st, spp, slot, r, h, out, cnt);
            }
        }
        const unsigned p = rtd::queue_slot(next, cout);
        if (dense_out) {   // (dense out implies dense in: entry q is slot q)
            if (next) rtd::store_qray(sc, qout, q, slot, r);
            else if (q < n) rtd::store_qray_inactive(qout, q);
        } else if (next) {
            rtd::store_qray(sc, qout, p, slot, r);
        }
    }
    rtd::counters_flush<COUNT>(cnt, counters);
}

// ------------------------------------------------------------------------ host side
namespace {

template <class T>
size_t append(std::vector<uint8_t> &blob, const std::vector<T> &v, size_t pre = 0) {
    size_t off = rtp::align_up(blob.size()) + pre;
    blob.resize(off + v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

// The device image of the scene, built once per scene (every device copies the same bytes).
int ensure_blob(rt_scene *s) {
    if (s->blob) return RT_OK;
    if (s->bvh_depth + 2 >= (uint32_t)rtd::kStack || s->light_bvh_depth + 2 >= (uint32_t)rtd::kStack)
        return rt_fail(RT_ERR_LIMIT, "BVH deeper than the device traversal stack (" + std::to_string(rtd::kStack) + ")");
    if (s->ray_depth > rtd::kMaxDepth) return rt_fail(RT_ERR_LIMIT, "ray_depth exceeds device limit");
    for (size_t k = 0; k < s->node.size() / 8; ++k) {  // traversal frame packing (rt_wavefront.h)
        uint32_t a, b;
        std::memcpy(&a, &s->node[8 * k + 6], 4);
        std::memcpy(&b, &s->node[8 * k + 7], 4);
        if (a >= rtd::kFrameMaxA || b >= 1024u)
            return rt_fail(RT_ERR_LIMIT, "scene too large for the device BVH frame packing (2^22 nodes/triangles, 255 per leaf)");
    }
    auto *b = new rt_device_blob();
    std::vector<uint8_t> &blob = b->bytes;
    // The device copy of the scene BVH is renumbered breadth-first (rt_bvh_layout.h): a
    // node's children stay an adjacent pair (right = left + 1) and leaves keep their triangle
    // ranges, so traversal visits, counters and results are unchanged.  It starts at +32 B so
    // a sibling pair (left odd, left + 1) shares one 64-B line.  Every array starts 256-B
    // aligned: a leaf lane's 4 x 16-B read of the last triangle stays inside the allocation.
    b->o_tri = append(blob, s->tri);
    b->o_attr = append(blob, s->tri_attr);
    b->o_tan = append(blob, s->tri_tan);
    b->o_node = append(blob, rtd::bfs_nodes(s->node, &s->bfs_order), 32);   // (the order: rt_refit_plan.h)
    b->o_light = append(blob, s->light);
    b->o_lnode = append(blob, s->light_node);
    b->o_mf = append(blob, s->mesh_f);
    b->o_mt = append(blob, s->mesh_tex);
    b->o_nt = append(blob, s->mesh_nt);
    // textures in 4x4-texel tiles (64 B, one cache line): a bilinear 2x2 footprint usually
    // stays in one line instead of always spanning two rows (rt_path.h tex_sample)
    std::vector<uint32_t> tinfo, tiled;
    rtmat::tile_textures(s->tex_info, s->texels, tinfo, tiled);
    b->o_ti = append(blob, tinfo);
    b->o_tx = append(blob, tiled);
    b->n_texels = tiled.size();
    std::vector<float> lut(512);
    rtd::fill_decode_lut(lut.data());
    b->o_lut = append(blob, lut);
    // per-mesh material records (rt_material.h): 128 B each, 128-B aligned (every array starts
    // 256-B aligned), descriptors of the tiled layout inline
    std::vector<uint32_t> mat;
    if (!rtmat::build_records(s->mesh_f.data(), s->mesh_tex.data(), s->mesh_f.size() / 12, tinfo.data(), tinfo.size() / 4, mat)) {
        delete b;
        return rt_fail(RT_ERR_FORMAT, "texture index out of range");
    }
    b->o_mat = append(blob, mat);
    blob.resize(rtp::align_up(blob.size()) + 256);
    s->blob = b;
    return RT_OK;
}

// The device copies that exist (rt_device_selfcheck 4 checks the material records of each).
std::mutex g_live_mu;
std::vector<rt_device_scene *> g_live;

void free_device_scene(rt_device_scene *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.erase(std::remove(g_live.begin(), g_live.end(), d), g_live.end());
    }
    DeviceGuard guard(d->device);
    if (guard.ok) {
        for (hipStream_t q : {d->fr.stream, d->fr.cp_stream})
            if (q) (void)hipStreamSynchronize(q);
        for (void *p : {d->buf, (void *)d->counters, (void *)d->queue, d->wf_buf, (void *)d->wf_count,
                        (void *)d->wf_fetch, (void *)d->fast_part, d->order_buf, d->refit_stage, d->relight_buf, d->pose_rest, d->pose_table, d->fr.buf[0], d->fr.buf[1], d->fr.root_buf})
            if (p) (void)hipFree(p);
        if (d->wf_host_count) (void)hipHostFree(d->wf_host_count);
        for (hipEvent_t e : {d->fr.copied[0], d->fr.copied[1], d->fr.finished, d->fr.last})
            if (e) (void)hipEventDestroy(e);
        for (hipStream_t q : {d->fr.stream, d->fr.cp_stream})
            if (q) (void)hipStreamDestroy(q);
    }
    delete d;
}

// rt_render_frame's per-device streams and events (created once per device copy).
hipError_t ensure_frame_streams(rt_device_scene *d) {
    hipError_t e = hipSuccess;
    if (!d->fr.stream) e = hipStreamCreateWithFlags(&d->fr.stream, hipStreamNonBlocking);
    if (e == hipSuccess && !d->fr.cp_stream) e = hipStreamCreateWithFlags(&d->fr.cp_stream, hipStreamNonBlocking);
    for (hipEvent_t *ev : {&d->fr.copied[0], &d->fr.copied[1], &d->fr.finished, &d->fr.last})
        if (e == hipSuccess && !*ev) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    return e;
}

int pose_rest_upload(rt_scene *s, rt_device_scene *d);   // rt_pose_device.h

int ensure_device_scene(rt_scene *s, int device) {
    if (device < 0 || device >= kRtMaxDevices) return rt_fail(RT_ERR_DEVICE, "no HIP device " + std::to_string(device));
    if (s->dev[device]) return RT_OK;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device >= ndev) return rt_fail(RT_ERR_DEVICE, "no HIP device " + std::to_string(device));
    int rc = ensure_blob(s);
    if (rc) return rc;
    const rt_device_blob &b = *s->blob;
    DeviceGuard guard(device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice(" + std::to_string(device) + ") failed");
    rt_device_scene *d = new rt_device_scene();
    d->device = device;
    hipError_t e = hipMalloc(&d->buf, b.bytes.size());
    if (e == hipSuccess) e = hipMemcpy(d->buf, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&d->counters, rtd::kCounterWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&d->queue, rtd::kQueueWords * sizeof(unsigned long long));
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        free_device_scene(d);
        return rt_fail(RT_ERR_DEVICE, std::string("scene upload: ") + hipGetErrorString(e));
    }
    d->cu_count = prop.multiProcessorCount;
    uint8_t *base = (uint8_t *)d->buf;
    DevScene &ds = d->ds;
    ds.tri = (const float4 *)(base + b.o_tri);
    ds.tri_attr = (const float4 *)(base + b.o_attr);
    ds.tri_tan = (const float4 *)(base + b.o_tan);
    ds.node = (const float4 *)(base + b.o_node);
    ds.light = (const float4 *)(base + b.o_light);
    ds.light_node = (const float4 *)(base + b.o_lnode);
    ds.mesh_f = (const float *)(base + b.o_mf);
    ds.mesh_tex = (const int *)(base + b.o_mt);
    ds.mesh_nt = (const double *)(base + b.o_nt);
    ds.tex_info = (const uint4 *)(base + b.o_ti);
    ds.texels = (const uint32_t *)(base + b.o_tx);
    ds.lut = (const float *)(base + b.o_lut);
    d->n_texels = b.n_texels;
#if RT_SHADE_GATHER
    ds.mat = (const uint4 *)(base + b.o_mat);
    ds.any_nmap = 0;
    for (size_t m = 0; m < s->mesh_tex.size() / 4; ++m) ds.any_nmap |= s->mesh_tex[4 * m + 1] >= 0;
#endif
    ds.n_lights = (int)(s->light.size() / 16);
    ds.n_tris = (int)(s->tri.size() / 12);
    ds.n_nodes = (int)(s->node.size() / 8);
    ds.n_meshes = (int)(s->mesh_f.size() / 12);
    ds.ray_depth = s->ray_depth;
    ds.max_distance = s->max_distance;
    ds.width = s->width;
    ds.height = s->height;
    ds.fwidth = (float)s->width;
    ds.fheight = (float)s->height;
    std::memcpy(ds.cam_pos, s->cam_pos, sizeof ds.cam_pos);
    std::memcpy(ds.cam_axes, s->cam_axes, sizeof ds.cam_axes);
    std::memcpy(ds.tan_fov, s->tan_half_fov, sizeof ds.tan_fov);
    if (s->poses_on)   // a posable scene's copy holds the rest records from the start
        if (int prc = pose_rest_upload(s, d)) {
            free_device_scene(d);
            return prc;
        }
    s->dev[device] = d;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.push_back(d);
    }
    return RT_OK;
}

// Workspace: wavefront path state for `n` slots, or the lane-resident kernel's vertex
// records for `n` lane slots, `D` vertices each.
int ensure_wf(rt_device_scene *d, long long n, int D) {
    if (d->wf_buf && d->wf_cap >= n && d->wf_D == D) return RT_OK;
    if (d->wf_buf) (void)hipFree(d->wf_buf);
    d->wf_buf = nullptr;
    d->wf_cap = 0;
    const long long cap = ((n + 255) / 256) * 256;
    const int planes = 8 + 9 * D + 20         // slot state (2 x 16 B), vertex records (36 B each), light-split mid (80 B)
                       + 2 * 4 * rtd::kQRec + 4;   // two ray queues (48 B / entry), hits (16 B / entry)
    const size_t bytes = (size_t)cap * 4 * (size_t)planes;
    HIP_TRY(hipMalloc(&d->wf_buf, bytes));
    if (!d->wf_count) HIP_TRY(hipMalloc((void **)&d->wf_count, 16));
    if (!d->wf_fetch) HIP_TRY(hipMalloc((void **)&d->wf_fetch, 16));
    if (!d->wf_host_count) HIP_TRY(hipHostMalloc((void **)&d->wf_host_count, 16, hipHostMallocDefault));
    float *f = (float *)d->wf_buf;
    auto take = [&](long long k) { float *p = f; f += (size_t)cap * k; return p; };
    rtd::WfState &w = d->wf;
    w.n = n;
    w.D = D;
    d->wf_queue[0] = (float4 *)take(4 * rtd::kQRec);   // 16-B aligned: cap is a multiple of 256
    d->wf_queue[1] = (float4 *)take(4 * rtd::kQRec);
    d->wf_hits = (float4 *)take(4);
    w.st = (float4 *)take(8);
    w.rec_ab = (float4 *)take(8 * D);
    w.rec_c = take(D);
    w.mid = (float4 *)take(20);   // 5 planes of float4, stride = lane slots (<= cap)
    {   // the hand-off's park list (32 B per lane slot) is the first ray queue (48 B per slot, unused
        // by the lane-resident kernels); its address goes where the kernel reads it
        const unsigned long long park = (unsigned long long)(uintptr_t)d->wf_queue[0];
        HIP_TRY(hipMemcpy(d->queue + rtd::kQueueParkList, &park, sizeof park, hipMemcpyHostToDevice));
    }
    d->wf_cap = cap;
    d->wf_D = D;
    return RT_OK;
}

// 256-thread blocks of `kernel` the device holds at once.
template <class K>
long long resident_blocks(rt_device_scene *d, K kernel) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    return (long long)d->cu_count * per_cu;
}
template <class K>
unsigned persistent_blocks(rt_device_scene *d, K kernel, long long work) {
    const long long need = (work + 255) / 256;
    const long long b = std::min<long long>(need, resident_blocks(d, kernel));
    return (unsigned)std::max<long long>(b, 1);
}

// Per-launch HIP events for RT_FLAG_KERNEL_TIMES (wavefront path).
struct LaunchTimer {
    bool on = false;
    std::vector<hipEvent_t> ev[2];   // [kernel]: start, end, start, end, ...
    hipError_t mark(int k, hipStream_t s) {
        if (!on) return hipSuccess;
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev[k].push_back(e);
        return hipEventRecord(e, s);
    }
    // sums the durations (after the stream has drained) and releases the events
    hipError_t collect(double ms[2], uint64_t n[2]) {
        hipError_t r = hipSuccess;
        for (int k = 0; k < 2; ++k) {
            ms[k] = 0.0;
            n[k] = ev[k].size() / 2;
            for (size_t j = 0; j + 1 < ev[k].size(); j += 2) {
                float t = 0.f;
                if (r == hipSuccess) r = hipEventElapsedTime(&t, ev[k][j], ev[k][j + 1]);
                ms[k] += t;
            }
            for (hipEvent_t e : ev[k]) (void)hipEventDestroy(e);
            ev[k].clear();
        }
        return r;
    }
    ~LaunchTimer() {
        for (auto &v : ev)
            for (hipEvent_t e : v) (void)hipEventDestroy(e);
    }
};

int launch_wavefront(rt_device_scene *d, const ShardGeom &g, int spp, int depth, float *d_out, hipStream_t stream,
                     bool count, LaunchTimer &timer) {
    if (depth < 1 || depth > 15) return rt_fail(RT_ERR_LIMIT, "wavefront path: ray_depth must be in [1, 15]");
    if (spp >= (1 << 20)) return rt_fail(RT_ERR_LIMIT, "wavefront path: spp must be < 2^20");
    if (g.n_pixels >= (1LL << 31)) return rt_fail(RT_ERR_LIMIT, "wavefront path: shards below 2^31 pixels");
    int rc = ensure_wf(d, g.n_pixels, depth);
    if (rc) return rc;
    rtd::WfState w = d->wf;
    w.n = g.n_pixels;
    const long long n = g.n_pixels;
    HIP_TRY(hipMemsetAsync(d->wf_count, 0, 16, stream));
    HIP_TRY(hipMemsetAsync(d->wf_fetch, 0, 16, stream));
    auto extend = count ? wf_extend_kernel<true> : wf_extend_kernel<false>;
    const unsigned ext_blocks = persistent_blocks(d, extend, n);
    const bool mat_lds = d->ds.n_meshes <= kMatLds;
    auto shade = count ? (mat_lds ? wf_shade_kernel<true, true> : wf_shade_kernel<true, false>)
                       : (mat_lds ? wf_shade_kernel<false, true> : wf_shade_kernel<false, false>);
    const unsigned sh_blocks = persistent_blocks(d, shade, n);
    const unsigned init_blocks = (unsigned)std::min<long long>((n + 255) / 256, (long long)d->cu_count * 8);
    hipLaunchKernelGGL(wf_init_kernel, dim3(init_blocks), dim3(256), 0, stream, d->ds, g, w, n, d->wf_queue[0],
                       &d->wf_count[0]);
    HIP_TRY(hipGetLastError());
    bool dense = true, to_compact = false;
    const long long max_iter = (long long)spp * depth + 16;
    int cur = 0;
    for (long long it = 0;; ++it) {
        if (it > max_iter) return rt_fail(RT_ERR_DEVICE, "wavefront path did not drain (internal error)");
        float4 *qi = d->wf_queue[cur], *qo = d->wf_queue[1 - cur];
        const unsigned npos = dense ? (unsigned)n : 0u;
        HIP_TRY(timer.mark(0, stream));
        hipLaunchKernelGGL(extend, dim3(ext_blocks), dim3(256), 0, stream, d->ds, qi, &d->wf_count[cur], npos,
                           d->wf_hits, d->wf_fetch, &d->wf_count[1 - cur], d->counters);
        HIP_TRY(timer.mark(0, stream));
        HIP_TRY(timer.mark(1, stream));
        const int dense_out = dense && !to_compact;
        hipLaunchKernelGGL(shade, dim3(sh_blocks), dim3(256), 0, stream, d->ds, g, w, spp, qi, &d->wf_count[cur], npos,
                           d->wf_hits, qo, &d->wf_count[1 - cur], dense_out, d->wf_fetch, d_out, d->counters);
        if (to_compact) dense = false;
        HIP_TRY(timer.mark(1, stream));
        HIP_TRY(hipGetLastError());
        cur = 1 - cur;
        if ((it & 7) == 7) {   // active rays: done at 0; compact once below kWfCompactBelow
            HIP_TRY(hipMemcpyAsync(d->wf_host_count, &d->wf_count[cur], 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (d->wf_host_count[0] == 0) break;
            if (dense && (double)d->wf_host_count[0] < kWfCompactBelow * (double)n) to_compact = true;
        }
    }
    return RT_OK;
}

// The order buffer of a device copy (d->order_buf): five arrays of one 4-byte entry per shard
// pixel, each 256-byte aligned, then the radix sort's scratch.  launch_order fills them: the
// pre-pass costs (box-filtered through cost_sorted, back into cost), their descending sort
// (cost_sorted, ids -> sorted) and the spread into `order`, which the main launch reads.
// The hand-off's second sort runs after the main launch, when `order` and everything but the
// filtered costs is dead, and reuses the arrays: cost stays the estimate it sorts by, its keys
// go to cost_sorted and their sorted copy over `order`, ids / sorted hold the park-list slots,
// and the resume map takes the keys' array once they are sorted.
struct OrderBuf {
    unsigned *cost, *cost_sorted;
    int *ids, *sorted, *order;
    void *tmp;
    // the hand-off's names for the arrays it reuses
    unsigned *park_keys, *park_keys_sorted;
    int *resume_map;
    static size_t array_bytes(long long n) { return rtp::align_up((size_t)n * 4); }
    static size_t bytes(long long n, size_t tmp_bytes) { return 5 * array_bytes(n) + tmp_bytes; }
    OrderBuf(void *base, long long n_pixels) {
        uint8_t *b = (uint8_t *)base;
        const size_t arr = array_bytes(n_pixels);
        cost = (unsigned *)b;
        cost_sorted = park_keys = (unsigned *)(b + arr);
        ids = (int *)(b + 2 * arr);
        sorted = (int *)(b + 3 * arr);
        order = (int *)(b + 4 * arr);
        tmp = b + 5 * arr;
        park_keys_sorted = (unsigned *)order;
        resume_map = (int *)park_keys;
    }
};

// Heaviest-first, spread pixel order for a parity-mode render of shard g, built inside the
// frame: a counting fast-mode pre-pass of kOrderSpp samples per pixel measures each pixel's
// traversal work (its own Philox streams: the pre-pass never touches the render's RNG), a
// box filter turns that into an estimate of the pixel's expected work, a radix sort ranks
// the pixels by it, and rt_order_spread_kernel deals the heaviest ones out over the render's
// `groups` waves.  Results never depend on the order; it only shortens the
// frame's tail.  Returns the order in d_order.
int launch_order(rt_device_scene *d, const ShardGeom &g, hipStream_t stream, long long groups, long long per,
                 const int **d_order) {
    const long long n = g.n_pixels;
    size_t tmp_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, (unsigned *)nullptr, (unsigned *)nullptr,
                                                         (int *)nullptr, (int *)nullptr, (int)n, 0, 32, stream));
    HIP_TRY(grow(&d->order_buf, &d->order_bytes, OrderBuf::bytes(n, tmp_bytes)));
    const OrderBuf ob(d->order_buf, n);
    HIP_TRY(grow((void **)&d->fast_part, &d->fast_part_bytes, (size_t)n * 3 * sizeof(float)));
    HIP_TRY(hipMemsetAsync(d->queue + rtd::kQueueOrder, 0, sizeof(unsigned long long), stream));
    rtp::Variant counting_fast;
    counting_fast.count = counting_fast.fast = true;
    const MegaKernel pre = mega_kernel_of(counting_fast);
    const unsigned blocks = persistent_blocks(d, pre, n);   // <= ceil(n / 256): lane slots fit the workspace
    rtd::WfState w = d->wf;
    w.n = n;
    w.lanes = (long long)blocks * 256;
    hipLaunchKernelGGL(pre, dim3(blocks), dim3(256), 0, stream, d->ds, g, w, kOrderSpp, d->fast_part,
                       d->counters + rtd::kOrderCounters, d->queue + rtd::kQueueOrder, (const int *)nullptr, ob.cost,
                       kOrderSpp, 0);
    HIP_TRY(hipGetLastError());
    const unsigned nb = (unsigned)((n + 255) / 256);
    if (kOrderRadius > 0) {   // box-filtered costs: the pixel's neighbourhood estimates its expected work
        hipLaunchKernelGGL(rt_order_box_kernel, dim3(nb), dim3(256), 0, stream, (const unsigned *)ob.cost, ob.cost_sorted, n,
                           g.width, kOrderRadius, 0);
        hipLaunchKernelGGL(rt_order_box_kernel, dim3(nb), dim3(256), 0, stream, (const unsigned *)ob.cost_sorted, ob.cost, n,
                           g.width, kOrderRadius, 1);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(rt_order_iota_kernel, dim3(nb), dim3(256), 0, stream, ob.ids, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(ob.tmp, tmp_bytes, ob.cost, ob.cost_sorted, ob.ids, ob.sorted, (int)n,
                                                         0, 32, stream));
    hipLaunchKernelGGL(rt_order_spread_kernel, dim3(nb), dim3(256), 0, stream, (const int *)ob.sorted, ob.order, n, groups,
                       per);
    HIP_TRY(hipGetLastError());
    *d_order = ob.order;
    return RT_OK;
}

// Flag bits outside RT_FLAG_ALL (e.g. ABI 5's RT_FLAG_POOL) are an error, not ignored.
int check_flags(const rt_params *p, const char *who) {
    if (p->flags & ~RT_FLAG_ALL)
        return rt_fail(RT_ERR_ARG, std::string(who) + ": unknown flag bits " + std::to_string(p->flags & ~RT_FLAG_ALL));
    return RT_OK;
}

// The shard (p->rank of p->world, in blocks of p->row_block rows) of the scene's frame, with
// the defaults filled in (world 1, row_block 8).
int norm_world(const rt_params *p) { return p->world > 0 ? p->world : 1; }
int norm_row_block(const rt_params *p) { return p->row_block > 0 ? p->row_block : 8; }
struct Shard {
    int world = 1, row_block = 8, rows = 0;
    long long n_pixels = 0;
    ShardGeom g{};
};
int shard_of(const rt_scene *s, const rt_params *p, const char *who, Shard &sh) {
    if ((int64_t)s->width * s->height > INT32_MAX)
        return rt_fail(RT_ERR_LIMIT, std::string(who) + ": frames above 2^31 pixels are not supported");
    sh.world = norm_world(p);
    sh.row_block = norm_row_block(p);
    const int64_t rows = rt_shard_rows_impl(s->height, p->rank, sh.world, sh.row_block, nullptr);
    if (rows < 0) return RT_ERR_ARG;
    sh.rows = (int)rows;
    sh.n_pixels = (long long)rows * s->width;
    sh.g = rtd::shard_geom(s->width, p->rank, sh.world, sh.row_block, sh.n_pixels);
    return RT_OK;
}

// An accumulator's pass (rt_accum_add): the chain buffer and the samples the pass adds.  The
// render's spp is then the absolute sample the pass ends at; the pixel order and the stats go
// by the pass's own sample count (rt_launch_plan.h PlanIn.pass_spp).
// A subset pass (rt_accum_add_selected) also names its item list: `n_items` shard pixels in
// `items` (device memory, made by rt_select_kernel), each raised to the render's spp from its
// own record; `n` is then only the plan's pass marker and `samples` the pass's sample total.
struct ChainPass {
    uint4 *chain;
    int n;
    const int *items = nullptr;
    long long n_items = 0;
    unsigned long long samples = 0;
    // A fast accumulator's pass (rt_accum_create_fast): its chunk size and the work units every
    // item of this launch gets (rt_launch_plan.h PlanIn.fast_units); 0, 0 for a parity pass.
    int fast_c = 0, fast_units = 0;
    // A moments accumulator's pass: its moment records and reported moments (else null).
    uint4 *mom = nullptr;
    float *moments = nullptr;
};

// One word of the queue block, written in stream order.
int set_queue_word(rt_device_scene *d, int word, const void *address, hipStream_t stream) {
    hipLaunchKernelGGL(rt_set_u64_kernel, dim3(1), dim3(1), 0, stream, d->queue + word,
                       (unsigned long long)(uintptr_t)address);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// Hand-off, after the plain kernel's launch: the parked pixels, on the runahead kernel `rk`
// over its whole resident grid.  With the pixel order's estimates at hand (gr.spread2) the
// park-list slots go heaviest first (work left), spread one per wave of that grid
// (RT_HANDOFF_SPREAD); else in slot order.  `w`: the main launch's workspace view.
int launch_handoff(rt_device_scene *d, const ShardGeom &g, const rtp::Grid &gr, MegaKernel rk, rtd::WfState w, int spp,
                   float *k_out, hipStream_t stream) {
    const long long slots = gr.slots;
    const int *map = nullptr;
    if (gr.spread2) {
        const OrderBuf ob(d->order_buf, g.n_pixels);   // (slots <= n_pixels: the arrays hold them)
        size_t tmp_bytes = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp_bytes, (unsigned *)nullptr, (unsigned *)nullptr,
                                                             (int *)nullptr, (int *)nullptr, (int)slots, 0, 32, stream));
        const unsigned nbs = (unsigned)((slots + 255) / 256);
        hipLaunchKernelGGL(rt_park_keys_kernel, dim3(nbs), dim3(256), 0, stream, (const uint4 *)d->wf_queue[0], slots, spp,
                           (const unsigned *)ob.cost, ob.park_keys, ob.ids);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceRadixSort::SortPairsDescending(ob.tmp, tmp_bytes, ob.park_keys, ob.park_keys_sorted, ob.ids,
                                                             ob.sorted, (int)slots, 0, 32, stream));
        // (the runahead launch's static deal: per2 slots to each of its waves, as in the kernel)
        hipLaunchKernelGGL(rt_order_spread_kernel, dim3(nbs), dim3(256), 0, stream, (const int *)ob.sorted, ob.resume_map,
                           slots, gr.waves2, gr.per2);
        HIP_TRY(hipGetLastError());
        map = ob.resume_map;
    }
    if (int rc = set_queue_word(d, rtd::kQueueResumeMap, map, stream)) return rc;
    w.lanes = gr.blocks2 * 256;
    w.n = slots;   // the park list's slots
    hipLaunchKernelGGL(rk, dim3((unsigned)gr.blocks2), dim3(256), 0, stream, d->ds, g, w, spp, k_out, d->counters, d->queue,
                       (const int *)nullptr, (unsigned *)nullptr, 0, gr.mode2);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The events a render with stats records: start, pixel order built, end.
struct RenderEvents {
    EventSet set;
    hipEvent_t start = nullptr, ordered = nullptr, end = nullptr;
};

// rt_stats of one shard, once its last launch is queued (waits for it).
int read_stats(rt_device_scene *d, const rtp::Schedule &plan, bool count, RenderEvents &ev, LaunchTimer &timer,
               hipStream_t stream, rt_stats *st, const ChainPass *cp = nullptr) {
    HIP_TRY(hipEventRecord(ev.end, stream));
    HIP_TRY(hipEventSynchronize(ev.end));
    float ms = 0.f, ms_order = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.start, ev.end));
    if (plan.ordered) HIP_TRY(hipEventElapsedTime(&ms_order, ev.start, ev.ordered));
    std::memset(st, 0, sizeof *st);
    st->pixels = (uint64_t)plan.n_pixels;
    st->samples = (uint64_t)plan.n_pixels * (uint64_t)plan.stats_spp;
    if (cp && cp->items) {   // a subset pass: the list's pixels and what they were raised by
        st->pixels = (uint64_t)cp->n_items;
        st->samples = cp->samples;
    }
    st->render_ms = ms;
    st->order_ms = ms_order;
    st->devices = 1;
    st->schedule = plan.sched;
    double kms[2];
    uint64_t kn[2];
    HIP_TRY(timer.collect(kms, kn));
    st->extend_ms = kms[0];
    st->shade_ms = kms[1];
    st->extend_launches = kn[0];
    st->shade_launches = kn[1];
    unsigned long long c[rtd::kOrderCounters];   // the render's counters (rt_wavefront.h counters_flush; [7]: wf_extend_kernel)
    HIP_TRY(hipMemcpy(c, d->counters, sizeof c, hipMemcpyDeviceToHost));
    st->extend_rays = c[7];
    if (count) {
        st->rays = c[0]; st->aabb_tests = c[1]; st->tri_tests = c[2];
        st->light_queries = c[3]; st->light_aabb_tests = c[4]; st->light_tri_tests = c[5];
        st->shading_hits = c[6];
    }
    return RT_OK;
}

// One shard on one device: rt_render_device, and with `cp` a pass of rt_accum_add (the caller
// has checked that the parameters select a parity render on the lane-resident kernel).  A
// one-shot render launches exactly what it launched before the accumulator existed.
int launch(rt_scene *s, const rt_params *p, float *d_out, hipStream_t stream, rt_stats *st,
           const ChainPass *cp = nullptr) {
    // validate and plan (rt_launch_plan.h)
    if (!s || !p || !d_out) return rt_fail(RT_ERR_ARG, "rt_render: NULL argument");
    if (int rc = check_flags(p, "rt_render")) return rc;
    if (p->device < 0 || p->device >= kRtMaxDevices || !s->dev[p->device])
        return rt_fail(RT_ERR_ARG, "rt_render: scene not uploaded to device " + std::to_string(p->device));
    rtp::PlanIn in;
    in.flags = p->flags;
    in.kernel = p->kernel;
    in.count = p->count;
    in.fast_chunk = p->fast_chunk;
    in.spp = p->spp > 0 ? p->spp : s->samples;
    in.pass_spp = cp ? cp->n : 0;
    in.subset_items = cp && cp->items ? cp->n_items : 0;
    if (cp && cp->fast_c > 0) {   // (the accumulator's chunk size, not the call's)
        in.fast_accum = true;
        in.fast_chunk = cp->fast_c;
        in.fast_units = cp->fast_units;
        in.moments = cp->mom != nullptr;
    }
    in.ray_depth = s->ray_depth;
    if (const rtp::Refusal r = rtp::plan_check(in)) return rt_fail(r.code, r.msg);
    Shard sh;
    if (int rc = shard_of(s, p, "rt_render", sh)) return rc;
    const ShardGeom &g = sh.g;
    rt_device_scene *d = s->dev[p->device];
    DeviceGuard guard(d->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    in.n_pixels = g.n_pixels;
    in.n_nodes = d->ds.n_nodes;
    rtp::Variant runahead;
    runahead.spec = true;
    runahead.chain = cp != nullptr;
    const MegaKernel rk = mega_kernel_of(runahead);   // (the hand-off's relaunch; its grid bounds the runahead shards)
    if (in.kernel == RT_KERNEL_LANE && g.n_pixels > 0) in.spec_blocks = resident_blocks(d, rk);
    const rtp::Schedule plan = rtp::plan_schedule(in);
    if (plan.refused) return rt_fail(plan.refused.code, plan.refused.msg);
    const MegaKernel mk = mega_kernel_of(plan.v);
    if (!mk) return rt_fail(RT_ERR_ARG, "rt_render: no kernel instantiation for these parameters");
    rtp::Grid grid;
    if (plan.lane) grid = rtp::plan_grid(plan, resident_blocks(d, mk));
    if (grid.refused) return rt_fail(grid.refused.code, grid.refused.msg);

    // counters and events
    const bool count = p->count != 0;
    if (count || st) HIP_TRY(hipMemsetAsync(d->counters, 0, rtd::kOrderCounters * sizeof(unsigned long long), stream));
    LaunchTimer timer;
    timer.on = st != nullptr && (p->flags & RT_FLAG_KERNEL_TIMES) != 0;
    HIP_TRY(hipMemsetAsync(d->queue + rtd::kQueueRender, 0, sizeof(unsigned long long), stream));
    RenderEvents ev;
    if (st) {
        HIP_TRY(ev.set.make(ev.start));
        HIP_TRY(ev.set.make(ev.ordered));
        HIP_TRY(ev.set.make(ev.end));
        HIP_TRY(hipEventRecord(ev.start, stream));
    }

    if (plan.sched == RT_SCHED_WAVEFRONT) {
        if (int rc = launch_wavefront(d, g, in.spp, s->ray_depth, d_out, stream, count, timer)) return rc;
    } else if (plan.lane) {   // lane-resident (rt_mega.h), the default
        if (int rc = ensure_wf(d, std::max<long long>(g.n_pixels, grid.slots), s->ray_depth)) return rc;   // vertex records
        rtd::WfState w = d->wf;
        w.n = cp && cp->items ? cp->n_items : g.n_pixels;   // (the CHAIN kernels' item count)
        w.lanes = grid.slots;   // LaneRec slots (<= the workspace capacity)
        w.round_min = plan.round_min;
        if (plan.handoff) {   // the park list: every slot "nothing parked"; the runahead launch's claim counter
            HIP_TRY(hipMemsetAsync(d->wf_queue[0], 0xff, (size_t)grid.slots * 32, stream));
            HIP_TRY(hipMemsetAsync(d->queue + rtd::kQueueResume, 0, sizeof(unsigned long long), stream));
        }
        const int *order = cp ? cp->items : nullptr;   // (a subset pass: the list is the order)
        if (plan.ordered)
            if (int rc = launch_order(d, g, stream, grid.groups, grid.per, &order)) return rc;
        if (st) HIP_TRY(hipEventRecord(ev.ordered, stream));
        float *k_out = d_out;
        if (plan.v.fast) {   // chunk-major partial sums, folded below
            // (a moments pass: the units' partials of squares follow the sums', six floats per unit)
            HIP_TRY(grow((void **)&d->fast_part, &d->fast_part_bytes,
                         (size_t)plan.n_items * (plan.v.mom ? 6 : 3) * sizeof(float)));
            k_out = d->fast_part;
        }
#ifdef RT_MEGA_PROF
        if (int rc = mega_prof_reset(stream)) return rc;
#endif
        // the chain buffer's address, where the chain kernels read it
        if (cp)
            if (int rc = set_queue_word(d, rtd::kChainWord, cp->chain, stream)) return rc;
        if (plan.v.mom) {
            if (int rc = set_queue_word(d, rtd::kMomentWord, cp->mom, stream)) return rc;
            if (int rc = set_queue_word(d, rtd::kMomentPartWord, k_out + 3 * plan.n_items, stream)) return rc;
        }
        hipLaunchKernelGGL(mk, dim3((unsigned)grid.blocks), dim3(256), 0, stream, d->ds, g, w, in.spp, k_out, d->counters,
                           d->queue, order, (unsigned *)nullptr, plan.cs, plan.mode);
        HIP_TRY(hipGetLastError());
        if (plan.handoff)
            if (int rc = launch_handoff(d, g, grid, rk, w, in.spp, k_out, stream)) return rc;
        if (plan.v.mom) {   // both partial sets into both records, the reported sums and moments
            hipLaunchKernelGGL(rt_fast_fold_moments_kernel, dim3((unsigned)((w.n + 255) / 256)), dim3(256), 0, stream, cp->chain,
                               cp->mom, order, w.n, plan.chunks, plan.cs, in.spp, (const float *)d->fast_part, d_out, cp->moments);
            HIP_TRY(hipGetLastError());
        } else if (plan.v.fast && plan.v.chain) {   // the items' partials into their records and reported sums (d_out: the accumulator's sums)
            hipLaunchKernelGGL(rt_fast_fold_chain_kernel, dim3((unsigned)((w.n + 255) / 256)), dim3(256), 0, stream, cp->chain,
                               order, w.n, plan.chunks, plan.cs, in.spp, (const float *)d->fast_part, d_out);
            HIP_TRY(hipGetLastError());
        } else if (plan.v.fast) {
            const long long n3 = g.n_pixels * 3;
            hipLaunchKernelGGL(rt_fast_reduce_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, stream,
                               (const float *)d->fast_part, d_out, n3, plan.chunks);
            HIP_TRY(hipGetLastError());
        }
#ifdef RT_MEGA_PROF
        if (int rc = mega_prof_report(stream, count, g.n_pixels, order, !grid.spread2)) return rc;
#endif
    }
    HIP_TRY(hipGetLastError());
    if (st) return read_stats(d, plan, count, ev, timer, stream, st, cp);
    return RT_OK;
}

// One shard rendered into host memory on the scene's copy on p->device.
int render_host(rt_scene *s, const rt_params *p, float *out, rt_stats *st) {
    int rc = ensure_device_scene(s, p->device);
    if (rc) return rc;
    Shard sh;
    if ((rc = shard_of(s, p, "rt_render", sh))) return rc;
    const size_t bytes = (size_t)sh.n_pixels * 3 * sizeof(float);
    DeviceGuard guard(p->device);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    float *d_out = nullptr;
    HIP_TRY(hipMalloc(&d_out, bytes ? bytes : 4));
    rt_stats local;
    rc = launch(s, p, d_out, nullptr, st ? st : &local);
    if (rc == RT_OK) {
        hipError_t e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = rt_fail(RT_ERR_DEVICE, std::string("rt_render copy: ") + hipGetErrorString(e));
    }
    (void)hipFree(d_out);
    return rc;
}

}  // namespace

void rt_device_scene_release(rt_scene *s) {
    if (!s) return;
    for (rt_device_scene *&d : s->dev) {
        free_device_scene(d);
        d = nullptr;
    }
    delete s->blob;
    s->blob = nullptr;
}

// rt_scene_set_camera's device half: the camera words of every copy's by-value DevScene (what
// ensure_device_scene fills from the same fields); the next launch carries them.
void rt_device_scene_set_camera(rt_scene *s) {
    for (rt_device_scene *d : s->dev) {
        if (!d) continue;
        std::memcpy(d->ds.cam_pos, s->cam_pos, sizeof d->ds.cam_pos);
        std::memcpy(d->ds.cam_axes, s->cam_axes, sizeof d->ds.cam_axes);
        std::memcpy(d->ds.tan_fov, s->tan_half_fov, sizeof d->ds.tan_fov);
    }
}

// Frame assembly on the root device of rt_render_frame (below).
__global__ void __launch_bounds__(256) rt_rows_scatter_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                              const int *__restrict__ frame_row_of, long long rows,
                                                              long long row_bytes) {
    // rows of whole 4-byte words (row_bytes % 4 == 0: W*3 floats, or W*3 bytes with W % 4 == 0)
    // go word by word; other widths byte by byte
    const long long r = blockIdx.y;
    if (r >= rows) return;
    const uint8_t *s = src + r * row_bytes;
    uint8_t *d = dst + (long long)frame_row_of[r] * row_bytes;
    if ((row_bytes & 3) == 0) {
        for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < row_bytes / 4; k += (long long)gridDim.x * blockDim.x)
            ((uint32_t *)d)[k] = ((const uint32_t *)s)[k];
    } else {
        for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < row_bytes; k += (long long)gridDim.x * blockDim.x)
            d[k] = s[k];
    }
}

extern "C" {

int rt_scene_upload(rt_scene *s, int32_t device) {
    if (!s) return rt_fail(RT_ERR_ARG, "rt_scene_upload: NULL scene");
    return ensure_device_scene(s, device);
}

int rt_render_device(rt_scene *s, const rt_params *p, float *d_out, void *stream, rt_stats *st) {
    return launch(s, p, d_out, (hipStream_t)stream, st);
}

// The quantizer thresholds go to each device's constant memory once; threads finishing on the
// same device at first use serialise on the mutex.
static int quant_thresholds_upload() {
    static std::mutex upload_mu;
    static bool uploaded[kRtMaxDevices] = {false};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= kRtMaxDevices) return rt_fail(RT_ERR_DEVICE, "rt_tonemap_u8_device: device id");
    std::lock_guard<std::mutex> lock(upload_mu);
    if (!uploaded[dev]) {
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(k_quant_thr), rtm::kQuantThr, sizeof rtm::kQuantThr));
        uploaded[dev] = true;
    }
    return RT_OK;
}

// The launch behind both tonemap entries: per-pixel counts where d_counts is given, else `normalizer`.
static int finish_launch(const float *d_sum, const int32_t *d_counts, float normalizer, int32_t width, int32_t height,
                         uint8_t *d_rgb, void *stream) {
    if (int rc = quant_thresholds_upload()) return rc;
    const long long n = (long long)width * height * 3;
    const dim3 blocks((unsigned)std::min<long long>((n + 255) / 256, 4096));
    if (d_counts)
        hipLaunchKernelGGL(rt_finish_counts_kernel, blocks, dim3(256), 0, (hipStream_t)stream, d_sum, d_counts, n, d_rgb);
    else
        hipLaunchKernelGGL(rt_finish_kernel, blocks, dim3(256), 0, (hipStream_t)stream, d_sum, n, normalizer, d_rgb);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_tonemap_u8_counts_device(const float *d_sum, const int32_t *d_counts, int32_t width, int32_t height, uint8_t *d_rgb,
                                void *stream) {
    if (!d_sum || !d_counts || !d_rgb || width <= 0 || height <= 0)
        return rt_fail(RT_ERR_ARG, "rt_tonemap_u8_counts_device: bad argument");
    return finish_launch(d_sum, d_counts, 0.f, width, height, d_rgb, stream);
}

int rt_tonemap_u8_device(const float *d_sum, int32_t width, int32_t height, int32_t spp, uint8_t *d_rgb, void *stream) {
    if (!d_sum || !d_rgb || width <= 0 || height <= 0 || spp <= 0)
        return rt_fail(RT_ERR_ARG, "rt_tonemap_u8_device: bad argument");
    return finish_launch(d_sum, nullptr, 1.f / (float)spp, width, height, d_rgb, stream);
}

int rt_render(rt_scene *s, const rt_params *p, float *out, rt_stats *st) {
    if (!s || !p || !out) return rt_fail(RT_ERR_ARG, "rt_render: NULL argument");
    if (int rc = check_flags(p, "rt_render")) return rc;
    return render_host(s, p, out, st);
}

}  // extern "C"

// ------------------------------------------------------------------------ feature buffer, denoiser, accumulator
#include "rt_denoise_device.h"   // the feature buffer and the denoiser: kernels, launch functions, entries
#include "rt_accum_device.h"     // rt_accum_*: the accumulator's kernels, helpers and entries
#include "rt_motion_device.h"    // rt_motion_device: the motion records' kernel
#include "rt_temporal_device.h"  // rt_temporal_device, rt_history_*: the temporal step's kernel and the history object
#include "rt_refit_device.h"     // rt_scene_update_tris*, rt_scene_read_device: the scatter and refit kernels and their entries
#include "rt_pose_device.h"      // rt_scene_pose_meshes' device half: the rest records, the pose kernel

// The whole frame as shards 0 .. n-1 of a (world n, row_block) split, shard r on device
// devices[r] (include/rt_hw.h rt_render_frame).  rt_frame_plan.h defines the layout: which
// device is the root (devices[0]), which shards share a device, where shard r's rows land in
// the root's staging buffer and how large every buffer is.  rt_render_frame (below) checks its
// arguments, plans, and then: frame_prepare_devices (scene copies, streams, events; kept in the
// device copies between frames), frame_setup_root (root buffer, row map, peer access), one
// FrameRun::work per distinct device (render, finish to 8 bits, copy to the root), on failure
// a drain of the copy streams, frame_assemble (rows into frame order on the root, one copy to
// the host per output) and rtp::merge_frame_stats.
// (On the one-GPU pool this runs with every shard on device 0; the peer copies between two
// MI355X have not run on hardware.  tests/test_frame_plan.py covers their host arithmetic.)
namespace {

static_assert(rtp::kMaxDevices == kRtMaxDevices, "the frame plan refuses the device ids a scene has no slot for");

int frame_prepare_devices(rt_scene *s, const rtp::FramePlan &f) {
    for (int d : f.uniq) {   // (kept between frames)
        if (int rc = ensure_device_scene(s, d)) return rc;
        DeviceGuard g(d);
        HIP_TRY(ensure_frame_streams(s->dev[d]));
    }
    return RT_OK;
}

// Grows the root buffer, uploads the row map and lets the root and its peers copy directly
// (xGMI) where the runtime allows.
int frame_setup_root(rt_scene *s, const rtp::FramePlan &f) {
    const int root = f.root();
    rt_device_scene::Frame &rf = s->dev[root]->fr;
    {
        DeviceGuard g(root);
        HIP_TRY(grow(&rf.root_buf, &rf.root_bytes, f.root_bytes));
        HIP_TRY(hipStreamSynchronize(rf.stream));   // (the previous frame's map upload is done)
        HIP_TRY(hipMemcpyAsync((uint8_t *)rf.root_buf + f.o_row_map, f.frame_row_of.data(),
                               (size_t)f.height * sizeof(int32_t), hipMemcpyHostToDevice, rf.stream));
    }
    for (int d : f.uniq) {
        if (d == root) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, d, root) == hipSuccess && can) {
            DeviceGuard g(d);
            (void)hipDeviceEnablePeerAccess(root, 0);
            (void)hipGetLastError();   // (already enabled is not an error here)
        }
        if (hipDeviceCanAccessPeer(&can, root, d) == hipSuccess && can) {
            DeviceGuard g(root);
            (void)hipDeviceEnablePeerAccess(d, 0);
            (void)hipGetLastError();
        }
    }
    return RT_OK;
}

// What the frame's workers share; work(ui) is the host thread of device f.uniq[ui].  It renders
// that device's shards one after another (one render per (scene, device) in flight), alternating
// between two buffers: shard r is rendered (launch waits for it: stats) and finished to 8 bits
// (rt_finish_kernel, scene.cpp:54-64) on the render stream; the copy stream waits for that
// finish and copies the shard, 8-bit rows and (if asked) float sums, to the root's staging
// buffer (hipMemcpyPeerAsync: over xGMI between MI355X), while the render stream goes on with
// the next shard in the other buffer (it waits for that buffer's previous copy first).  The
// device's last copy is marked by fr.last, which frame_assemble waits for.
struct FrameRun {
    rt_scene *s;
    const rt_params *p;
    const rtp::FramePlan &f;
    uint8_t *root_buf;               // the root's (staging parts at f.o_stage_u8, f.o_stage_f)
    std::vector<rt_stats> stats;     // [shard]
    std::vector<int> rcs;            // [uniq index] the worker's failure, with its text
    std::vector<std::string> errs;

    void fail(size_t ui, int rc) { rcs[ui] = rc, errs[ui] = rt_last_error(); }

    void work(size_t ui) {
        const int dev = f.uniq[ui], root = f.root();
        const rtp::FrameDevice &fd = f.dev[ui];
        rt_device_scene::Frame &fr = s->dev[dev]->fr;
        DeviceGuard g(dev);
        if (!g.ok) return fail(ui, rt_fail(RT_ERR_DEVICE, "hipSetDevice failed"));
        hipError_t e = hipSuccess;
        for (int b = 0; b < 2 && e == hipSuccess; ++b) e = grow(&fr.buf[b], &fr.bytes[b], fd.buf_bytes);
        int nb = 0;   // shards done on this device (buffer = nb % 2)
        for (int r = 0; r < f.n && e == hipSuccess && rcs[ui] == RT_OK; ++r) {
            if (f.dev_of[r] != dev || f.rows[r] == 0) continue;
            const int b = nb % 2;
            float *sum = (float *)fr.buf[b];
            uint8_t *rgb = (uint8_t *)fr.buf[b] + fd.sum_bytes;
            if (nb >= 2) e = hipStreamWaitEvent(fr.stream, fr.copied[b], 0);   // buffer b's last copy done
            if (e != hipSuccess) break;
            rt_params q = *p;
            q.rank = r;
            q.world = f.n;
            q.row_block = f.row_block;
            q.device = dev;
            q.spp = f.spp;
            int lr = launch(s, &q, sum, fr.stream, &stats[r]);   // waits (stats)
            if (!lr) lr = rt_tonemap_u8_device(sum, f.width, (int32_t)f.rows[r], f.spp, rgb, fr.stream);
            if (lr) { fail(ui, lr); break; }   // (fr.last is still recorded below)
            e = hipEventRecord(fr.finished, fr.stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(fr.cp_stream, fr.finished, 0);
            if (e == hipSuccess)
                e = hipMemcpyPeerAsync(root_buf + f.o_stage_u8 + f.base[r] * f.row_u8, root, rgb, dev, f.rows[r] * f.row_u8,
                                       fr.cp_stream);
            if (e == hipSuccess && f.want_sums)
                e = hipMemcpyPeerAsync(root_buf + f.o_stage_f + f.base[r] * f.row_f, root, sum, dev, f.rows[r] * f.row_f,
                                       fr.cp_stream);
            if (e == hipSuccess) e = hipEventRecord(fr.copied[b], fr.cp_stream);
            ++nb;
        }
        if (e == hipSuccess) e = hipEventRecord(fr.last, fr.cp_stream);
        if (e != hipSuccess && rcs[ui] == RT_OK)
            fail(ui, rt_fail(RT_ERR_DEVICE, std::string("rt_render_frame: ") + hipGetErrorString(e)));
    }
};

// Assembles the frame on the root behind every device's last copy; one copy to the host per output.
int frame_assemble(rt_scene *s, const rtp::FramePlan &f, uint8_t *out_rgb, float *out_sum) {
    const int root = f.root();
    DeviceGuard g(root);
    if (!g.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const rt_device_scene::Frame &rf = s->dev[root]->fr;
    hipStream_t q = rf.stream;
    uint8_t *buf = (uint8_t *)rf.root_buf, *frame_u8 = buf + f.o_frame_u8, *frame_f = buf + f.o_frame_f;
    const int *row_map = (const int *)(buf + f.o_row_map);
    const long long H = f.height;
    // The root's own last copy is waited for on its stream.  A peer's copy is waited for on
    // the host (hipEventSynchronize on the peer's event) before the assembly is queued: a
    // root-stream wait on an event recorded on another device is the cheaper form, but it
    // has not run on a multi-GPU box yet, so the host wait stays the
    // conservative default until it has.
    for (int d : f.uniq) {
        if (d == root) {
            HIP_TRY(hipStreamWaitEvent(q, s->dev[d]->fr.last, 0));
        } else {
            DeviceGuard gp(d);
            if (!gp.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
            HIP_TRY(hipEventSynchronize(s->dev[d]->fr.last));
        }
    }
    hipLaunchKernelGGL(rt_rows_scatter_kernel, dim3(4, (unsigned)H), dim3(256), 0, q, (const uint8_t *)(buf + f.o_stage_u8),
                       frame_u8, row_map, H, (long long)f.row_u8);
    HIP_TRY(hipGetLastError());
    if (out_sum) {
        hipLaunchKernelGGL(rt_rows_scatter_kernel, dim3(8, (unsigned)H), dim3(256), 0, q,
                           (const uint8_t *)(buf + f.o_stage_f), frame_f, row_map, H, (long long)f.row_f);
        HIP_TRY(hipGetLastError());
    }
    if (out_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, frame_u8, (size_t)H * f.row_u8, hipMemcpyDeviceToHost, q));
    if (out_sum) HIP_TRY(hipMemcpyAsync(out_sum, frame_f, (size_t)H * f.row_f, hipMemcpyDeviceToHost, q));
    HIP_TRY(hipStreamSynchronize(q));
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_render_frame(rt_scene *s, const rt_params *p, int32_t n_shards, const int32_t *devices, uint8_t *out_rgb,
                    float *out_sum, rt_stats *st) {
    // 1. the arguments (the devices check needs no device count and comes before it)
    if (!s || !p || (!out_rgb && !out_sum)) return rt_fail(RT_ERR_ARG, "rt_render_frame: NULL argument");
    if (int rc = check_flags(p, "rt_render_frame")) return rc;
    if (const rtp::Refusal r = rtp::frame_check_devices(n_shards, devices)) return rt_fail(r.code, r.msg);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    const rtp::FrameIn in{s->width, s->height, n_shards, devices, norm_row_block(p), p->spp > 0 ? p->spp : s->samples,
                          ndev, out_sum != nullptr};
    if (const rtp::Refusal r = rtp::frame_check(in)) return rt_fail(r.code, r.msg);
    if (int rc = ensure_blob(s)) return rc;   // built once here, copied to every device
    // 2. the plan
    const rtp::FramePlan f = rtp::plan_frame(in);
    if (f.refused) return rt_fail(f.refused.code, f.refused.msg);
    // 3. and 4. the devices and the root
    if (int rc = frame_prepare_devices(s, f)) return rc;
    if (int rc = frame_setup_root(s, f)) return rc;
    // 5. one worker per device (the root's on this thread)
    const size_t nu = f.uniq.size();
    FrameRun run{s, p, f, (uint8_t *)s->dev[f.root()]->fr.root_buf, std::vector<rt_stats>(f.n),
                 std::vector<int>(nu, RT_OK), std::vector<std::string>(nu)};
    std::vector<std::thread> threads;
    for (size_t ui = 1; ui < nu; ++ui) threads.emplace_back(&FrameRun::work, &run, ui);
    run.work(0);
    for (std::thread &t : threads) t.join();
    // every shard's render has ended here (launch waited for each); from now on the host waits
    // only for the copies still in flight, the assembly and the copy to the host: gather_ms
    const auto t0 = std::chrono::steady_clock::now();
    // 6. a failed worker: leave no copy in flight into the root's buffers
    for (size_t ui = 0; ui < nu; ++ui)
        if (run.rcs[ui] != RT_OK) {
            for (int d : f.uniq) {
                DeviceGuard g(d);
                (void)hipStreamSynchronize(s->dev[d]->fr.cp_stream);
            }
            return rt_fail(run.rcs[ui], "device " + std::to_string(f.uniq[ui]) + ": " + run.errs[ui]);
        }
    // 7. and 8. the frame and its stats
    if (int rc = frame_assemble(s, f, out_rgb, out_sum)) return rc;
    const double gather_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (st) rtp::merge_frame_stats(f, run.stats.data(), gather_ms, st);
    return RT_OK;
}

// The float frame over devices 0 .. n-1 (ABI 3 entry; rt_render_frame with shard r on device r).
int rt_render_multi(rt_scene *s, const rt_params *p, int32_t n_devices, float *out, rt_stats *st) {
    if (!s || !p || !out) return rt_fail(RT_ERR_ARG, "rt_render_multi: NULL argument");
    if (int rc = check_flags(p, "rt_render_multi")) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    const int n = n_devices > 0 ? n_devices : ndev;
    if (n < 1 || n > ndev || n > kRtMaxDevices)
        return rt_fail(RT_ERR_DEVICE, "rt_render_multi: " + std::to_string(n) + " devices requested, " +
                                          std::to_string(ndev) + " visible");
    return rt_render_frame(s, p, n, nullptr, nullptr, out, st);
}

int32_t rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rt_device_synchronize(void) {
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

}  // extern "C"

#include "rt_check_device.h"   // rt_device_selfcheck, rt_intersect_rays[_via], rt_debug_*: kernels, host halves, entries
