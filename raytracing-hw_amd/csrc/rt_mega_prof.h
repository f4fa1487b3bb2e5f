// rt_mega_prof.h — the diagnostics build of the lane-resident kernel (make prof, RT_MEGA_PROF).
// Included by rt_mega_device.h only, under the macro, ahead of rt_mega_kernel: the device globals
// the kernel's #ifdef RT_MEGA_PROF lines add to, TbAcc, and the host side's two calls,
// mega_prof_reset before a lane-resident launch and mega_prof_report after it.
#pragma once

// Per-wave clock64() split of the main loop.
// [0] shade-iteration cycles [1] traversal-iteration cycles [2] pixel-assign cycles
// [3] shade iterations [4] traversal iterations [5] sum of ready lanes over shade iterations
// [6] sum of traversing lanes over traversal iterations [7] waves
__device__ unsigned long long g_mega_prof[8];
__device__ unsigned long long g_mega_seg[8];   // shading segments (rt_path.h RT_PROF_SEG)
// per-wave start and end (wall_clock64, 100 MHz): the distribution of wave finish times
constexpr int kProfWaves = 16384;
__device__ unsigned long long g_wave_t[2 * kProfWaves];
__device__ unsigned int g_wave_n;
// time buckets of 5 ms (wall clock since the wave's start; the waves of a launch start within
// microseconds of each other): [0] traversal iterations [1] traversing lanes summed over them
// [2] lanes holding work (state != idle) summed over them [3] shading passes [4] READY lanes
// summed over them [5] management passes (runahead kernel)
constexpr int kTb = 256, kTbN = 6;
constexpr unsigned long long kTbTicks = 500000;   // 5 ms at 100 MHz
__device__ unsigned long long g_tb[kTb * kTbN];
struct TbAcc {
    int b = 0;
    unsigned long long c[kTbN] = {0, 0, 0, 0, 0, 0};
    __device__ void at(unsigned long long t0) {   // (every lane; lane 0 flushes)
        const unsigned long long e = (wall_clock64() - t0) / kTbTicks;
        const int nb = e < (unsigned long long)kTb ? (int)e : kTb - 1;
        if (nb != b) flush(nb);
    }
    __device__ void flush(int nb) {
        if ((threadIdx.x & 63) == 0)
            for (int k = 0; k < kTbN; ++k)
                if (c[k]) atomicAdd(&g_tb[b * kTbN + k], c[k]);
        for (int k = 0; k < kTbN; ++k) c[k] = 0;
        b = nb;
    }
};

namespace {

// Zeroes the profile's device globals, in stream order.
int mega_prof_reset(hipStream_t stream) {
    const unsigned long long z[16] = {};
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_mega_prof), z, 8 * sizeof z[0], 0, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_mega_seg), z, 8 * sizeof z[0], 0, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(rtd::g_spec_prof), z, sizeof z, 0, hipMemcpyHostToDevice, stream));
    static const unsigned long long zp[rtd::kPopProfN] = {};
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(rtd::g_pop_prof), zp, sizeof zp, 0, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_wave_n), z, sizeof(unsigned), 0, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(rtd::g_chain_n), z, sizeof(unsigned), 0, hipMemcpyHostToDevice, stream));
    static const std::vector<unsigned long long> ztb(kTb * kTbN, 0ull);
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_tb), ztb.data(), ztb.size() * 8, 0, hipMemcpyHostToDevice, stream));
    return RT_OK;
}

// The runahead kernel's chain completions: when they end, and where the last of them stood in
// the claim order (0 = the first pixel claimed).  `order`: the render's pixel order (null:
// row-major); `order_valid`: false once the hand-off's second sort has reused its array
// (rt_device.hip OrderBuf), when the positions are not reported.
int mega_prof_chains(hipStream_t stream, unsigned long long t0, long long np, const int *order, bool order_valid) {
    unsigned nc = 0;
    HIP_TRY(hipMemcpyFromSymbolAsync(&nc, HIP_SYMBOL(rtd::g_chain_n), sizeof nc, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    nc = std::min<unsigned>(nc, (unsigned)rtd::kChainRec);
    if (!nc) return RT_OK;
    std::vector<unsigned long long> ct(nc);
    std::vector<unsigned> cpx(nc);
    HIP_TRY(hipMemcpyFromSymbolAsync(ct.data(), HIP_SYMBOL(rtd::g_chain_t), nc * 8ull, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyFromSymbolAsync(cpx.data(), HIP_SYMBOL(rtd::g_chain_pix), nc * 4ull, 0, hipMemcpyDeviceToHost, stream));
    std::vector<int> rank;
    if (order_valid) {
        rank.resize((size_t)np);
        if (order) {
            std::vector<int> ord((size_t)np);
            HIP_TRY(hipMemcpyAsync(ord.data(), order, (size_t)np * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            for (long long q = 0; q < np; ++q) rank[ord[q]] = (int)q;
        } else {
            for (long long q = 0; q < np; ++q) rank[q] = (int)q;
        }
    }
    HIP_TRY(hipStreamSynchronize(stream));
    std::vector<unsigned> ix(nc);
    for (unsigned q = 0; q < nc; ++q) ix[q] = q;
    std::sort(ix.begin(), ix.end(), [&](unsigned a, unsigned b) { return ct[a] < ct[b]; });
    auto ms = [&](unsigned q) { return (double)(ct[ix[q]] - t0) / 1e5; };
    std::fprintf(stderr, "[mega chains] runahead-kernel chain completions=%u, end ms: p10=%.1f p50=%.1f "
                 "p90=%.1f p99=%.1f max=%.1f\n", nc, ms(nc / 10), ms(nc / 2), ms(9 * nc / 10),
                 ms((unsigned)(99ull * nc / 100)), ms(nc - 1));
    if (!order_valid) {
        std::fprintf(stderr, "[mega chains] claim-order positions not reported: the hand-off's sort reused the pixel order's array\n");
        return RT_OK;
    }
    const double fr[4] = {0.5, 0.1, 0.01, 0.001};
    for (double f : fr) {
        const unsigned k = std::max(1u, (unsigned)(f * nc));
        std::vector<double> rr(k);
        for (unsigned q = 0; q < k; ++q) {
            const unsigned px = cpx[ix[nc - 1 - q]];
            rr[q] = px < (unsigned)np ? (double)rank[px] / (double)np : -1.0;
        }
        std::sort(rr.begin(), rr.end());
        std::fprintf(stderr, "[mega chains] last %.1f%% (%u chains, from %.1f ms): claim-order position / pixels "
                     "p10=%.3f p50=%.3f p90=%.3f\n", 100.0 * f, k, ms(nc - k), rr[k / 10], rr[k / 2],
                     rr[9 * k / 10]);
    }
    return RT_OK;
}

// Reads the profile back after the render's last launch (waits for the stream) and prints it.
int mega_prof_report(hipStream_t stream, bool count, long long n_pixels, const int *order, bool order_valid) {
    unsigned long long pf[8];
    HIP_TRY(hipMemcpyFromSymbolAsync(pf, HIP_SYMBOL(g_mega_prof), sizeof pf, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const double tot = (double)(pf[0] + pf[1] + pf[2]);
    std::fprintf(stderr,
                 "[mega prof] count=%d waves=%llu cycles/wave=%.3g shade=%.3f trav=%.3f assign=%.3f "
                 "shade_iters/wave=%.0f trav_iters/wave=%.0f ready/shade=%.1f trav_lanes/iter=%.1f "
                 "cyc/shade_iter=%.0f cyc/trav_iter=%.0f\n",
                 (int)count, pf[7], tot / pf[7], pf[0] / tot, pf[1] / tot, pf[2] / tot,
                 (double)pf[3] / pf[7], (double)pf[4] / pf[7], (double)pf[5] / pf[3],
                 (double)pf[6] / pf[4], (double)pf[0] / pf[3], (double)pf[1] / pf[4]);
    unsigned long long sg[8];
    HIP_TRY(hipMemcpyFromSymbolAsync(sg, HIP_SYMBOL(g_mega_seg), sizeof sg, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::fprintf(stderr, "[mega prof] shade segments, cycles per shade iteration: mesh+emission=%.0f "
                 "normal=%.0f mr=%.0f sample=%.0f pdf=%.0f base+brdf=%.0f before=%.0f after=%.0f\n",
                 (double)sg[0] / pf[3], (double)sg[1] / pf[3], (double)sg[2] / pf[3],
                 (double)sg[3] / pf[3], (double)sg[4] / pf[3], (double)sg[5] / pf[3], (double)sg[6] / pf[3],
                 (double)sg[7] / pf[3]);
    // the pop block of the coop step (rt_wavefront.h g_pop_prof): how often it runs, for how many
    // lanes, and its share of the traversal iterations' cycles
    unsigned long long pp[rtd::kPopProfN];
    HIP_TRY(hipMemcpyFromSymbolAsync(pp, HIP_SYMBOL(rtd::g_pop_prof), sizeof pp, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (pp[0]) {
        const double st = (double)pp[0];
        std::fprintf(stderr, "[mega pop] coop steps/wave=%.0f lanes at step end: node=%.1f leaf=%.1f pop=%.1f | "
                     "steps with a pop=%.3f popping lanes/such step=%.2f cyc/pop block=%.0f "
                     "pop cycles/step=%.0f share of cyc/trav_iter=%.3f\n",
                     st / pf[7], pp[1] / st, pp[2] / st, pp[3] / st, pp[4] / st,
                     pp[4] ? (double)pp[5] / pp[4] : 0.0, pp[4] ? (double)pp[6] / pp[4] : 0.0, pp[6] / st,
                     pf[1] ? (double)pp[6] / (double)pf[1] : 0.0);
        std::fprintf(stderr, "[mega pop] steps with a pop by popping lanes (1-4, 5-8, ..., 61-64):");
        for (int b = 0; b < 16; ++b) std::fprintf(stderr, " %.4f", pp[4] ? (double)pp[8 + b] / pp[4] : 0.0);
        std::fprintf(stderr, "\n");
        // best frames (rt_wavefront.h trav_pop ELIDE): a far child that survives pushes one unless its near best
        // is 1e9 and the kernel elides those; a popped one is a merge, carried over when its lane entered the step popping
        // (counted in wave 0 of every block: per coop step of those waves)
        const double ss = pp[7] ? (double)pp[7] : 1.0;
        std::fprintf(stderr, "[mega pop] best frames, wave 0 of each block: far children entered after a near subtree/step=%.3f "
                     "with near best 1e9=%.4f | best frames popped/step=%.3f carried over=%.4f\n",
                     pp[24] / ss, pp[24] ? (double)pp[25] / pp[24] : 0.0, pp[26] / ss, pp[26] ? (double)pp[27] / pp[26] : 0.0);
    }
    // wave finish times relative to the first wave start: percentiles (ms)
    unsigned nw = 0;
    HIP_TRY(hipMemcpyFromSymbolAsync(&nw, HIP_SYMBOL(g_wave_n), sizeof nw, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    nw = std::min<unsigned>(nw, (unsigned)kProfWaves);
    std::vector<unsigned long long> wt(2 * (size_t)nw);
    if (nw) HIP_TRY(hipMemcpyFromSymbolAsync(wt.data(), HIP_SYMBOL(g_wave_t), wt.size() * 8, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (nw) {
        unsigned long long t0 = ~0ull;
        std::vector<double> ends(nw);
        for (unsigned i = 0; i < nw; ++i) t0 = std::min(t0, wt[2 * i]);
        for (unsigned i = 0; i < nw; ++i) ends[i] = (double)(wt[2 * i + 1] - t0) / 1e5;
        std::sort(ends.begin(), ends.end());
        std::fprintf(stderr, "[mega prof] wave end ms: p10=%.1f p25=%.1f p50=%.1f p75=%.1f p90=%.1f p99=%.1f max=%.1f\n",
                     ends[nw / 10], ends[nw / 4], ends[nw / 2], ends[3 * nw / 4], ends[9 * nw / 10],
                     ends[99 * (size_t)nw / 100], ends[nw - 1]);
        // per 5-ms bucket: waves alive, traversal iterations per alive wave, lanes per
        // iteration (traversing, holding work), shading passes, READY lanes per pass,
        // management passes
        std::vector<unsigned long long> tbv(kTb * kTbN);
        HIP_TRY(hipMemcpyFromSymbolAsync(tbv.data(), HIP_SYMBOL(g_tb), tbv.size() * 8, 0, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const int nbk = std::min(kTb, (int)(ends[nw - 1] / 5.0) + 1);
        for (int b = 0; b < nbk; ++b) {
            double alive = 0;   // wave-buckets alive (fraction of the bucket)
            for (unsigned i = 0; i < nw; ++i) {
                const double s0 = (double)(wt[2 * i] - t0) / 1e5, e0 = (double)(wt[2 * i + 1] - t0) / 1e5;
                const double lo = std::max(s0, 5.0 * b), hi = std::min(e0, 5.0 * (b + 1));
                if (hi > lo) alive += (hi - lo) / 5.0;
            }
            const unsigned long long *c = &tbv[(size_t)b * kTbN];
            std::fprintf(stderr, "[mega tb] t=%3d-%3d ms waves=%.0f iters/wave=%.0f trav_lanes=%.1f busy_lanes=%.1f "
                         "shades/wave=%.1f ready/shade=%.1f passes/wave=%.1f\n", 5 * b, 5 * b + 5, alive,
                         alive > 0 ? c[0] / alive : 0.0, c[0] ? (double)c[1] / c[0] : 0.0,
                         c[0] ? (double)c[2] / c[0] : 0.0, alive > 0 ? c[3] / alive : 0.0,
                         c[3] ? (double)c[4] / c[3] : 0.0, alive > 0 ? c[5] / alive : 0.0);
        }
        if (int rc = mega_prof_chains(stream, t0, n_pixels, order, order_valid)) return rc;
    }
    unsigned long long sp[16];
    HIP_TRY(hipMemcpyFromSymbolAsync(sp, HIP_SYMBOL(rtd::g_spec_prof), sizeof sp, 0, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    std::fprintf(stderr, "[mega prof] runahead: tail waves=%llu passes/tail wave=%.1f cycles/pass=%.0f "
                 "cycles in passes/wave=%.3g frontier jobs=%llu runahead jobs=%llu added=%llu "
                 "runahead jobs proven=%llu invalidations=%llu\n", sp[7], sp[7] ? (double)sp[0] / sp[7] : 0.0,
                 sp[0] ? (double)sp[1] / sp[0] : 0.0, (double)sp[1] / pf[7], sp[2], sp[3], sp[4], sp[5], sp[6]);
    std::fprintf(stderr, "[mega prof] parked pixels claimed in the tail (hand-off): %llu\n", sp[8]);
    std::fprintf(stderr, "[mega prof] runahead chains: proven share of runahead jobs=%.3f, pixels completed "
                 "in the tail=%llu, mean time per chain link (completion / spp)=%.1f us\n",
                 sp[3] ? (double)sp[5] / (double)sp[3] : 0.0, sp[15], sp[15] ? (double)sp[14] / sp[15] / 100.0 : 0.0);
    return RT_OK;
}

}  // namespace
