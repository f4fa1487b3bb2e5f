// rt_check_device.h — the test and diagnosis surface of the device half: rt_device_selfcheck (six check
// kernels and their host halves), the ray queries rt_intersect_rays[_via] (rt_rays_kernel, rt_rays_via_kernel)
// and the debug build's rt_debug_take / rt_debug_set_poison.  Included by rt_device.hip at its end, after
// rt_temporal_device.h and the whole-frame path, so the build stays one translation unit: it needs DeviceGuard,
// (and the shading-frame query rt_sample_frames_via: rt_frames_kernel)
// HIP_TRY, ensure_device_scene and g_live from there and the plain kernel's constants (kCoopLeavesPlain,
// kCoopRoundMinPlain, kPlainFarDist2, kPlainAccElide, RT_PLAIN_MAX_POPS) from rt_mega_device.h for the steps of rt_wavefront.h.

// HIP_TRY for these entries: the failure's text is the entry's prefix `who` and the error string.
#define HIP_TRY_AS(who, expr) \
    if (const hipError_t _e = (expr)) return rt_fail(RT_ERR_DEVICE, std::string(who) + hipGetErrorString(_e))
// The end of every check kernel: `local` summed over the wave, one atomic per wave that counted.
__device__ __forceinline__ void check_count(unsigned long long local, unsigned long long *bad) {
    for (int off = 32; off > 0; off >>= 1) local += __shfl_down(local, off, 64);
    if ((threadIdx.x & 63) == 0 && local) atomicAdd(bad, local);
}

extern "C" {

#if defined(RT_DEBUG_CHECKS)
// debug builds only: first recorded index violation (code << 56 | value), 0 = none
int rt_debug_take(unsigned long long *word) {
    unsigned long long z = 0;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(word, HIP_SYMBOL(rt_debug_word), sizeof z));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt_debug_word), &z, sizeof z));
    return RT_OK;
}
// debug builds only: poison every lane's traversal phase and stack depth at the lane-resident
// kernel's start (rt_mega_kernel), for the packing test
int rt_debug_set_poison(int on) {
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rt_debug_poison), &on, sizeof on));
    return RT_OK;
}
#endif

// rt_device_selfcheck 0: rcp_ieee against the IEEE division 1.f / x over every float x
// with a normal reciprocal path (|x| in [2^-126, 2^125)), on the device.
__global__ void __launch_bounds__(256) rcp_check_kernel(unsigned long long *bad) {
    unsigned long long local = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32);
         i += (uint64_t)gridDim.x * blockDim.x) {
        const float x = __uint_as_float((uint32_t)i);
        const float ax = fabsf(x);
        if (!(ax >= 0x1p-126f && ax < 0x1p125f)) continue;
        const float a = rtd::rcp_ieee(x), b = 1.f / x;
        local += __float_as_uint(a) != __float_as_uint(b);
    }
    check_count(local, bad);
}

// rt_device_selfcheck 1: the computed linear texel decode (rt_path.h unorm8) against the IEEE
// division (float)b / 255.f for every byte b, and the packed LDS RNG word (rt_mega.h
// rng_word_pack) round trip over the state range and both normal-cache flags.
__global__ void __launch_bounds__(256) decode_check_kernel(unsigned long long *bad) {
    unsigned long long local = 0;
    if (blockIdx.x == 0) {
        const uint32_t b = threadIdx.x;
        local += __float_as_uint(rtd::unorm8(b)) != __float_as_uint((float)b / 255.f);
    }
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2147483647ull;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = (uint32_t)i;
#pragma unroll
        for (uint32_t f = 0; f < 2; ++f) {
            uint32_t ux, uf;
            rtd::rng_word_unpack(rtd::rng_word_pack(x, f), ux, uf);
            local += (ux != x) | (uf != f);
        }
    }
    check_count(local, bad);
}

// rt_device_selfcheck 4: every material record of an uploaded scene (rt_material.h), read the
// way the shading pass reads it, against the scene's own tables on the device: the 12 mesh_f
// floats and 4 mesh_tex indices bit for bit, each slot's descriptor against its texture's
// tex_info row, (0, 1, 1) for an absent slot, zero padding; a present slot's texture must end
// inside the texel array (n_texels).  Counts the dwords that differ.
#if RT_SHADE_GATHER
__global__ void __launch_bounds__(256) mat_check_kernel(rtd::DevScene sc, unsigned long long n_texels, unsigned long long *bad) {
    unsigned long long local = 0;
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < sc.n_meshes; m += gridDim.x * blockDim.x) {
        uint32_t r[32];
        for (int q = 0; q < 8; ++q) {
            const uint4 x = sc.mat[8 * m + q];
            r[4 * q] = x.x; r[4 * q + 1] = x.y; r[4 * q + 2] = x.z; r[4 * q + 3] = x.w;
        }
        for (int k = 0; k < 12; ++k) local += r[k] != __float_as_uint(sc.mesh_f[12 * m + k]);
        for (int k = 0; k < 4; ++k) {
            const int t = sc.mesh_tex[4 * m + k];
            local += r[rtmat::kRecTex + k] != (uint32_t)t;
            uint4 ti = make_uint4(0u, 1u, 1u, 4u);
            if (t >= 0) {
                ti = sc.tex_info[t];
                local += (unsigned long long)ti.x + (unsigned long long)((ti.y + 3) / 4) * ((ti.z + 3) / 4) * 16 > n_texels;
            }
            const uint32_t *d = r + rtmat::kRecDesc + 3 * k;
            local += (d[0] != ti.x) + (d[1] != ti.y) + (d[2] != ti.z);
        }
        for (int k = 28; k < 32; ++k) local += r[k] != 0u;
    }
    check_count(local, bad);
}
#endif

// rt_device_selfcheck 3: the root-free cull (rt_wavefront.h far_gt, kFarMax2) against the
// device's own sqrtf(x) > acc: 2^24 of the host test's generated pairs (far_case_acc /
// far_case_x: every exponent of acc, x around acc * acc and around the exact boundary), the
// special values (zeros, denormals, perfect squares, inf, NaN) and the floats within 64 ulps
// of kFarMax2 against sqrtf(x) > 1e9f.
__global__ void __launch_bounds__(256) far_check_kernel(unsigned long long *bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // (2^24 threads)
    unsigned long long local = 0;
    {
        const uint32_t j = i / (uint32_t)rtd::kFarCaseXs, v = i % (uint32_t)rtd::kFarCaseXs;
        const float acc = rtd::far_case_acc(j % (uint32_t)rtd::kFarCaseExps, j / (uint32_t)rtd::kFarCaseExps);
        const float x = rtd::far_case_x(acc, (int)v);
        local += rtd::far_gt(x, acc) != (sqrtf(x) > acc);
    }
    if (i < 54u) {
        const float accs[6] = {0.f, -0.f, 1e-45f, 0x1p-126f, 1.f, 1e9f};
        const float xs[9] = {0.f, 1e-45f, 0x1p-126f, 1.f, 4.f, 9.f, 1e18f, __builtin_inff(), __builtin_nanf("")};
        const float acc = accs[i / 9u], x = xs[i % 9u];
        local += rtd::far_gt(x, acc) != (sqrtf(x) > acc);
    }
    if (i < 132u) {
        const float x = i < 129u ? rtd::far_case_step(rtd::kFarMax2, (int)i - 64)
                                 : (i == 129u ? 0.f : (i == 130u ? __builtin_inff() : __builtin_nanf("")));
        local += (x > rtd::kFarMax2) != (sqrtf(x) > 1e9f);
    }
    check_count(local, bad);
}

}  // extern "C"

// rt_device_selfcheck 2: the cooperative leaf step (rt_wavefront.h trav_step_coop: four
// helper lanes per leaf lane, DPP quad min with the triangle index as tie-break, NaN t as no
// hit, several leaf rounds) against the per-lane sequential loop of trav_step (the reference's
// in-order strict < of bvh.cpp:226-232 over primitive.cpp:17-57).  Leaves of 1-7 triangles
// over groups rich in exact duplicates (equal t, u, v), coplanar triangles (equal t), NaN and
// infinite vertices; every lane of a 256-thread block is a leaf lane, so each step serves 8 of
// a wave's 64 and the rest wait.  Both round policies (one round per step; rounds until every
// leaf lane is served).  One mismatching field of a case counts once.
template <int kLeaves>
__global__ void __launch_bounds__(256) coop_check_kernel(const float4 *tri, int n_tris, const float4 *nodes,
                                                          const float4 *rays, const uint2 *leaves, int n_cases,
                                                          int round_min, unsigned long long *bad) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const bool valid = i < n_cases;
    DevScene sc{};
    sc.tri = tri;
    sc.n_tris = n_tris;
    sc.node = nodes;
    sc.n_nodes = 2;
    const float4 ro = rays[2 * (valid ? i : 0)], rdv = rays[2 * (valid ? i : 0) + 1];
    const rtd::Ray r = rtd::make_ray(rtv::V3{ro.x, ro.y, ro.z}, rtv::V3{rdv.x, rdv.y, rdv.z});
    const uint2 lf = leaves[valid ? i : 0];
    rtd::TravState T;
    T.best.t = 1e9f;
    T.best.u = T.best.v = 0.f;
    T.best.prim = -1;
    T.acc = 1e9f;
    T.sp = 0;
    T.a = T.b = 0;
    T.k = lf.x;
    T.kend = lf.y;
    T.phase = rtd::TP_LEAF;
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    uint2 spill[rtd::kStack - 4];
    rtd::LdsStackT<4> S{spill};
    const rtd::GlobalNodes gn{nodes};
    bool active = valid;
    for (int it = 0; it < 64 && __any(active); ++it)   // (bounded: 7 triangles, 64 lanes, 8 per round)
        if (rtd::trav_step_coop<false, kLeaves, false>(sc, r, T, S, gn, cnt, active, round_min)) active = false;
    // the step keeps (t, triangle) only: (u, v) as the shading pass recomputes them
    if (rtd::kUvRecompute && valid && T.best.prim >= 0) rtd::hit_uv(sc, r, T.best);
    // sequential reference: trav_step's per-lane loop, one triangle at a time
    float acc = 1e9f;
    rtd::Hit best{1e9f, 0.f, 0.f, -1};
    for (uint32_t k = lf.x; valid && k < lf.y; ++k) {
        const float4 q0 = tri[3 * k], q1 = tri[3 * k + 1], q2 = tri[3 * k + 2];
        rtd::TriHit h;
        if (rtd::tri_hit_bl(rtv::V3{q0.x, q0.y, q0.z}, rtv::V3{q0.w, q1.x, q1.y}, rtv::V3{q1.z, q1.w, q2.x}, r, h)) {
            acc = h.t < acc ? h.t : acc;
            if (h.t < best.t) best = rtd::Hit{h.t, h.u, h.v, (int)k};
        }
    }
    unsigned long long local = 0;
    if (valid)
        local = (active | (T.best.prim != best.prim) | (__float_as_uint(T.best.t) != __float_as_uint(best.t)) |
                 (__float_as_uint(T.best.u) != __float_as_uint(best.u)) |
                 (__float_as_uint(T.best.v) != __float_as_uint(best.v)) | (__float_as_uint(T.acc) != __float_as_uint(acc)))
                    ? 1ull : 0ull;
    check_count(local, bad);
}

// rt_device_selfcheck 5: whole closest-hit queries on an uploaded scene through trav_step_coop (K
// stack frames in LDS, at most POPS frames popped per step, with every best frame or with none after a
// near subtree without a hit: ELIDE), against the per-lane trav_step loop, which pushes every best
// frame, over an ArrayStack in scratch, in the same kernel: t, triangle, the local best and the AABB
// and triangle counts, bit for bit.  The waves hold the real mix of node, leaf and pop lanes
// (the plain kernel's coop records, leaf rounds and leaf deferral); with K = 4 most waves hold
// lanes whose frames are in scratch.  Ray i starts inside the root box with a direction uniform
// on the sphere, both from a hash of i; every 64th lane is inactive from the start and the last
// wave has a single active lane.  Both loops are bounded by `bound` steps: a lane still
// traversing there counts as a mismatch (a liveness bug fails the check, it does not hang).
__device__ __forceinline__ uint32_t pop_check_hash(uint32_t x) {   // (lowbias32)
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// The whole queries of rt_device_selfcheck 5 and of rt_intersect_rays_via, each bounded by
// `bound` steps; false: the lane was still traversing there.  `bits`: the root box result as the
// producers store it (rt_wavefront.h store_qray, rt_mega.h mega_begin).
__device__ __forceinline__ uint32_t query_root_bits(const rtd::NodeRec &root, const rtd::Ray &r) {
    float e;
    return rtd::box_hit<false>(root.mn, root.mx, r, e) ? 0u : 8u;
}
// trav_step_coop with the plain kernel's constants; every lane of the wave calls (valid or not).
// ELIDE: no best frame after a near subtree without a hit (rt_wavefront.h trav_pop).
template <int POPS, bool ELIDE, class Stack>
__device__ __forceinline__ bool coop_query(const DevScene &sc, const rtd::NodeRec &root, const rtd::Ray &r, uint32_t bits,
                                           bool valid, int bound, rtd::TravStateU &T, Stack &S, Counters &cnt) {
    const rtd::GlobalNodes gn{sc.node};
    bool active = rtd::trav_start<true>(bits, root.a, root.b, T, cnt) && valid;
    int leaf_defer = 0;
    for (int it = 0; it < bound && __any(active); ++it)
        if (rtd::trav_step_coop<true, kCoopLeavesPlain, false, rtd::kLeafDeferPlain, kPlainFarDist2, POPS, ELIDE>(
                sc, r, T, S, gn, cnt, active, kCoopRoundMinPlain, rtd::NoHook{}, &leaf_defer))
            active = false;
    return !active;
}
// the per-lane trav_step loop (ELIDE as above)
template <bool DIST2, bool ELIDE, class Stack>
__device__ __forceinline__ bool lane_query(const DevScene &sc, const rtd::NodeRec &root, const rtd::Ray &r, uint32_t bits,
                                           bool valid, int bound, rtd::TravState &T, Stack &S, Counters &cnt) {
    const rtd::GlobalNodes gn{sc.node};
    bool active = rtd::trav_start<true>(bits, root.a, root.b, T, cnt) && valid;
    for (int it = 0; it < bound && active; ++it)
        if (rtd::trav_step<true, DIST2, ELIDE>(sc, r, T, S, gn, cnt)) active = false;
    return !active;
}
// ManyLightsDistribution::pdf(r.o, r.d) as the light-split kernel walks it (rt_mega.h
// mega_shade_split starts the walk, light_step is one node of it); lp: light_pdf's result.
template <class Stack>
__device__ __forceinline__ bool light_query(const DevScene &sc, const rtd::Ray &r, bool valid, int bound, Stack &S,
                                            Counters &cnt, float &lp) {
    const rtd::Ray lr = rtd::make_ray(r.o, r.d);   // light_pdf's Ray(point, direction)
    const float4 dq = make_float4(r.d.x, r.d.y, r.d.z, 0.f);
    rtd::TravState T;
    T.acc = 0.f;
    T.sp = 0;
    S.put(T.sp++, make_uint2(0u, 0u));
    cnt.lq++;
    bool active = valid;
    for (int it = 0; it < bound && active; ++it)
        if (rtd::light_step<true>(sc, lr, T, S, cnt, &dq)) active = false;
    lp = T.acc / (float)sc.n_lights;
    return !active;
}

template <int K, int POPS, bool ELIDE>
__global__ void __launch_bounds__(256) pop_check_kernel(DevScene sc, int n_rays, int bound, unsigned long long *bad) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int lane = (int)(threadIdx.x & 63);
    const bool last_wave = i >= n_rays - 64;
    const bool valid = i < n_rays && (last_wave ? lane == 0 : lane != 63);
    const rtd::NodeRec root = rtd::load_node(sc.node, 0);
    float u[6];
    for (int c = 0; c < 6; ++c) u[c] = (float)(pop_check_hash(6u * (uint32_t)i + (uint32_t)c) >> 8) * 0x1p-24f;
    rtv::V3 o{root.mn[0] + u[0] * (root.mx[0] - root.mn[0]), root.mn[1] + u[1] * (root.mx[1] - root.mn[1]),
              root.mn[2] + u[2] * (root.mx[2] - root.mn[2])};
    const float z = 2.f * u[3] - 1.f, ph = 6.28318530718f * u[4], s = sqrtf(fmaxf(0.f, 1.f - z * z));
    const rtd::Ray r = rtd::make_ray(o, rtv::V3{s * cosf(ph), s * sinf(ph), z});
    // the coop query
    rtd::TravStateU T;
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    uint2 spill[rtd::kStack - K];
    rtd::LdsStackT<K> S{spill};
    const bool active = !coop_query<POPS, ELIDE>(sc, root, r, 0u, valid, bound, T, S, cnt);
    // the per-lane query, with every best frame
    rtd::TravState T2;
    Counters cnt2{0, 0, 0, 0, 0, 0, 0};
    uint2 frames[rtd::kStack];
    rtd::ArrayStack S2{frames};
    const bool active2 = !lane_query<kPlainFarDist2, false>(sc, root, r, 0u, valid, bound, T2, S2, cnt2);
    unsigned long long local = 0;
    if (valid)
        local = (active | active2 | (T.best.prim != T2.best.prim) | (__float_as_uint(T.best.t) != __float_as_uint(T2.best.t)) |
                 (__float_as_uint(T.acc) != __float_as_uint(T2.acc)) | (cnt.aabb != cnt2.aabb) | (cnt.tri != cnt2.tri))
                    ? 1ull : 0ull;
    check_count(local, bad);
}

// The record of a ray query (include/rt_hw.h rt_intersect_rays_via): the caller's ray k, and its result: t, u, v
// (0 unless `ok`) and the light pdf; the status word, the triangle or -1, the tests of the scene walk c1 and the light walk c2.
__device__ __forceinline__ rtd::Ray query_ray(const float *org, const float *dir, long long k) {
    return rtd::make_ray(rtv::V3{org[3 * k], org[3 * k + 1], org[3 * k + 2]},
                         rtv::V3{dir[3 * k], dir[3 * k + 1], dir[3 * k + 2]});
}
__device__ __forceinline__ void query_store(float *out_f, long long *out_i, long long k, bool ok, const rtd::Hit &h, float lp,
                                            long long status, const Counters &c1, const Counters &c2) {
    out_f[4 * k + 0] = ok ? h.t : 0.f;
    out_f[4 * k + 1] = ok ? h.u : 0.f;
    out_f[4 * k + 2] = ok ? h.v : 0.f;
    out_f[4 * k + 3] = lp;
    out_i[6 * k + 0] = status;
    out_i[6 * k + 1] = ok ? h.prim : -1;
    out_i[6 * k + 2] = c1.aabb;
    out_i[6 * k + 3] = c1.tri;
    out_i[6 * k + 4] = c2.laabb;
    out_i[6 * k + 5] = c2.ltri;
}

// Ray-level entry: BVH::intersect + ManyLightsDistribution::pdf for explicit rays.
__global__ void __launch_bounds__(256) rt_rays_kernel(DevScene sc, long long n, const float *org, const float *dir,
                                                       float *out_f, long long *out_i) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    rtd::Ray r = query_ray(org, dir, k);
    Counters c1{0, 0, 0, 0, 0, 0, 0}, c2{0, 0, 0, 0, 0, 0, 0};
    rtd::Hit h;
    const bool ok = rtd::closest_hit<true>(sc, r, h, c1);
    const float lp = sc.n_lights ? rtd::light_pdf<true>(sc, r.o, r.d, c2) : 0.f;
    query_store(out_f, out_i, k, ok, h, lp, ok, c1, c2);
}

// rt_intersect_rays_via paths 1 and 2: the caller's ray k through the production traversals
// (thread k; threads past n take ray 0 and write nothing, since every lane of a wave must call
// the coop step).  Path 1: trav_step with the runahead kernel's cull form over an ArrayStack.
// Path 2: the coop query above, as rt_device_selfcheck 5 instantiates it with four LDS frames
// and the plain kernel's pop cap, then hit_uv.  Both then walk the light BVH with light_step
// over the same stack.  hit = -2: a loop reached its bound.
template <int PATH>
__global__ void __launch_bounds__(256) rt_rays_via_kernel(DevScene sc, long long n, int bound, int light_bound,
                                                           const float *org, const float *dir, float *out_f,
                                                           long long *out_i) {
    static_assert(PATH == 1 || PATH == 2, "path 0 is rt_rays_kernel");
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = k < n;
    const rtd::Ray r = query_ray(org, dir, valid ? k : 0);
    const rtd::NodeRec root = rtd::load_node(sc.node, 0);
    const uint32_t bits = query_root_bits(root, r);
    Counters c1{0, 0, 0, 0, 0, 0, 0}, c2{0, 0, 0, 0, 0, 0, 0};
    rtd::Hit h;
    bool done, light_done = true;
    float lp = 0.f;
    if constexpr (PATH == 1) {
        uint2 frames[rtd::kStack];
        rtd::ArrayStack S{frames};
        rtd::TravState T;
        done = lane_query<RT_SPEC_FAR_DIST2 != 0, RT_SPEC_ACC_ELIDE != 0>(sc, root, r, bits, valid, bound, T, S, c1);
        h = T.best;
        if (sc.n_lights) light_done = light_query(sc, r, valid, light_bound, S, c2, lp);
    } else {
        uint2 spill[rtd::kStack - 4];
        rtd::LdsStackT<4> S{spill};
        rtd::TravStateU T;
        done = coop_query<RT_PLAIN_MAX_POPS, kPlainAccElide>(sc, root, r, bits, valid, bound, T, S, c1);
        h = T.best;
        if (rtd::kUvRecompute && valid && h.prim >= 0) rtd::hit_uv(sc, r, h);
        if (sc.n_lights) light_done = light_query(sc, r, valid, light_bound, S, c2, lp);
    }
    if (!valid) return;
    const bool ok = h.prim >= 0;
    query_store(out_f, out_i, k, ok, h, lp, (done && light_done) ? (long long)ok : -2ll, c1, c2);
}

// rt_sample_frames_via: the caller's shading frame k (point, normal, eye, roughness2) on thread k, from
// Rng(seed[k]) with an empty normal cache, after warm[k] (0 or 1) polar normals, which fill it:
// scene_sample, then the pdf of the drawn direction.  Path 0: scene_pdf<true> over a LocalStack, as
// shade_hit and the wavefront shade kernel compose them (the light pdf alone is a second, uncounted
// light_pdf).  Path 1: light_query (the light_step walk, status -2 at its bound) and scene_pdf_lp, as
// both lane-resident families compose them.  Then one more polar normal and one engine output: the
// cache's flag and value and the number of draws.  The host has checked seed and warm, so the RNG's
// rejection loops end by themselves; no other loop here depends on the caller's values.
template <int PATH>
__global__ void __launch_bounds__(256) rt_frames_kernel(DevScene sc, long long n, int light_bound, const float *frame,
                                                         const uint32_t *seed, const uint32_t *warm, float *out_f,
                                                         long long *out_i) {
    static_assert(PATH == 0 || PATH == 1, "two compositions");
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float *f = frame + 10 * k;
    const rtv::V3 pos{f[0], f[1], f[2]}, N{f[3], f[4], f[5]}, eye{f[6], f[7], f[8]};
    const float r2 = f[9];
    rtd::Rng rng{seed[k], 0u, 0.f};
    if (warm[k]) (void)rtd::rng_normal(rng);
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    const rtv::V3 d = rtd::scene_sample(sc, pos, N, eye, r2, rng);
    float pdf, lp = 0.f;
    bool done = true;
    if constexpr (PATH == 0) {
        rtd::LocalStack S;
        pdf = rtd::scene_pdf<true>(sc, pos, N, eye, r2, d, cnt, S);
        Counters c2{0, 0, 0, 0, 0, 0, 0};
        if (sc.n_lights) lp = rtd::light_pdf<false>(sc, pos, d, c2, S);
    } else {
        if (sc.n_lights) {
            rtd::LocalStack S;
            rtd::Ray q;   // (light_query makes light_pdf's Ray(point, direction) of these two)
            q.o = pos;
            q.d = d;
            q.inv = d;
            done = light_query(sc, q, true, light_bound, S, cnt, lp);
        }
        pdf = rtd::scene_pdf_lp(sc, N, eye, r2, d, lp);
    }
    out_f[6 * k + 0] = d.x;
    out_f[6 * k + 1] = d.y;
    out_f[6 * k + 2] = d.z;
    out_f[6 * k + 3] = pdf;
    out_f[6 * k + 4] = lp;
    out_f[6 * k + 5] = rtd::rng_normal(rng);
    out_i[4 * k + 0] = done ? 0ll : -2ll;
    out_i[4 * k + 1] = (long long)rtd::rng_next(rng);
    out_i[4 * k + 2] = cnt.laabb;
    out_i[4 * k + 3] = cnt.ltri;
}

namespace {
// Host-made cases of selfcheck 2 (deterministic): 8-triangle groups of a base triangle, its
// exact copy, a coplanar one behind an equal-t prefix, its copy, a NaN-vertex one, a random
// one, the base again and an infinite-vertex one; rays from random origins at the base's
// centroid (jittered); leaves of 1-7 consecutive triangles.
void coop_cases(std::vector<float> &tri, std::vector<float> &rays, std::vector<uint32_t> &leaves, int n_cases) {
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {   // [0, 1)
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return (float)((x >> 40) & 0xffffff) / 16777216.f;
    };
    const int groups = 512;
    tri.assign((size_t)groups * 8 * 12, 0.f);
    std::vector<float> cen((size_t)groups * 3);
    for (int gi = 0; gi < groups; ++gi) {
        float v0[3], U[3], V[3];
        for (int c = 0; c < 3; ++c) {
            v0[c] = rnd() * 4.f - 2.f;
            U[c] = rnd() * 2.f - 1.f;
            V[c] = rnd() * 2.f - 1.f;
            cen[3 * gi + c] = v0[c] + (U[c] + V[c]) / 3.f;
        }
        for (int t = 0; t < 8; ++t) {
            float *o = &tri[((size_t)gi * 8 + t) * 12];
            float a[3], u[3], w[3];
            for (int c = 0; c < 3; ++c) {
                a[c] = v0[c]; u[c] = U[c]; w[c] = V[c];
                if (t == 2 || t == 3) { a[c] = v0[c] + 0.25f * U[c]; }   // same plane, shifted: equal t, other u
                if (t == 5) { a[c] = rnd() * 4.f - 2.f; u[c] = rnd() * 2.f - 1.f; w[c] = rnd() * 2.f - 1.f; }
            }
            if (t == 4) a[1] = __builtin_nanf("");
            if (t == 7) u[0] = __builtin_inff();
            for (int c = 0; c < 3; ++c) { o[c] = a[c]; o[3 + c] = u[c]; o[6 + c] = w[c]; }
        }
    }
    rays.assign((size_t)n_cases * 8, 0.f);
    leaves.assign((size_t)n_cases * 2, 0u);
    for (int i = 0; i < n_cases; ++i) {
        const int gi = (int)(rnd() * groups) % groups;
        float o[3], d[3];
        for (int c = 0; c < 3; ++c) {
            o[c] = rnd() * 20.f - 10.f;
            d[c] = cen[3 * gi + c] + (rnd() - 0.5f) * 0.2f - o[c];
        }
        for (int c = 0; c < 3; ++c) { rays[8 * (size_t)i + c] = o[c]; rays[8 * (size_t)i + 4 + c] = d[c]; }
        const uint32_t len = 1u + (uint32_t)(rnd() * 7.f) % 7u, first = (uint32_t)gi * 8u + (uint32_t)(rnd() * 8.f) % 8u;
        const uint32_t k0 = std::min<uint32_t>(first, (uint32_t)groups * 8u - len);
        leaves[2 * (size_t)i] = k0;
        leaves[2 * (size_t)i + 1] = k0 + len;
    }
}
struct CoopCases {   // those cases on the device, as coop_check_kernel takes them (nodes: a block of zeros)
    const float4 *tri, *nodes, *rays;
    const uint2 *leaves;
    int n_tris;
};
struct DeviceBuf {   // device memory released on every return path
    uint8_t *p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc((void **)&p, bytes); }
    ~DeviceBuf() { (void)hipFree(p); }
};
// The u64 a check's kernels count into, on the current device, and `cases` bytes for the check's inputs 256 bytes
// after it: make() allocates and zeroes both, `d` goes to the launches, report() reads it back; freed on every return path.
struct CheckCount {
    const char *who = "rt_device_selfcheck: ";   // the prefix of the check's device failures
    DeviceBuf buf;
    unsigned long long *d = nullptr;
    int make(size_t cases = 0) {
        HIP_TRY_AS(who, buf.alloc(256 + cases));
        HIP_TRY_AS(who, hipMemset(buf.p, 0, 256 + cases));
        d = (unsigned long long *)buf.p;
        return RT_OK;
    }
    int report(uint64_t *count) {   // (*count is written on success only)
        unsigned long long h = 0;
        HIP_TRY_AS(who, hipGetLastError());
        HIP_TRY_AS(who, hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
        *count = h;
        return RT_OK;
    }
};
// Checks 0, 1 and 3: one launch on the current device, no scene.
int bare_selfcheck(void (*kernel)(unsigned long long *), unsigned blocks, uint64_t *mismatches) {
    CheckCount c;
    if (int rc = c.make()) return rc;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, nullptr, c.d);
    return c.report(mismatches);
}
int rcp_selfcheck(uint64_t *mismatches) { return bare_selfcheck(rcp_check_kernel, 4096, mismatches); }
int decode_selfcheck(uint64_t *mismatches) { return bare_selfcheck(decode_check_kernel, 4096, mismatches); }
int far_selfcheck(uint64_t *mismatches) { return bare_selfcheck(far_check_kernel, (1u << 24) / 256u, mismatches); }
int coop_selfcheck(uint64_t *mismatches) {
    const int n_cases = 1 << 16;
    std::vector<float> tri, rays;
    std::vector<uint32_t> leaves;
    coop_cases(tri, rays, leaves, n_cases);
    // the cases' bytes: the triangles and 64 bytes past them, the rays, the leaves, the node block
    const size_t bt = tri.size() * 4 + 64, br = rays.size() * 4, bl = leaves.size() * 4, bn = 256;
    CheckCount c;
    if (int rc = c.make(bt + br + bl + bn)) return rc;
    uint8_t *b = c.buf.p + 256;
    const CoopCases v{(const float4 *)b, (const float4 *)(b + bt + br + bl), (const float4 *)(b + bt), (const uint2 *)(b + bt + br),
                      (int)(tri.size() / 12)};
    HIP_TRY_AS(c.who, hipMemcpy(b, tri.data(), tri.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY_AS(c.who, hipMemcpy(b + bt, rays.data(), br, hipMemcpyHostToDevice));
    HIP_TRY_AS(c.who, hipMemcpy(b + bt + br, leaves.data(), bl, hipMemcpyHostToDevice));
    for (int rm : {65, 1})   // one round per step; every leaf lane served in the step
        for (auto kernel : {coop_check_kernel<8>, coop_check_kernel<16>})
            hipLaunchKernelGGL(kernel, dim3((unsigned)(n_cases / 256)), dim3(256), 0, nullptr, v.tri, v.n_tris, v.nodes, v.rays,
                               v.leaves, n_cases, rm, c.d);
    return c.report(mismatches);
}
// Checks 4 and 5: over every device copy that exists (an error where there is none), the sum of the
// copies' counts.  per_copy(copy, counter) refuses the copy or makes the counter and launches.
template <class F>
int selfcheck_every_copy(const char *who, uint64_t *mismatches, F per_copy) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    if (g_live.empty()) return rt_fail(RT_ERR_ARG, std::string(who) + "no scene is uploaded");
    uint64_t total = 0, h = 0;
    for (rt_device_scene *ds : g_live) {
        DeviceGuard guard(ds->device);
        if (!guard.ok) return rt_fail(RT_ERR_DEVICE, std::string(who) + "hipSetDevice failed");
        CheckCount c{who};
        if (int rc = per_copy(*ds, c)) return rc;
        if (int rc = c.report(&h)) return rc;
        total += h;
    }
    *mismatches = total;
    return RT_OK;
}
int mat_selfcheck(uint64_t *mismatches) {
#if RT_SHADE_GATHER
    return selfcheck_every_copy("rt_device_selfcheck 4: ", mismatches, [](const rt_device_scene &ds, CheckCount &c) -> int {
        if (int rc = c.make()) return rc;
        hipLaunchKernelGGL(mat_check_kernel, dim3(64), dim3(256), 0, nullptr, ds.ds, (unsigned long long)ds.n_texels, c.d);
        return RT_OK;
    });
#else
    return rt_fail(RT_ERR_ARG, "rt_device_selfcheck 4: built without RT_SHADE_GATHER");
#endif
}
int pop_selfcheck(uint64_t *mismatches) {
    return selfcheck_every_copy("rt_device_selfcheck 5: ", mismatches, [](const rt_device_scene &ds, CheckCount &c) -> int {
        if (ds.ds.n_nodes < 1 || ds.ds.n_tris < 1) return rt_fail(RT_ERR_ARG, "rt_device_selfcheck 5: empty scene");
        const int n_rays = 16384;
        const long long bound = 4ll * ((long long)ds.ds.n_nodes + ds.ds.n_tris) + 64;
        if (bound > 0x7fffffffll) return rt_fail(RT_ERR_LIMIT, "rt_device_selfcheck 5: scene too large");
        if (int rc = c.make()) return rc;
        // (4: frames in scratch in most waves; both frame rules, rt_wavefront.h trav_pop ELIDE)
        for (auto kernel : {pop_check_kernel<rtd::kLdsStack, 1, false>, pop_check_kernel<rtd::kLdsStack, 2, false>,
                            pop_check_kernel<4, 1, false>, pop_check_kernel<4, 2, false>,
                            pop_check_kernel<rtd::kLdsStack, 1, true>, pop_check_kernel<rtd::kLdsStack, 2, true>,
                            pop_check_kernel<4, 1, true>, pop_check_kernel<4, 2, true>})
            hipLaunchKernelGGL(kernel, dim3((unsigned)(n_rays / 256)), dim3(256), 0, nullptr, ds.ds, n_rays, (int)bound, c.d);
        return RT_OK;
    });
}
}  // namespace

extern "C" {

int rt_intersect_rays_via(rt_scene *s, int32_t path, int64_t n, const float *org, const float *dir, float *out_f,
                          int64_t *out_i) {
    const char *who = "rt_intersect_rays: ";
    if (!s || n < 0 || (n > 0 && (!org || !dir || !out_f || !out_i))) return rt_fail(RT_ERR_ARG, "rt_intersect_rays: bad argument");
    if (path < 0 || path > 2) return rt_fail(RT_ERR_ARG, "rt_intersect_rays_via: unknown path " + std::to_string(path));
    if (n == 0) return RT_OK;
    if (int rc = ensure_device_scene(s, 0)) return rc;
    DeviceGuard guard(0);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const DevScene &sc = s->dev[0]->ds;
    // (a walk visits every node and triangle at most once; the factor covers deferred steps)
    const long long bound = 4ll * ((long long)sc.n_nodes + sc.n_tris) + 64, light_bound = 8ll * sc.n_lights + 64;
    if (path != 0 && (sc.n_nodes < 1 || sc.n_tris < 1)) return rt_fail(RT_ERR_ARG, "rt_intersect_rays_via: empty scene");
    if (bound > 0x7fffffffll || light_bound > 0x7fffffffll) return rt_fail(RT_ERR_LIMIT, "rt_intersect_rays_via: scene too large");
    // one buffer: the integer results (8-byte words), the float results, the origins, the directions
    const size_t bi = (size_t)n * 6 * sizeof(long long), bf = (size_t)n * 4 * sizeof(float), v3 = (size_t)n * 3 * sizeof(float);
    DeviceBuf buf;
    HIP_TRY_AS(who, buf.alloc(bi + bf + 2 * v3));
    long long *d_i = (long long *)buf.p;
    float *d_f = (float *)(buf.p + bi), *d_o = (float *)(buf.p + bi + bf), *d_d = (float *)(buf.p + bi + bf + v3);
    HIP_TRY_AS(who, hipMemcpy(d_o, org, v3, hipMemcpyHostToDevice));
    HIP_TRY_AS(who, hipMemcpy(d_d, dir, v3, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (path == 0)
        hipLaunchKernelGGL(rt_rays_kernel, grid, block, 0, nullptr, sc, (long long)n, d_o, d_d, d_f, d_i);
    else
        hipLaunchKernelGGL(path == 1 ? rt_rays_via_kernel<1> : rt_rays_via_kernel<2>, grid, block, 0, nullptr, sc, (long long)n,
                           (int)bound, (int)light_bound, d_o, d_d, d_f, d_i);
    HIP_TRY_AS(who, hipGetLastError());
    HIP_TRY_AS(who, hipMemcpy(out_f, d_f, bf, hipMemcpyDeviceToHost));
    HIP_TRY_AS(who, hipMemcpy(out_i, d_i, bi, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_intersect_rays(rt_scene *s, int64_t n, const float *org, const float *dir, float *out_f, int64_t *out_i) {
    return rt_intersect_rays_via(s, 0, n, org, dir, out_f, out_i);
}

int rt_sample_frames_via(rt_scene *s, int32_t path, int64_t n, const float *frame, const uint32_t *seed, const uint32_t *warm,
                         float *out_f, int64_t *out_i) {
    const char *who = "rt_sample_frames_via: ";
    if (!s || n < 0 || (n > 0 && (!frame || !seed || !warm || !out_f || !out_i)))
        return rt_fail(RT_ERR_ARG, "rt_sample_frames_via: bad argument");
    if (path < 0 || path > 1) return rt_fail(RT_ERR_ARG, "rt_sample_frames_via: unknown path " + std::to_string(path));
    // (an engine state of 0 or 2^31 - 1 stays there, and the polar loop would not end on it)
    for (int64_t k = 0; k < n; ++k) {
        if (seed[k] < 1u || seed[k] > 2147483646u)
            return rt_fail(RT_ERR_ARG, "rt_sample_frames_via: seed of frame " + std::to_string(k) + " is outside 1 .. 2147483646");
        if (warm[k] > 1u) return rt_fail(RT_ERR_ARG, "rt_sample_frames_via: warm of frame " + std::to_string(k) + " is neither 0 nor 1");
    }
    if (n == 0) return RT_OK;
    if (n > (1ll << 30)) return rt_fail(RT_ERR_LIMIT, "rt_sample_frames_via: more than 2^30 frames");
    if (int rc = ensure_device_scene(s, 0)) return rc;
    DeviceGuard guard(0);
    if (!guard.ok) return rt_fail(RT_ERR_DEVICE, "hipSetDevice failed");
    const DevScene &sc = s->dev[0]->ds;
    const long long light_bound = 8ll * sc.n_lights + 64;   // (as rt_intersect_rays_via's)
    if (light_bound > 0x7fffffffll) return rt_fail(RT_ERR_LIMIT, "rt_sample_frames_via: scene too large");
    // one buffer: the integer results (8-byte words), the float results, the frames, the seeds, the warm flags
    const size_t bi = (size_t)n * 4 * sizeof(long long), bf = (size_t)n * 6 * sizeof(float), bfr = (size_t)n * 10 * sizeof(float),
                 bw = (size_t)n * sizeof(uint32_t);
    DeviceBuf buf;
    HIP_TRY_AS(who, buf.alloc(bi + bf + bfr + 2 * bw));
    long long *d_i = (long long *)buf.p;
    float *d_f = (float *)(buf.p + bi), *d_fr = (float *)(buf.p + bi + bf);
    uint32_t *d_s = (uint32_t *)(buf.p + bi + bf + bfr), *d_w = (uint32_t *)(buf.p + bi + bf + bfr + bw);
    HIP_TRY_AS(who, hipMemcpy(d_fr, frame, bfr, hipMemcpyHostToDevice));
    HIP_TRY_AS(who, hipMemcpy(d_s, seed, bw, hipMemcpyHostToDevice));
    HIP_TRY_AS(who, hipMemcpy(d_w, warm, bw, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(path == 0 ? rt_frames_kernel<0> : rt_frames_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       nullptr, sc, (long long)n, (int)light_bound, d_fr, d_s, d_w, d_f, d_i);
    HIP_TRY_AS(who, hipGetLastError());
    HIP_TRY_AS(who, hipMemcpy(out_f, d_f, bf, hipMemcpyDeviceToHost));
    HIP_TRY_AS(who, hipMemcpy(out_i, d_i, bi, hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_device_selfcheck(int32_t which, uint64_t *mismatches) {
    static int (*const checks[])(uint64_t *) = {rcp_selfcheck, decode_selfcheck, coop_selfcheck,
                                                far_selfcheck, mat_selfcheck, pop_selfcheck};
    if (!mismatches) return rt_fail(RT_ERR_ARG, "rt_device_selfcheck: null output");
    if (which < 0 || which >= (int32_t)(sizeof checks / sizeof *checks))
        return rt_fail(RT_ERR_ARG, "rt_device_selfcheck: unknown check " + std::to_string(which));
    return checks[which](mismatches);
}

}  // extern "C"
