// rt_gbuffer.h — the first-hit feature record of a pixel (include/rt_hw.h rt_gbuffer).
//
// One record per pixel from the pixel-centre camera ray, camera_ray(sc, i, j, 0.f, 0.f): no
// random number is drawn, so the record depends on neither spp nor an accumulator.  The
// attribute operations restate those of shade_pre / shade_post (rt_path.h) in the same order,
// in a function of their own: nothing rt_mega_kernel instantiates is touched, so the render
// kernels' code generation stays what it was.  Built for the device by rt_device.hip
// (rt_gbuffer_kernel) and for the host by tests/native/gbuffer_host.cpp, like rt_path.h.
//
// The record is four float4 (64 B):
//   0: shading normal N.xyz, hit distance t
//   1: base colour (albedo).xyz, triangle id (int bits)
//   2: emission.xyz, mesh id (int bits)
//   3: hit position P = o + d * t, 0
// A miss (closest_hit fails, or t >= max_distance: trace_sample's test) is all-zero words with
// both ids -1.
#pragma once
#include "rt_path.h"

namespace rtd {

constexpr int kGbufferQuads = 4;   // float4 per record

struct GRecord {
    float4 q[kGbufferQuads];
};

__device__ __forceinline__ GRecord gbuffer_miss() {
    GRecord g;
    g.q[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    g.q[1] = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    g.q[2] = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
    g.q[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    return g;
}

// The attributes of one hit: emission, shading normal and position as shade_pre computes them
// (the normal before the sampled-direction fallback to the geometric normal), the base colour
// as shade_post does.
__device__ __forceinline__ GRecord gbuffer_hit(const DevScene &sc, const Ray &r, const Hit &hit) {
    const int id = hit.prim;
    const float u = hit.u, v = hit.v;
    const float4 t2 = sc.tri[3 * id + 2];
    const V3 ngeo{t2.y, t2.z, t2.w};
    const bool inside = rtv::dot(r.d, ngeo) > 0;
    const float4 a0 = sc.tri_attr[4 * id], a1 = sc.tri_attr[4 * id + 1], a2 = sc.tri_attr[4 * id + 2],
                 a3 = sc.tri_attr[4 * id + 3];
    const int mesh = __float_as_int(a3.w);
    const float *mf = sc.mesh_f + 12 * mesh;
    const int *mt = sc.mesh_tex + 4 * mesh;
    const int mt_b = mt[0], mt_n = mt[1], mt_e = mt[3];
    const float w = 1 - u - v;
    const V2 tc{w * a2.y + u * a2.w + v * a3.y, w * a2.z + u * a3.x + v * a3.z};
    // Primitive::get_emission (primitive.cpp:121-129)
    V3 emission{mf[3], mf[4], mf[5]};
    if (mt_e >= 0) emission = rtv::mulv(rtv::reduce(tex_sample(sc, mt_e, tc, true)), emission);
    // Primitive::get_shading_normal (primitive.cpp:86-105)
    V3 n0{a0.x, a0.y, a0.z}, n1{a0.w, a1.x, a1.y}, n2{a1.z, a1.w, a2.x};
    V3 lz = rtv::normal(rtv::add(rtv::add(rtv::mul(n0, w), rtv::mul(n1, u)), rtv::mul(n2, v)));
    V3 N = lz;
    if (mt_n >= 0) {
        const float4 g0 = sc.tri_tan[3 * id], g1 = sc.tri_tan[3 * id + 1], g2 = sc.tri_tan[3 * id + 2];
        V3 t0{g0.x, g0.y, g0.z}, t1{g1.x, g1.y, g1.z}, tt2{g2.x, g2.y, g2.z};
        V3 lx = rtv::normal(mul_vector_d(sc.mesh_nt + 16 * mesh,
                                         rtv::normal(rtv::add(rtv::add(rtv::mul(t0, w), rtv::mul(t1, u)), rtv::mul(tt2, v)))));
        V3 ly = rtv::mul(rtv::cross(lz, lx), g0.w);
        V3 s = rtv::reduce(tex_sample(sc, mt_n, tc, false));
        V3 ln = rtv::mul(rtv::addf(s, -0.5f), 2.f);
        N = rtv::normal(rtv::add(rtv::add(rtv::mul(lx, ln.x), rtv::mul(ly, ln.y)), rtv::mul(lz, ln.z)));
    }
    if (inside) N = rtv::neg(N);
    const V3 pos = rtv::add(r.o, rtv::mul(r.d, hit.t));
    // the base colour of shade_post (scene.cpp:134-154)
    V3 base{mf[0], mf[1], mf[2]};
    if (mt_b >= 0) base = rtv::mulv(rtv::reduce(tex_sample(sc, mt_b, tc, true)), base);
    GRecord g;
    g.q[0] = make_float4(N.x, N.y, N.z, hit.t);
    g.q[1] = make_float4(base.x, base.y, base.z, __int_as_float(id));
    g.q[2] = make_float4(emission.x, emission.y, emission.z, __int_as_float(mesh));
    g.q[3] = make_float4(pos.x, pos.y, pos.z, 0.f);
    return g;
}

// The record of frame pixel (i, j); ray_out (may be null) receives the ray it cast.
__device__ __forceinline__ GRecord gbuffer_pixel(const DevScene &sc, int i, int j, Ray *ray_out = nullptr) {
    const Ray r = camera_ray(sc, i, j, 0.f, 0.f);
    if (ray_out) *ray_out = r;
    Hit hit;
    Counters cnt{0, 0, 0, 0, 0, 0, 0};
    const bool ok = closest_hit<false>(sc, r, hit, cnt);
    if (!(ok && hit.t < sc.max_distance)) return gbuffer_miss();
    return gbuffer_hit(sc, r, hit);
}

}  // namespace rtd
