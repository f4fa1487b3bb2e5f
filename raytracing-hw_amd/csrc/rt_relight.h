// rt_relight.h — the light list and the light BVH of a scene whose emissive triangles moved (host
// and device, no HIP).
//
// A scene that opted in (include/rt_hw.h rt_scene_enable_light_updates) lets rt_scene_update_tris*
// replace emissive triangles too; the light record of each and every box of the light BVH then
// follow from the triangle records, as the reference's build derives them (random.cpp:156-168
// makes the light list from the emissive primitives and a BVH over it with the scene's builder):
//   record    words 0..11 are the triangle record's words as given (v0, U, V and the caller's
//             geometric normal; nothing is normalised), word 12 the area
//             0.5f * length(cross(U, V)) with rt_vec.h's cross and length
//             (Primitive::get_geometric_normal, primitive.cpp:77-84); words 13..15 are not written
//   boxes     rt_refit.h's rule over the light records: tri_box over words 0..8 of each record,
//             a leaf folds its lights first .. first + count - 1 in order, an internal node
//             grow(left) then grow(right), every fold from the empty box, selects not min / max
// The order of the lights and the light tree's topology are kept.  The host functions (rt_host.cpp
// rt_relight_view, rt_scene_update_tris), the device kernels (rt_refit_device.h) and the CPU tests
// share this one text; what rt_refit.h says about fast-math flags holds here too.
#pragma once
#include "rt_refit.h"
#include "rt_vec.h"

namespace rtrl {

constexpr uint32_t kNoLight = 0xFFFFFFFFu;

// Word 12 of a light record from words 3..8 of its triangle's record (U, V).
RT_HD float light_area(float ux, float uy, float uz, float vx, float vy, float vz) {
    return 0.5f * rtv::length(rtv::cross(rtv::V3{ux, uy, uz}, rtv::V3{vx, vy, vz}));
}

// Words 0..12 of a light record (16 words) from a triangle record (12 words).
RT_HD void light_from_tri(const float *tri, float *light) {
    for (int w = 0; w < 12; ++w) light[w] = tri[w];
    light[12] = light_area(tri[3], tri[4], tri[5], tri[6], tri[7], tri[8]);
}

// A light leaf's box: the fold over its lights; light = the scene's `light` array (16 words per record).
RT_HD rtrf::Box leaf_box(const float *light, uint32_t first, uint32_t count) {
    rtrf::Box b = rtrf::empty_box();
    for (uint32_t k = 0; k < count; ++k) {
        const float *t = light + 16 * (size_t)(first + k);
        rtrf::grow_box(b, rtrf::tri_box(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]));
    }
    return b;
}

// One light node's box into the first six words of its record; a and b are only read.
RT_HD void refit_node(const float *light, float *node, size_t id) {
    float *rec = node + 8 * id;
    const uint32_t a = rtrf::word_bits(rec[6]), b = rtrf::word_bits(rec[7]);
    const rtrf::Box bx =
        rtrf::is_leaf(b) ? leaf_box(light, a, b >> 2) : rtrf::pair_box(node + 8 * (size_t)a, node + 8 * ((size_t)a + 1));
    for (int c = 0; c < 3; ++c) rec[c] = bx.lo[c], rec[3 + c] = bx.hi[c];
}

// Children come after their parents in light_node (build order): one reverse sweep.
inline void refit_sweep(const float *light, float *node, size_t n_nodes) {
    for (size_t i = n_nodes; i-- > 0;) refit_node(light, node, i);
}

}  // namespace rtrl
