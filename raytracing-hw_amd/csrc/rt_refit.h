// rt_refit.h — the boxes of a BVH whose triangles moved (host and device, no HIP).
//
// rt_scene_update_tris (include/rt_hw.h) replaces triangle records and then recomputes every node
// box bottom-up, keeping the tree's topology and the primitive order.  The rule restates what the
// reference's build computes for the same ranges: Primitive::aabb() is AABB::grow over v0, v0 + U,
// v0 + V (primitive.cpp:63-75), a node's box is grow over the boxes of its primitive range in order
// (bvh.cpp:131-133), and grow is std::min / std::max per component (primitive.h:22-30):
//   select    smin(a, b) = b < a ? b : a,  smax(a, b) = a < b ? b : a  (the bound is kept on a tie
//             and on a NaN, so a bound's bits are those of the first element that attains it, +0
//             and -0 keep their order, and a NaN component is never taken)
//   start     every fold starts from the empty box (+FLT_MAX, -FLT_MAX)
//   triangle  grow over v0, v0 + U, v0 + V in that order, each sum one f32 add per component
//   leaf      grow over the boxes of triangles first .. first + count - 1, in order
//   internal  grow(left child's box), then grow(right child's box)
// A fold of selects that keep the first attaining element does not depend on how the sequence is
// bracketed, so the internal rule gives the reference's sequential fold over the node's whole range.
// The host function (rt_host.cpp rt_refit_view), the device kernels (rt_refit_device.h) and the CPU
// tests share this one text.  The selects must stay compare-and-select: a min / max instruction
// ranks -0 below +0 and treats a NaN differently (no fast-math flag may apply to a translation unit
// that includes this file; tests/test_refit.py and tests/test_gpu_refit.py hold the +-0 / NaN cases).
#pragma once
#include <cfloat>
#include <cstdint>

#include "rt_libm.h"

namespace rtrf {

struct Box {
    float lo[3], hi[3];
};

RT_HD float smin(float a, float b) { return (b < a) ? b : a; }   // std::min
RT_HD float smax(float a, float b) { return (a < b) ? b : a; }   // std::max

// The device compiler may fold a select against a constant it knows (not NaN, not zero) into
// v_min_f32 / v_max_f32: the same value there, but the listing is then harder to check.  The empty
// box's bounds pass through an empty asm statement, so every select of the kernels stays
// v_cmp_lt_f32 + v_cndmask_b32.
RT_HD float opaque_word(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}

RT_HD Box empty_box() {
    const float lo = opaque_word(FLT_MAX), hi = opaque_word(-FLT_MAX);
    return {{lo, lo, lo}, {hi, hi, hi}};
}

RT_HD void grow_point(Box &b, float x, float y, float z) {   // AABB::grow(vector3f)
    b.lo[0] = smin(b.lo[0], x), b.lo[1] = smin(b.lo[1], y), b.lo[2] = smin(b.lo[2], z);
    b.hi[0] = smax(b.hi[0], x), b.hi[1] = smax(b.hi[1], y), b.hi[2] = smax(b.hi[2], z);
}

RT_HD void grow_box(Box &b, const Box &o) {   // AABB::grow(AABB)
    for (int c = 0; c < 3; ++c) b.lo[c] = smin(b.lo[c], o.lo[c]);
    for (int c = 0; c < 3; ++c) b.hi[c] = smax(b.hi[c], o.hi[c]);
}

// Primitive::aabb() of a `tri` record's first nine words: v0, U, V.
RT_HD Box tri_box(float v0x, float v0y, float v0z, float ux, float uy, float uz, float vx, float vy, float vz) {
    Box b = empty_box();
    grow_point(b, v0x, v0y, v0z);
    grow_point(b, v0x + ux, v0y + uy, v0z + uz);
    grow_point(b, v0x + vx, v0y + vy, v0z + vz);
    return b;
}

// A leaf's box: the fold over its triangles; tri = the scene's `tri` array (12 words per record).
RT_HD Box leaf_box(const float *tri, uint32_t first, uint32_t count) {
    Box b = empty_box();
    for (uint32_t k = 0; k < count; ++k) {
        const float *t = tri + 12 * (size_t)(first + k);
        grow_box(b, tri_box(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]));
    }
    return b;
}

// An internal node's box from its children's (the first six words of their records).
RT_HD Box pair_box(const float *left, const float *right) {
    Box b = empty_box();
    grow_box(b, Box{{left[0], left[1], left[2]}, {left[3], left[4], left[5]}});
    grow_box(b, Box{{right[0], right[1], right[2]}, {right[3], right[4], right[5]}});
    return b;
}

RT_HD bool is_leaf(uint32_t b_word) { return (b_word & 3u) == 3u; }

RT_HD uint32_t word_bits(float f) {
    union { float f; uint32_t u; } c;
    c.f = f;
    return c.u;
}

// One node's box into the first six words of its record; a and b (words 6, 7) are only read.
// `node`: the array the record's child id indexes.
RT_HD void refit_node(const float *tri, float *node, size_t id) {
    float *rec = node + 8 * id;
    const uint32_t a = word_bits(rec[6]), b = word_bits(rec[7]);
    const Box bx = is_leaf(b) ? leaf_box(tri, a, b >> 2) : pair_box(node + 8 * (size_t)a, node + 8 * ((size_t)a + 1));
    for (int c = 0; c < 3; ++c) rec[c] = bx.lo[c], rec[3 + c] = bx.hi[c];
}

// The host function: children come after their parents in the array (BVH::buildBVH order, and the
// breadth-first numbering too), so one reverse sweep refits the whole tree.
inline void refit_sweep(const float *tri, float *node, size_t n_nodes) {
    for (size_t i = n_nodes; i-- > 0;) refit_node(tri, node, i);
}

}  // namespace rtrf
