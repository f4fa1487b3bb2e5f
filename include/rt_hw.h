/* rt_hw.h — C ABI of the MI355X path-tracing core (librt_hw_amd.so).
 *
 * The reference (Korinin38/raytracing-hw) has no plugin API; its hot path is reached
 * through three C++ calls made by src/main.cpp:46-57.  Each entry point below replaces
 * one of them (plain pointers and sizes, no C++ or torch types, never throws):
 *
 *   rt_scene_load_gltf   <- parse_scene_gltf            src/io/scene_parser.cpp:25-350
 *                           + Scene::Scene (BVH build, light list)  src/core/scene.cpp:197-249
 *   rt_render / rt_render_device
 *                        <- Scene::render sample loop   src/core/scene.cpp:17-52
 *                           (per-pixel float RGB sums = sample_canvas, scene.cpp:20,42)
 *   rt_render_frame      <- the same loop over every GPU of the node (one row-block shard
 *                           per device), finished to 8 bits on each device and gathered
 *                           device-to-device onto one GPU (scene.cpp:17-64, canvas.h:76-89)
 *   rt_render_multi      <- the float frame of the same split (ABI 3 entry)
 *   rt_tonemap_u8        <- Scene::render frame finish  src/core/scene.cpp:54-64
 *   rt_tonemap_u8_device <- the same finish on the GPU   src/core/scene.cpp:54-64
 *   rt_write_ppm         <- Canvas::write_to            src/render/canvas.h:76-89
 *   rt_gbuffer, rt_denoise*  (no reference counterpart: the first hit's features and a filter
 *                           for low-sample previews in front of the finish)
 *   rt_last_error        <- the reference's std::runtime_error messages (23 throw sites);
 *                           the host wrappers re-throw them (drop-in failure behaviour).
 *
 * RNG convention: pixel (i,j) runs minstd_rand seeded with j*W+i
 * (pixel 0 -> state 1) and a polar-normal cache reset at the pixel start, so output does
 * not depend on threads, GPUs or the pixel partition.
 *
 * Status codes: 0 = OK, < 0 = error (message in rt_last_error(), thread-local).
 */
#ifndef RT_HW_H
#define RT_HW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6   /* 6: RT_FLAG_POOL and RT_SCHED_POOL removed (the path pool, round 5) */

enum rt_status {
    RT_OK = 0,
    RT_ERR_ARG = -1,      /* bad argument / NULL pointer */
    RT_ERR_IO = -2,       /* file missing or unreadable */
    RT_ERR_FORMAT = -3,   /* glTF / image content not supported (reference throws the same) */
    RT_ERR_DEVICE = -4,   /* HIP runtime error or no device */
    RT_ERR_LIMIT = -5,    /* scene exceeds a device limit (e.g. BVH deeper than the stack) */
    RT_ERR_STATE = -6     /* the scene is not in the state the call needs (posable meshes: no rest data, poses not enabled) */
};

typedef struct rt_scene rt_scene; /* opaque: host arrays + lazily uploaded device copies */

/* Read-only view of the flattened scene (the layout the kernels read from HBM).
 * Triangles and BVH nodes are in the reference's post-build order (bvh.cpp:166 reorders
 * `objects` in place), so object ids equal the reference's Intersection::object_id. */
typedef struct {
    int32_t width, height, samples, ray_depth; /* canvas, spp (scene_parser.cpp:16-22); a render
                                                  of a ray_depth outside 1..15 is RT_ERR_LIMIT,
                                                  before any launch                          */
    float max_distance;                        /* camera zfar or 1e9 (scene_parser.cpp:119) */
    float cam_pos[3];                          /* camera.h position_                        */
    float cam_axes[9];                         /* right, up, forward (camera.h axes_)       */
    float cam_fov[2];                          /* fov_x, fov_y radians                      */
    float tan_half_fov[2];                     /* tanf(fov/2) as camera.cpp:51-52 computes  */
    uint32_t n_tris;
    const float *tri;       /* n_tris x 12: v0.xyz, U.xyz, V.xyz, geometric normal.xyz       */
    const float *tri_attr;  /* n_tris x 16: normal[3].xyz, texcoord[3].xy, mesh_id (int bits) */
    const float *tri_tan;   /* n_tris x 12: tangent[3].xyzw                                   */
    uint32_t n_nodes;
    const float *node;      /* n_nodes x 8: aabb min.xyz, max.xyz, a, b (int bits):
                               internal: a = left child (right = left+1), b = split_dim
                               leaf:     a = first primitive, b = 3 | count << 2           */
    uint32_t bvh_depth;     /* max root-to-leaf depth (root = 0)                            */
    uint32_t n_lights;
    const float *light;     /* n_lights x 16: v0.xyz, U.xyz, V.xyz, geo normal.xyz, area, 0,0,0
                               (ManyLightsDistribution objects, light-BVH order)          */
    uint32_t n_light_nodes;
    const float *light_node; /* same format as node */
    uint32_t light_bvh_depth;
    uint32_t n_meshes;
    const float *mesh_f;     /* n_meshes x 12: base_color.xyz, emission.xyz, metallic,
                                roughness2, alpha, ior, 0, 0                               */
    const int32_t *mesh_tex; /* n_meshes x 4: base_color_i, normal_i, metallic_roughness_i,
                                emission_i (-1 = none)                                     */
    const double *mesh_normal_transform; /* n_meshes x 16 (column-major matrix4d)          */
    uint32_t n_textures;
    const uint32_t *tex_info; /* n_textures x 4: texel offset, width, height, channels     */
    const uint8_t *texels;    /* RGBA8, all textures concatenated                          */
    uint64_t n_texel_bytes;
} rt_scene_view;

typedef struct {
    int32_t spp;          /* samples per pixel (0 = the scene's)                         */
    int32_t rank, world;  /* pixel-row partition: rows whose (row / row_block) % world == rank */
    int32_t row_block;    /* rows per interleave block (default 8)                       */
    int32_t count;        /* 1 = accumulate ray / AABB / triangle test counters          */
    int32_t kernel;       /* RT_KERNEL_LANE (0, default) or RT_KERNEL_WAVEFRONT (4)      */
    int32_t flags;        /* RT_FLAG_* */
    int32_t fast_chunk;   /* RT_FLAG_FAST: samples per work unit (0 = 2; raised so a pixel
                             has at most 128 units)                                      */
    int32_t device;       /* HIP device to render on (rt_render uploads the scene there;
                             rt_render_device needs rt_scene_upload(scene, device) first) */
} rt_params;

/* rt_params.kernel: two schedules of the same per-pixel arithmetic (same bits) */
#define RT_KERNEL_LANE 0       /* lane-resident persistent kernel (rt_mega.h)            */
#define RT_KERNEL_WAVEFRONT 4  /* wavefront: init / extend / shade launches (rt_wavefront.h) */

/* rt_params.flags */
#define RT_FLAG_KERNEL_TIMES 1  /* wavefront path (kernel 4): time every extend / shade launch (HIP events) */
/* Fast mode (kernel 0 only): every (pixel, sample) draws from its own
 * stream (Philox4x32-10 keyed by pixel j*W+i, counter = sample, seeds the sample's minstd
 * stream; normal cache empty per sample), so a pixel's samples are independent work units
 * of fast_chunk samples that any lane may run.  The pixel sum is the chunk partials added in
 * chunk order: deterministic for a given (spp, fast_chunk), statistically equivalent to the
 * reference, NOT bit-identical to it (the parity mode is the default). */
#define RT_FLAG_FAST 2
/* Light-split kernel (kernel 0, parity mode): the light pdf's light-BVH
 * walk as its own traversal state between two shading passes.  Same bits; measured slower
 * on every scene tried, so off by default. */
#define RT_FLAG_LIGHT_SPLIT 4
/* Parity mode at spp >= 128 renders pixels heaviest-first: a counting pre-pass of 1 sample
 * per pixel (its own Philox streams), a box filter, a radix sort and a spread over the
 * waves, all inside the call and inside render_ms.  Below 128 spp it renders in row-major
 * order (the pre-pass would cost more than it gains).  NATURAL_ORDER always renders in
 * row-major order, HEAVY_ORDER always builds the heaviest-first order; same bits either way,
 * and the two flags exclude each other (RT_ERR_ARG). */
#define RT_FLAG_NATURAL_ORDER 8
#define RT_FLAG_HEAVY_ORDER 32
/* Parity mode, once the pixel queue is empty, runs the next samples of a wave's unfinished
 * pixels on its idle lanes before their start state is known, and adds only those whose
 * start state is proven equal to the sequential chain's (rt_mega.h, speculative sample
 * runahead): same bits, shorter frame tail.  A shard of at most two pixels per resident lane
 * runs on the runahead kernel throughout; a larger one runs on the plain kernel, which hands
 * its sparse tail waves' pixels to the runahead kernel at a sample boundary (the hand-off:
 * schedule = RT_SCHED_LANE | RT_SCHED_RUNAHEAD).  This flag turns both off.  (Counting
 * renders, count = 1, never use it: their counters are those of the sequential chain.) */
#define RT_FLAG_NO_RUNAHEAD 16
/* Every defined flag; a call with any other bit set fails with RT_ERR_ARG (e.g. ABI 5's
 * RT_FLAG_POOL = 64, removed in ABI 6). */
#define RT_FLAG_ALL (RT_FLAG_KERNEL_TIMES | RT_FLAG_FAST | RT_FLAG_LIGHT_SPLIT | RT_FLAG_NATURAL_ORDER | \
                     RT_FLAG_NO_RUNAHEAD | RT_FLAG_HEAVY_ORDER)

typedef struct {
    uint64_t pixels;        /* pixels rendered by this call                               */
    uint64_t samples;       /* pixels x spp                                               */
    uint64_t rays;          /* scene closest-hit queries (calls of BVH::intersect)         */
    uint64_t aabb_tests;    /* AABB::intersect calls inside those queries                 */
    uint64_t tri_tests;     /* Primitive::intersect calls inside those queries            */
    uint64_t light_queries; /* BVH::intersectAll calls (light pdf)                        */
    uint64_t light_aabb_tests;
    uint64_t light_tri_tests;
    uint64_t shading_hits;  /* scene hits that were shaded (texture / attribute fetches)  */
    double render_ms;       /* device time of the whole render (order pre-pass included), HIP events;
                               rt_render_frame / _multi: the slowest device (its shards summed) */
    /* RT_FLAG_KERNEL_TIMES (wavefront path): summed launch durations and launch counts   */
    double extend_ms, shade_ms;
    uint64_t extend_launches, shade_launches;
    uint64_t extend_rays;   /* rays traced by the extend launches (always filled)          */
    double order_ms;        /* part of render_ms spent building the pixel order            */
    double gather_ms;       /* rt_render_frame / _multi: device-to-device copies of the slowest
                               device + assembly on the root device + the copy to the host  */
    uint64_t devices;       /* devices that rendered                                       */
    uint64_t schedule;      /* RT_SCHED_* bits of the kernels that rendered (ABI 5; for
                               rt_render_frame / _multi the union over the shards)          */
} rt_stats;

/* rt_stats.schedule bits: which instantiation of the sample loop ran */
#define RT_SCHED_LANE 1         /* lane-resident kernel (rt_mega.h), no runahead            */
#define RT_SCHED_RUNAHEAD 2     /* lane-resident kernel with speculative sample runahead
                                   (both bits: the plain kernel's tail handed to it)        */
#define RT_SCHED_FAST 4         /* fast mode (RT_FLAG_FAST)                                 */
#define RT_SCHED_LIGHT_SPLIT 8  /* light-split kernel (RT_FLAG_LIGHT_SPLIT)                 */
#define RT_SCHED_WAVEFRONT 16   /* wavefront launches (RT_KERNEL_WAVEFRONT)                 */

/* --- scene ------------------------------------------------------------------------ */
int rt_scene_load_gltf(const char *path, int32_t width, int32_t height, int32_t samples, rt_scene **out);
/* Builds a scene from already-flattened arrays (same layout as rt_scene_view; copied).
 * This is the seam for a host that keeps its own loader: e.g. the reference's parsed and
 * BVH-built `Scene` (scene.h:14-38) flattened field by field. */
int rt_scene_from_view(const rt_scene_view *view, rt_scene **out);
int rt_scene_get_view(const rt_scene *scene, rt_scene_view *view);
void rt_scene_free(rt_scene *scene);

/* --- movable camera (additive in ABI 6) ---------------------------------------------------- */
/* The camera is not part of the scene's device image: the kernels take it by value with every
 * launch.  rt_scene_set_camera replaces the scene's camera on the host and in the launch
 * arguments of every device the scene is uploaded to; it uploads nothing and launches nothing, and
 * works on a scene that is on no device.  rt_scene_get_view reports the new values, cam_fov as
 * 2 * atanf(tan_half_fov) (nothing on the render path reads cam_fov: the kernels take the tangents).
 * A NULL argument, a non-finite word or a tangent that is not > 0: RT_ERR_ARG.  The call falls
 * under "one render per (scene, device) in flight": not while a render or a pass of the scene is.
 * After rt_scene_set_camera(C) every entry (rt_render*, rt_render_frame, rt_gbuffer*,
 * rt_intersect_rays, both kernels, fast mode, the counters) behaves bit for bit as on a scene built
 * by rt_scene_from_view from the same arrays with camera C.
 *
 * Accumulators: the scene counts its camera changes (the camera epoch), and an accumulator
 * remembers the epoch it was created, loaded or reset at.  On an accumulator whose epoch is not
 * the scene's (a stale one) the read-outs still work and give the old view's result:
 * rt_accum_sums, rt_accum_device_sums, rt_accum_counts*, rt_accum_moments,
 * rt_accum_device_moments, rt_accum_state, rt_accum_samples, rt_accum_sample_range (and
 * rt_accum_fast_chunk, rt_accum_has_moments).  Every other entry (one that renders, selects, marks,
 * reads the cached G-buffer or writes a file: a checkpoint's header holds the camera, and would
 * pair the old sums with the new one) fails with RT_ERR_ARG, a message that names rt_accum_reset,
 * and nothing launched.  rt_accum_reset returns the accumulator to the state rt_accum_create* left
 * it in (records, sums, moment buffers, samples done = 0), drops the marks, the pending selection
 * and the cached G-buffer and adopts the scene's epoch; kind, chunk size, partition, flags and
 * buffers are kept.  After it the accumulator is, bit for bit, a new one on the scene as it now
 * stands.  It works on an accumulator that is not stale too; it waits for the reset kernel. */
typedef struct { float pos[3]; float axes[9]; float tan_half_fov[2]; } rt_camera;  /* axes: right, up, forward, as rt_scene_view */
int rt_scene_get_camera(const rt_scene *scene, rt_camera *out);
int rt_scene_set_camera(rt_scene *scene, const rt_camera *cam);

/* --- movable geometry: triangle updates and a device-side BVH refit (additive in ABI 6) ------- */
/* New triangle records go into the scene in place and every node box is recomputed bottom-up; the
 * tree's topology and the primitive order are kept.  csrc/rt_refit.h is the rule's text, shared by
 * the host function, the device kernels and the CPU tests:
 *   select    smin(a, b) = b < a ? b : a, smax(a, b) = a < b ? b : a per component (std::min / std::max)
 *   start     every fold starts from the empty box (+FLT_MAX, -FLT_MAX)
 *   triangle  grow over v0, v0 + U, v0 + V in that order, each sum one f32 add per component
 *   leaf      grow over the boxes of its triangles first .. first + count - 1, in order
 *   internal  grow(left child's box), then grow(right child's box)
 * These are the boxes the reference's build gives the same ranges (Primitive::aabb primitive.cpp:63-75,
 * buildNode bvh.cpp:131-133): the bits of a bound are those of the first element in primitive order that
 * attains it (+0 and -0 keep their order), and a NaN component is never taken (an all-NaN triangle
 * gives the empty box, which changes nothing in its parent).
 *
 * rt_scene_update_tris replaces triangles [first, first + count) (post-build order, the ids
 * rt_intersect_rays reports).  tri: count x 12; tri_attr: count x 16 or NULL (kept); tri_tan: count x 12
 * or NULL (kept); records are taken as given (nothing normalised, non-finite words allowed).  The mesh
 * id word of tri_attr is ignored: a triangle never changes mesh.  Topology, primitive order, bvh_depth,
 * the light list and the light BVH are unchanged.  It updates the host arrays and refits the host
 * `node`, patches the cached device image (a later upload to another device is current), and on every
 * device the scene is uploaded to copies the range, scatters it into the arrays, runs the device
 * refit and waits: a device copy's boxes come from the device kernels, not from the host's.  It works
 * on a scene that is on no device.
 * rt_scene_update_tris_device: the same with the new records already on `device` (device pointers,
 * 16-byte aligned, not inside the scene's own arrays), the scatter and the refit enqueued on `stream`;
 * it then reads the changed range and the node array back into the host arrays and the cached image, and
 * waits.  The scene must be uploaded to `device` and to no other device.
 * Refusals, all before any launch or copy (nothing is left half made): NULL tri, a range beyond
 * n_tris, a triangle of the range that belongs to an emissive mesh (mesh_f emission not all zero;
 * moving lights are not supported: the light records and the light BVH are not remapped; a scene that
 * opted in with rt_scene_enable_light_updates, below, is not refused this), and for the
 * device entry a scene that is not on `device`, or also on another, or a misaligned pointer:
 * RT_ERR_ARG.  count == 0 is RT_OK and nothing happens.
 * Both fall under "one render per (scene, device) in flight", and so do rt_gbuffer*, rt_history_push and
 * the ray queries against an update: no update may run while any entry reads the scene's device copy.
 *
 * Contract: after an update every entry (rt_render*, rt_render_frame, both kernels, fast mode,
 * runahead, the counters, rt_gbuffer*, rt_intersect_rays*, rt_sample_frames_via, rt_device_selfcheck
 * 4 and 5) behaves bit for bit as on rt_scene_from_view(the same arrays, node = rt_refit_view(...)).
 * Accumulators: an update bumps the scene's epoch exactly as rt_scene_set_camera does, so the stale
 * rule and rt_accum_reset above apply unchanged.  A checkpoint's header holds no geometry: loading one
 * onto moved geometry is undetected, as it is for any other scene with equal counts.
 * rt_history: nothing changes in it; for a moved object its mesh, normal and plane tests accept or
 * reject as they stand.  A history that opted in with rt_history_enable_motion follows moved triangles
 * through per-pixel motion records ("per-pixel motion records" below).
 * A refit keeps the topology: after large moves the tree is still correct, but its quality (overlap
 * of sibling boxes) is whatever the moves left; there is no rebuild. */
int rt_scene_update_tris(rt_scene *scene, uint32_t first, uint32_t count,
                         const float *tri, const float *tri_attr, const float *tri_tan);
int rt_scene_update_tris_device(rt_scene *scene, int32_t device, uint32_t first, uint32_t count,
                                const float *d_tri, const float *d_tri_attr, const float *d_tri_tan, void *stream);
/* Pure host function: the refit boxes of a view's triangles and topology.
 * out_node: n_nodes x 8, with a and b copied. */
int rt_refit_view(const rt_scene_view *view, float *out_node);
/* Test / inspection entry: the device copy's arrays back in the host layout, nodes in build order.
 * Any pointer may be NULL. */
int rt_scene_read_device(rt_scene *scene, int32_t device, float *tri, float *tri_attr, float *tri_tan, float *node);

/* --- movable lights: emissive triangle updates, light list and light-BVH refit (additive in ABI 6) - */
/* Opt-in: until rt_scene_enable_light_updates succeeds on a scene, everything above holds as written,
 * the refusal of an emissive triangle included.  After it, rt_scene_update_tris* accept ranges that
 * hold triangles of emissive meshes and keep the light list (`light`, 16 words per light) and the light
 * BVH (`light_node`) in step; every other refusal stays.  csrc/rt_relight.h is the rule's text, shared
 * by the host functions, the device kernels and the CPU tests:
 *   record    words 0..11 of a light are its triangle's 12 words as given (the caller's geometric normal
 *             in words 9..11 included; nothing is normalised); word 12 is the area 0.5f * length(cross(U, V)),
 *             every operation one f32 rounding, no fused multiply-add:
 *               cross(a, b) = (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y)
 *               length(v)   = sqrt(((0 + v.x*v.x) + v.y*v.y) + v.z*v.z), correctly rounded sqrt
 *             words 13..15 are never written
 *   boxes     the rule above over the light records: v0, U, V are words 0..8 of a 16-word record, a light
 *             leaf folds lights first .. first + count - 1 in order, an internal node grow(left) then
 *             grow(right), every fold from the empty box, the same selects
 * These are the reference's light records and boxes for the same triangles in the same order
 * (Primitive::get_geometric_normal primitive.cpp:77-84; the light list and its BVH random.cpp:156-168).
 * The order of the lights and the light tree's topology are kept: a moved light keeps its index.
 *
 * The map.  Light k restates triangle tri_of_light[k]: the lights are walked in ascending index, and
 * light k takes the lowest-numbered triangle of an emissive mesh (mesh_f emission not all zero) that is
 * not yet taken and whose 12 words equal the light's words 0..11 bit for bit.  Both a loaded scene and
 * one from rt_scene_from_view follow this rule.  rt_scene_enable_light_updates builds the map and the
 * light tree's levels on the host (it works on a scene that is on no device, and is idempotent).  It
 * fails with RT_ERR_ARG, naming the first such light or triangle, if a light finds no triangle or an
 * emissive triangle is left without a light, or if the light tree is not what the refit relies on (leaf
 * ranges within n_lights, children above their parents); the scene then stays as it was, not opted in.
 * rt_scene_light_map copies tri_of_light (n_lights words); RT_ERR_ARG before the opt-in.
 *
 * Updates on an opted-in scene.  The host entry restates the light records of the range's light
 * triangles and every light box in the host arrays, patches the cached image, and on every device copy
 * launches, after the triangle scatter and the node refit, the light scatter (one thread per triangle of
 * the range) and one launch per level of the light tree, deepest first; the kernel boundary is the only
 * ordering.  The device entry does the same on `stream` and reads the light array and the light node
 * array back into the host arrays and the image before it returns.  A range that holds no light triangle
 * launches none of the light kernels and reads no light data back.  A device copy's first update after
 * the opt-in puts the map and the level lists into a small allocation of that copy.
 *
 * Contract: after an update on an opted-in scene every entry named in the contract above behaves bit for
 * bit as on rt_scene_from_view(the same arrays, node = rt_refit_view(...), light and light_node =
 * rt_relight_view(...)).  One exception: where a light's area is NaN, host and device may store different
 * NaN bit patterns (an invalid operation yields different default NaNs on the two); nothing is
 * canonicalised.  The epoch rule is unchanged: an update bumps the scene's epoch.
 * Limits: topology kept, no rebuild, and the light order kept (the reference picks a light uniformly by
 * index; a fresh build of the moved scene might order the lights differently). */
int rt_scene_enable_light_updates(rt_scene *scene);
int rt_scene_light_map(const rt_scene *scene, uint32_t *tri_of_light);
/* Pure host function, the twin of rt_refit_view: out_light (n_lights x 16) is the view's `light` with words
 * 0..12 of every light restated from triangle tri_of_light[k] (words 13..15 copied); out_light_node
 * (n_light_nodes x 8) is the view's `light_node` with every box recomputed by the sweep, a and b copied. */
int rt_relight_view(const rt_scene_view *view, const uint32_t *tri_of_light, float *out_light, float *out_light_node);
/* Test / inspection entry: the device copy's light and light_node arrays (the host layout).  Either
 * pointer may be NULL. */
int rt_scene_read_device_lights(rt_scene *scene, int32_t device, float *light, float *light_node);

/* --- posable meshes: per-mesh node matrices, applied on the device (additive in ABI 6) ------------- */
/* A mesh posed with matrix M holds, triangle for triangle, the records the loader makes of the same glTF
 * whose node carries M — and the loader's are the reference's (tests/test_loader.py).  csrc/rt_pose.h is
 * the rule's text, shared by the loader's triangle loop, the host functions, the device kernel and the
 * CPU tests.  M is a matrix4<double> in column storage: element (row i, column j) is m[4 * j + i].
 *   positions  v0 = M q0, U = M q1 - v0, V.x = (M q2).x - v0.x with M q the reference's multiply (float
 *              accumulators, every add in double and rounded to float); V.y, V.z are differences of the
 *              once-rounded dots of q2 and q0 (the shipped binary's loop)
 *   normals    normal(NT n), x and y rounded once, z per add; NT = inverse(transpose(M)), the cofactor
 *              inverse, computed on the host once per posed mesh
 *   tri 9..11  normal(cross(U, V)); a light's area follows as in the movable-lights rule above
 * tri_attr words 9..15 and tri_tan do not depend on M and are never written: tangents stay in object
 * space and shading carries them with the mesh's mesh_normal_transform, which therefore follows the pose
 * in the host arrays, in the cached image and on every device copy.
 *
 * Rest data.  rt_scene_load_gltf keeps, per triangle in post-build order, the rest record (18 floats: the
 * object-space positions q0 q1 q2 and normals n0 n1 n2; (0,0,1) where the primitive has no NORMAL) and
 * tri_source, the triangle's index in load order (node, primitive, triangle), and per mesh the loaded node
 * matrix.  A scene from rt_scene_from_view holds none until rt_scene_set_rest hands the same three arrays
 * in (tri_source must be a permutation; RT_ERR_STATE once poses are enabled).  rt_scene_get_rest copies
 * them out (any pointer may be NULL) and rt_scene_tri_source copies tri_source alone; RT_ERR_STATE where
 * the scene holds none.
 *
 * rt_scene_enable_poses: idempotent; RT_ERR_STATE without rest data, the scene untouched.  It puts the rest
 * records (padded to five 16-byte quads each) on every device the scene is on; a device it is uploaded to
 * later takes them then.  rt_scene_get_mesh_transform: the mesh's current matrix (the loaded one until it
 * is posed).
 *
 * rt_scene_pose_meshes gives each of the n named meshes its whole node matrix (16 doubles each; not an
 * offset from the loaded one).  The host twin restates the meshes' records, every node box (the refit
 * rule above), and, where an emissive mesh is posed, the light records of the covering range and every
 * light box; it patches the cached image.  On every device copy a table goes up (per posed mesh M and NT,
 * and a slot per mesh), the posed meshes' mesh_normal_transform is rewritten, one kernel recomputes the
 * records of the covering range's posed triangles from the copy's own rest records (one thread per
 * triangle; tri as three 16-byte stores and words 0..8 of tri_attr), and the refit launches and, for an
 * emissive mesh, the light launches follow; the call waits.  No record crosses the bus.
 * Refusals, all before any launch or copy, the scene left exactly as it was: poses not enabled
 * (RT_ERR_STATE); n == 0 or a NULL pointer, a mesh id beyond n_meshes, a mesh named twice, a matrix whose
 * determinant (as the cofactor inverse computes it) is zero, an emissive mesh on a scene without
 * rt_scene_enable_light_updates (RT_ERR_ARG).  A matrix with a NaN or infinite entry and a non-zero
 * determinant is not refused: the records are whatever the rule gives and the boxes follow the refit rule
 * (a NaN component is never taken); where a word is NaN, host and device may hold different NaN bits.
 * Contract: as for rt_scene_update_tris — every entry then behaves as on rt_scene_from_view(the same
 * arrays).  The call bumps the scene's epochs as an update does: accumulators go stale, and a history with
 * motion records follows the posed triangles.
 * Limits: topology kept (a rotation degrades the tree more than a translation does; no rebuild); one level
 * (a pose is the mesh's world matrix, there is no node hierarchy); checkpoints hold no pose.
 *
 * rt_pose_view: pure host function, the twin of rt_refit_view: out_tri (n_tris x 12), out_tri_attr
 * (n_tris x 16) and out_mesh_nt (n_meshes x 16) are the view's with the named meshes posed; rest is
 * n_tris x 18.  The refusals that need no scene apply (RT_ERR_ARG).
 * rt_trs_matrix: matrix4::TRS as the loader computes a node's (float arithmetic, stored to double);
 * r is the quaternion x y z w. */
int rt_scene_set_rest(rt_scene *scene, const float *rest, const uint32_t *tri_source, const double *mesh_matrix);
int rt_scene_get_rest(const rt_scene *scene, float *rest, uint32_t *tri_source, double *mesh_matrix);
int rt_scene_tri_source(const rt_scene *scene, uint32_t *out);
int rt_scene_enable_poses(rt_scene *scene);
int rt_scene_get_mesh_transform(const rt_scene *scene, uint32_t mesh, double m[16]);
int rt_scene_pose_meshes(rt_scene *scene, uint32_t n, const uint32_t *mesh, const double *m);
int rt_pose_view(const rt_scene_view *view, const float *rest, uint32_t n, const uint32_t *mesh, const double *m,
                 float *out_tri, float *out_tri_attr, double *out_mesh_nt);
int rt_trs_matrix(const float t[3], const float r[4], const float s[3], double out[16]);

/* --- render ----------------------------------------------------------------------- */
/* Copies the scene to `device` (once per device; later calls reuse it).  One render per
 * (scene, device) may be in flight at a time; different devices render independently. */
int rt_scene_upload(rt_scene *scene, int32_t device);
/* Number of pixels a (rank, world, row_block) shard owns, and their row-major order:
 * rows_out (may be NULL) receives the owned row indices, ascending. */
int64_t rt_shard_rows(int32_t height, int32_t rank, int32_t world, int32_t row_block, int32_t *rows_out);
/* Renders the shard into host memory: out_sum[k*W*3 + i*3 + c] for the k-th owned row. */
int rt_render(rt_scene *scene, const rt_params *params, float *out_sum, rt_stats *stats);
/* Same into device memory (d_out_sum on the scene's device, same layout) on HIP stream
 * `stream` (NULL = default stream); returns after the launch (asynchronous) unless
 * stats != NULL, in which case it waits and fills the counters and kernel time. */
int rt_render_device(rt_scene *scene, const rt_params *params, float *d_out_sum, void *stream, rt_stats *stats);
/* The whole frame on devices 0 .. n_devices-1 (n_devices <= 0: every visible device), one
 * host thread per device, device d rendering the shard (rank d, world n_devices,
 * params->row_block); params->rank / world / device are ignored.  out_sum: W*H*3 floats,
 * host memory, row-major.  Bits do not depend on n_devices. */
int rt_render_multi(rt_scene *scene, const rt_params *params, int32_t n_devices, float *out_sum, rt_stats *stats);
/* The whole frame as shards 0 .. n_shards-1 of a (world = n_shards, params->row_block) split,
 * shard r rendered on device devices[r] (devices NULL: device r; a device given several shards
 * renders them one after another).  Each shard is rendered and finished to 8 bits on its own
 * device (scene.cpp:54-64), then copied device-to-device (hipMemcpyPeerAsync, xGMI between
 * MI355X) to devices[0], which places the rows in frame order; the frame leaves the devices
 * in one copy per output.  out_rgb: W*H*3 bytes, the reference's canvas (canvas.h:76-89);
 * out_sum: W*H*3 floats (sample_canvas, scene.cpp:20,42); either may be NULL, not both.
 * params->rank / world / device are ignored.  Bits do not depend on n_shards or devices. */
int rt_render_frame(rt_scene *scene, const rt_params *params, int32_t n_shards, const int32_t *devices,
                    uint8_t *out_rgb, float *out_sum, rt_stats *stats);

/* --- progressive rendering (additive in ABI 6) ---------------------------------------- */
/* An accumulator owns the per-pixel chain state of one shard on one device (per pixel: next
 * sample, minstd_rand state, polar-normal cache, running float sum) and renders further
 * samples in passes of any size.  After passes of n1, n2, ..., nk samples its sums are
 * bit-identical to rt_render at spp = n1 + ... + nk, for every split and every schedule flag:
 * a pixel's samples still run in order from the carried state and add in order to the carried
 * sum.  This is the seam for the reference's Scene::render(ProgressFunc): previews, progress,
 * early stop, more samples on a finished frame, checkpoint and resume.
 *
 * (Fast mode has accumulators of its own kind, with their own invariant: rt_accum_create_fast
 * below.)  Parity mode on the lane-resident kernel only: RT_FLAG_NATURAL_ORDER, RT_FLAG_HEAVY_ORDER and
 * RT_FLAG_NO_RUNAHEAD are honoured; RT_FLAG_FAST, RT_FLAG_LIGHT_SPLIT, RT_FLAG_KERNEL_TIMES,
 * count != 0 and kernel != RT_KERNEL_LANE fail with RT_ERR_ARG.  The pixel order is chosen per
 * pass by rt_render's rule on the pass's own sample count (pre-pass at >= 128 samples or with
 * HEAVY_ORDER); bits never depend on it.
 *
 * A pass uses the device scene's workspace: the rule "one render per (scene, device) in
 * flight" covers accumulator passes too (passes of two accumulators of one scene on one
 * device, or a pass and an rt_render_device, must not overlap).  Free an accumulator before
 * its scene. */
typedef struct rt_accum rt_accum;
/* Uses rank, world, row_block, device and flags of params (spp is ignored); the scene must be
 * uploaded to that device (rt_scene_upload).  No samples yet: sums are 0. */
int rt_accum_create(rt_scene *scene, const rt_params *params, rt_accum **out);
/* Renders samples [done, done + n_samples) of every owned pixel on HIP stream `stream`;
 * asynchronous unless stats != NULL, like rt_render_device (stats->samples = pixels x
 * n_samples; schedule, render_ms, order_ms as there).  n_samples < 1: RT_ERR_ARG; a total of
 * 2^20 or more: RT_ERR_LIMIT (nothing is launched). */
int rt_accum_add(rt_accum *accum, int32_t n_samples, void *stream, rt_stats *stats);
int32_t rt_accum_samples(const rt_accum *accum); /* samples done */
/* The sums so far in host memory, in rt_render's shard layout (waits for the last pass). */
int rt_accum_sums(rt_accum *accum, float *out_sum);
/* The same sums on the device: valid until rt_accum_free, written by every pass. */
const float *rt_accum_device_sums(rt_accum *accum);
/* The shard finished to 8 bits at spp = samples done (rt_tonemap_u8_device): rows x W x 3. */
int rt_accum_frame_u8(rt_accum *accum, uint8_t *out_rgb);
/* Test / inspection entry: n_pixels x 4 words per pixel: next sample, engine state, cache
 * flag, cached value bits. */
int rt_accum_state(rt_accum *accum, uint32_t *out);
/* Checkpoint: a 128-byte header (magic "RTACCUM\0", u32 version 1; i32 width, height,
 * ray_depth, rank, world, row_block; u32 n_tris, n_nodes, n_lights; i64 n_pixels; i32 samples
 * done, i32 0; 14 floats cam_pos, cam_axes, tan_half_fov; 8 bytes 0), then n_pixels records of
 * 8 words (pixel, next sample, engine state | cache flag << 31, cached value, sum x, y, z, 0).
 * rt_accum_load checks the file before any device call: missing RT_ERR_IO; bad magic, version
 * or length RT_ERR_FORMAT; a header that does not fit the scene RT_ERR_ARG.  It then uploads
 * the scene to `device` if need be; the loaded accumulator (rank, world and row_block of the
 * file, default schedule flags) continues bit-identically. */
int rt_accum_save(rt_accum *accum, const char *path);
int rt_accum_load(rt_scene *scene, int32_t device, const char *path, rt_accum **out);
void rt_accum_free(rt_accum *accum);
/* Back to the state after rt_accum_create*, on the scene's camera as it now stands ("movable
 * camera" above); on `stream`, and it waits. */
int rt_accum_reset(rt_accum *accum, void *stream);

/* --- per-pixel sample counts: subset passes and adaptive refinement (additive in ABI 6) --- */
/* Every pixel's record carries its own next sample, so a pass may render a subset of the shard:
 * a window, a mask, the pixels below a sample count, the pixels an error estimate still calls
 * noisy.  The invariant carries over: after any sequence of full and subset passes, a pixel that
 * has n samples holds exactly the sum rt_render gives that pixel at spp = n.
 *
 * The subset is chosen on the device (rt_accum_select) and rendered by the next
 * rt_accum_add_selected; a caller never hands in a pixel list.  (Liveness: a listed pixel whose
 * record is at or past the pass's end sample would never finish, and a pixel listed twice would
 * be raced by two lanes.  The selection's rule includes next < target and emits every pixel at
 * most once.)  A pending selection is dropped by every pass (rt_accum_add,
 * rt_accum_add_selected), which change the records it was made from; a new or loaded
 * accumulator has none.  rt_accum_mark changes no record and leaves it pending, so the
 * adaptive loop is select, mark, add_selected.
 *
 * The rule, per owned pixel (csrc/rt_select.h is its text, shared by the device and the CPU
 * test; f32 arithmetic in the order written).  n_b = the pixel's sample count, S_b = its sum;
 * n_a, S_a = both at the last rt_accum_mark (n_a = 0 without one):
 *   1. outside the window, mask byte 0, or n_b >= target                   -> not selected
 *   2. threshold <= 0                                                      -> selected
 *   3. n_b == 0 or n_a == 0 (no estimate yet)                              -> selected
 *      n_b == n_a (no sample since it was last judged: convergence sticks) -> not selected
 *   4. per channel ma = S_a / n_a, mn = (S_b - S_a) / (n_b - n_a), mb = S_b / n_b (each as a
 *      product with the f32 reciprocal of the count), d = |mn - ma|;
 *      e = ((d_r + d_g) + d_b) / sqrtf(((mb_r + mb_g) + mb_b) + 1e-4f); selected iff
 *      e > threshold.  A NaN e (non-finite sums) is never selected.
 * The estimate compares the mean of the samples before the mark with the mean of those since
 * (normalised like the half-buffer criterion of Dammertz et al.); it is a first estimator: the
 * 1e-4 floor and the per-pixel form without a spatial filter are choices, not measurements. */
typedef struct {
    int32_t target;           /* absolute sample count the selected pixels are raised to */
    int32_t x0, y0, x1, y1;   /* frame window [x0, x1) x [y0, y1), all 0 = whole frame */
    const uint8_t *mask;      /* host, n_pixels bytes in the shard's layout, NULL = all */
    float threshold;          /* <= 0: no error test */
} rt_select;
/* Copies the sums and counts as they stand into the accumulator's mark buffers (3 floats and one
 * int per pixel, made on first use); asynchronous on `stream`.  Marks are not part of a
 * checkpoint: a loaded accumulator has no mark. */
int rt_accum_mark(rt_accum *accum, void *stream);
/* Applies the rule and keeps the selected pixels as the pending list, in ascending shard-pixel
 * order (deterministic: no atomics order it); waits, and returns the list's length in
 * *n_selected (may be NULL).  Checked before any launch: target < 1 RT_ERR_ARG; target >= 2^20
 * RT_ERR_LIMIT; a window with x1 < x0, y1 < y0 or outside the frame RT_ERR_ARG. */
int rt_accum_select(rt_accum *accum, const rt_select *select, void *stream, int64_t *n_selected);
/* Test / inspection entry: the pending list (n_selected shard pixels). */
int rt_accum_selection(rt_accum *accum, int32_t *out_pixels);
/* Renders every listed pixel from its own next sample up to the selection's target, on the
 * schedule rt_accum_add's rule gives for that many items (a small list runs on the runahead
 * kernel throughout, a large one on the plain kernel with the hand-off); the list is the pixel
 * order, so no order pre-pass runs and RT_FLAG_HEAVY_ORDER is ignored.  Asynchronous unless
 * stats != NULL (stats->pixels = the list's length, samples = the sum of target - next over it,
 * order_ms = 0).  Without a pending selection RT_ERR_ARG; an empty selection launches nothing
 * (RT_OK, stats zero).  Pixels not listed keep their sums and records. */
int rt_accum_add_selected(rt_accum *accum, void *stream, rt_stats *stats);
/* The sample-count map: every owned pixel's count, to host memory (waits) or to device memory
 * on `stream` (asynchronous). */
int rt_accum_counts(rt_accum *accum, int32_t *out);
int rt_accum_counts_device(rt_accum *accum, int32_t *d_out, void *stream);
/* The smallest and the largest count (either pointer may be NULL). */
int rt_accum_sample_range(rt_accum *accum, int32_t *min_out, int32_t *max_out);
/* While the counts differ: rt_accum_samples returns the largest; rt_accum_add fails with
 * RT_ERR_ARG (level first: select with target = the largest count and no threshold, then
 * rt_accum_add_selected); rt_accum_frame_u8 divides every pixel by its own count
 * (rt_tonemap_u8_counts_device); rt_accum_save writes header word `i32 0` as 1 and `samples done`
 * as the largest count, and rt_accum_load then accepts any record whose next sample is at most
 * that (with 0 there, every record must equal it, as before).  The rule "one render per (scene,
 * device) in flight" covers rt_accum_mark, rt_accum_select and rt_accum_add_selected. */

/* --- fast-mode accumulators: progressive and adaptive passes on Philox units (additive in ABI 6) --- */
/* A fast accumulator is an rt_accum whose passes render fast-mode work units (RT_FLAG_FAST): sample
 * s of a pixel draws from its own Philox stream keyed by (pixel, s), so its record needs no RNG
 * state and a pixel's samples have no chain: a subset pass is as parallel as a full one.  A one-shot
 * fast sum is defined by where its chunk boundaries fall, and rt_render moves them with spp; here
 * they never move.  The accumulator has a chunk size c >= 1, fixed at creation from
 * params->fast_chunk (0 = 2) and never raised: chunk j of a pixel is its samples [j c, (j + 1) c).
 *
 * Invariant: after any sequence of full and subset passes of any sizes, a pixel that has n samples
 * holds, bit for bit, the fast sum of n samples in chunks of c: the partials of chunks 0, 1, ...
 * (each the sum of its samples in sample order, from +0.f) added in chunk order from +0.f, the
 * last one ragged when c does not divide n (the CPU oracle's rt_oracle_render_fast(spp = n,
 * chunk = c)).  For n <= 128 c that is also rt_render with RT_FLAG_FAST at spp = n, fast_chunk = c.
 *
 * Per pixel the 32-byte record holds (pixel, next sample, total x, y, z, open x, y, z):
 *   total  the fold, from +0.f, of the partials of all complete chunks, in chunk order;
 *   open   the running partial of the chunk that contains `next` when next % c != 0, zero words
 *          otherwise;
 * and the reported sum (rt_accum_sums, rt_accum_device_sums, what rt_accum_mark copies and the
 * selection rule and the frame finish read) is total when next % c == 0, else total + open (always
 * added; open is never reported alone).  So a pass may stop and resume anywhere, in or between
 * chunks.  csrc/rt_fast_units.h is the text of the unit arithmetic and the fold, shared by the
 * device and the CPU test.
 *
 * Every rt_accum_* entry works on a fast accumulator as on a parity one, with these differences:
 *   rt_accum_add / rt_accum_add_selected  any n >= 1 and any target, multiples of c or not; stats
 *       schedule = RT_SCHED_FAST, order_ms = 0, pixels and samples as for parity passes.  A launch
 *       carries at most 128 units per item; a pass that needs more runs as successive complete
 *       passes to chunk boundaries on the way (same bits).  Items are never ordered.
 *   rt_accum_state   n_pixels x 4 words: next sample, then the three words of `open`.
 *   rt_accum_save    magic "RTFACCUM", u32 version 1, the same 128-byte header with c (i32) in the
 *       first four of its eight trailing bytes, then the records verbatim.  Marks are not saved.
 *   rt_accum_load    reads both kinds (the magic says which) and returns that kind; for a fast
 *       file, besides the parity checks (the record / samples-done rule included): c < 1 and
 *       non-zero `open` words where next % c == 0 are RT_ERR_FORMAT.  All before any device call.
 * rt_accum_create_fast uses rank, world, row_block, device and fast_chunk of params; the scene must
 * be uploaded to that device.  RT_FLAG_FAST may be set or not; RT_FLAG_NATURAL_ORDER,
 * RT_FLAG_HEAVY_ORDER and RT_FLAG_NO_RUNAHEAD are accepted and ignored.  count != 0, a kernel other
 * than RT_KERNEL_LANE, RT_FLAG_LIGHT_SPLIT, RT_FLAG_KERNEL_TIMES and fast_chunk < 0 fail with
 * RT_ERR_ARG.  (rt_accum_create goes on refusing RT_FLAG_FAST: its accumulators are parity ones.) */
int rt_accum_create_fast(rt_scene *scene, const rt_params *params, rt_accum **out);
/* The accumulator's chunk size c; 0 for a parity accumulator (or NULL). */
int32_t rt_accum_fast_chunk(const rt_accum *accum);

/* Closest hit + light pdf for n explicit rays (BVH::intersect bvh.cpp:239-243 and
 * ManyLightsDistribution::pdf random.cpp:179-188; origin/dir as given to Ray::Ray, which
 * normalises dir).  Host arrays: org/dir n x 3; out_f n x 4 (t, u, v, light_pdf);
 * out_i n x 6 (hit, object id or -1, AABB tests, triangle tests, light AABB tests,
 * light triangle tests). */
int rt_intersect_rays(rt_scene *scene, int64_t n, const float *org, const float *dir, float *out_f, int64_t *out_i);
/* The same query and output layout through one of the device's traversals (test entry; ray i is
 * thread i, so the caller decides which rays share a wave):
 *   path 0  closest_hit and light_pdf (rt_path.h): rt_intersect_rays is this call;
 *   path 1  the per-lane steps: trav_step over a private stack with the runahead kernel's cull
 *           form, then light_step;
 *   path 2  the cooperative step trav_step_coop with the plain kernel's constants and four stack
 *           frames in LDS ((u, v) recomputed afterwards, as its shading pass does), then light_step.
 * The loops of paths 1 and 2 are bounded by the scene's size; a ray still traversing at the
 * bound is reported with hit = -2.  Any other path is RT_ERR_ARG. */
int rt_intersect_rays_via(rt_scene *scene, int32_t path, int64_t n, const float *org, const float *dir, float *out_f,
                          int64_t *out_i);
/* Sampler-level query (test entry): SceneDistribution::sample, then ::pdf of the drawn direction, for
 * explicit shading frames.  Host arrays: frame n x 10 (point, normal, eye direction, roughness2; taken
 * as given, nothing is normalised), seed n (the engine's seed, 1 .. 2147483646), warm n (0, or 1: one
 * polar normal is drawn first, so the normal cache is full where the sampler starts).  Frame i is thread
 * i and starts from Engine(seed[i]) with an empty normal cache.  out_f n x 6 (direction, pdf, the light
 * distribution's pdf alone, the next polar normal), out_i n x 4 (status, the next engine output, light
 * AABB tests, light triangle tests).
 *   path 0  scene_sample, then scene_pdf over a private stack (rt_path.h), as the per-pixel and
 *           wavefront kernels compose them;
 *   path 1  scene_sample, the light_step walk (bounded by the light list's size), scene_pdf_lp, as the
 *           lane-resident kernels compose them.
 * Status 0: complete; -2: the light walk reached its bound.  A NULL argument, another path, a seed
 * outside its range or a warm flag above 1: RT_ERR_ARG, before any device work. */
int rt_sample_frames_via(rt_scene *scene, int32_t path, int64_t n, const float *frame, const uint32_t *seed,
                         const uint32_t *warm, float *out_f, int64_t *out_i);

/* --- frame finish / output (host) ---------------------------------------------------- */
/* mean -> ACES -> powf(1/2.2) -> roundf(clamp(v*255)) per scene.cpp:54-64, vector.h:222-233, :400-407 */
int rt_tonemap_u8(const float *sum, int32_t width, int32_t height, int32_t spp, uint8_t *rgb_out);
/* The same finish on the device (current HIP device, asynchronous on `stream`): d_sum and
 * d_rgb are device pointers; bit-identical to rt_tonemap_u8 (the gamma quantizer is glibc
 * powf's, as exact thresholds). */
int rt_tonemap_u8_device(const float *d_sum, int32_t width, int32_t height, int32_t spp, uint8_t *d_rgb, void *stream);
/* The finish of a frame whose pixels hold different sample counts (subset passes): pixel p's sum
 * is multiplied by 1.f / (float)counts[p] where rt_tonemap_u8 multiplies by 1.f / (float)spp,
 * then the same ACES, gamma and quantizer (same NaN / inf behaviour); a pixel with 0 samples
 * gives 0, 0, 0.  With every count equal to spp the bytes are rt_tonemap_u8's.  The device
 * twin runs on the current HIP device, asynchronous on `stream`, bit-identical to the host's. */
int rt_tonemap_u8_counts(const float *sum, const int32_t *counts, int32_t width, int32_t height, uint8_t *rgb_out);
int rt_tonemap_u8_counts_device(const float *d_sum, const int32_t *d_counts, int32_t width, int32_t height, uint8_t *d_rgb,
                                void *stream);
/* "P6\n{W} {H}\n255\n" + raw RGB (canvas.h:76-89) */
int rt_write_ppm(const char *path, const uint8_t *rgb, int32_t width, int32_t height);

/* --- first-hit feature buffer and frame denoiser (additive in ABI 6) ------------------- */
/* The first-hit feature buffer (G-buffer).  Every owned pixel gets one record from the ray through
 * its centre, Camera::cast_in_pixel with zero offsets (camera.cpp:49-62): no random number is
 * drawn, so the record depends on neither spp nor an accumulator.  A record is RT_GBUFFER_WORDS
 * 32-bit words (64 B), four groups of four:
 *   words  0..3   shading normal N.xyz, hit distance t
 *   words  4..7   base colour (albedo).xyz, triangle id (int32 bits)
 *   words  8..11  emission.xyz, mesh id (int32 bits)
 *   words 12..15  hit position P = o + d * t (each component one multiply, one add, f32), 0
 * A hit is the scene's closest hit with t < max_distance (the sample loop's own test); a miss is
 * all-zero words with both ids -1.  N is Primitive::get_shading_normal (primitive.cpp:86-105:
 * interpolated vertex normals, the normal map, negated where the ray is inside), before the
 * sample loop's fall-back to the geometric normal; albedo is the mesh's base colour factor times
 * the sRGB base-colour texture sample where the mesh has one; emission is Primitive::get_emission
 * (primitive.cpp:121-129).  csrc/rt_gbuffer.h is the text, shared by the device kernel and the CPU
 * test; the render kernels are not touched by it.
 *
 * Both entries use rank, world, row_block and device of params (the other fields are ignored) and
 * write the records in rt_render's shard layout: record k * W + i for column i of the k-th owned
 * row.  rt_gbuffer writes host memory and uploads the scene to the device if need be;
 * rt_gbuffer_device writes device memory on `stream`, asynchronously, and needs the scene on the
 * device (rt_scene_upload).  A NULL argument, a bad partition and (rt_gbuffer_device) a scene that
 * is not on the device are RT_ERR_ARG; no such device or a HIP error RT_ERR_DEVICE.
 * Both only read the device copy of the scene and use none of its workspace, so they do not fall
 * under "one render per (scene, device) in flight": they may run beside a render or a pass of the
 * same scene on the same device (rt_gbuffer works on the default stream and waits for its copy); but
 * not beside rt_scene_update_tris*, which writes what they read. */
#define RT_GBUFFER_WORDS 16
int rt_gbuffer(rt_scene *scene, const rt_params *params, float *out);
int rt_gbuffer_device(rt_scene *scene, const rt_params *params, float *d_out, void *stream);

/* The denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a WHOLE frame
 * on one device, guided by the frame's G-buffer (five levels reach 62 pixels, so it cannot run per
 * row-block shard).  A pure function of its inputs.  csrc/rt_denoise.h is its text, shared by the
 * device kernels and the host function.  Only f32 +, -, *, /, comparisons and selects in the order
 * written below; the falloffs are rational, so the host function, the device kernels and a
 * restatement in any IEEE f32 arithmetic without contraction give the same bits.
 *
 * Parameters.  A NULL params is all defaults.  iterations: 0 is a value (no filtering), a negative
 * one takes the default 5, more than 6 is RT_ERR_ARG.  sigma_color, sigma_plane: <= 0 takes the
 * default (2 and 0.02); NaN or infinite is RT_ERR_ARG.  normal_power_log2: <= 0 takes the default
 * 6, more than 16 is RT_ERR_ARG.  The 5 levels and the exponent 2^6 are the filter's usual
 * choices; the two sigmas are picked, not tuned: no measurement stands behind them.
 *
 * Inputs: sums (W * H * 3 floats, row-major), then either counts (W * H sample counts) or, with
 * counts NULL, one spp >= 1 for every pixel; the G-buffer (W * H records).  Output: the W * H * 3
 * float MEAN frame; rt_tonemap_u8 with spp = 1 turns it into bytes (1.f / 1.f is exact).
 *
 * Prepare, per pixel with n samples (a negative count is 0), sums S, record (N, t, albedo, E, P):
 *   m  = S * (n > 0 ? 1.f / (float)n : 0.f)                       per channel, as the finish does
 *   a' = albedo > 1e-3f ? albedo : 1e-3f                          per channel
 *   L  = (m - E) / a'                                             per channel
 *   kind: pass   a miss (triangle id < 0), or a hit with n > 0 whose m or L has a non-finite channel
 *         fill   a hit with n <= 0
 *         valid  every other hit; only a valid pixel keeps its L (the others hold 0, 0, 0)
 * One level k = 0 .. iterations - 1, stride s = 2^k, reading one buffer of (L, kind) and writing
 * the other (all pixels read level k's input).  For a centre p of kind pass: copied.  Otherwise,
 * over the 25 taps q = p + (dx * s, dy * s), dy = -2 .. 2 outer, dx = -2 .. 2 inner, skipping a tap
 * outside the frame or not of kind valid:
 *   h  = b(dx) * b(dy),  b(0) = 3/8, b(+-1) = 1/4, b(+-2) = 1/16
 *   nd = (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z;  nd = nd > 0 ? nd : 0;  nd = nd * nd,
 *        normal_power_log2 times
 *   e  = Pq - Pp;  pd = (Np.x * e.x + Np.y * e.y) + Np.z * e.z;  pr = pd / (sigma_plane * tp);
 *   wp = 1 / (1 + pr * pr)
 *   wc = 1 for a centre of kind fill, else with d = Lq - Lp:
 *        1 / (1 + ((d.x * d.x + d.y * d.y) + d.z * d.z) / c_k),  c_k = (sigma_color * 2^-k)^2
 *   w  = ((h * nd) * wp) * wc;  a tap whose w is not > 0 (zero or NaN) is skipped
 *   sw = sw + w;  sL = sL + w * Lq                                per channel, all from +0
 * and the centre becomes (sL / sw, valid) when sw > 0 and the three quotients are finite (so a
 * filled pixel contributes from the next level on), (0, 0, 0, its kind) when sw is not > 0, and
 * stays as it was when a quotient overflowed.
 * Resolve: a pixel of kind pass gives its own m; every other gives L' * a' + E per channel (a fill
 * pixel no level could fill has L' = 0).  With iterations = 0 every pixel gives m, bit for bit.
 *
 * So: a hit without samples is filled from its neighbours; a miss keeps its mean; a hit with a NaN
 * or infinite mean keeps it, so the finish treats it as before, and it never reaches another
 * pixel; across perpendicular faces nd is exactly 0.
 *
 * rt_denoise runs on the host.  rt_denoise_device runs on the current HIP device, asynchronously
 * on `stream`, every pointer but params a device pointer; its bits are rt_denoise's.  Its scratch
 * (64 B per pixel) is kept per device from the first call on and only grows, so one
 * rt_denoise_device per device may be in flight.  NULL sums, G-buffer or output, a width or height
 * < 1, counts NULL with spp < 1 and the parameter refusals above are RT_ERR_ARG; a frame of 2^31
 * pixels or more RT_ERR_LIMIT; a HIP error or no device RT_ERR_DEVICE. */
typedef struct {
    int32_t iterations;          /* 0..6; < 0: 5                      */
    float sigma_color;           /* <= 0: 2 (demodulated radiance, at level 0) */
    float sigma_plane;           /* <= 0: 0.02 (fraction of the centre's hit distance) */
    int32_t normal_power_log2;   /* 1..16; <= 0: 6                    */
} rt_denoise_params;
int rt_denoise(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
               const float *gbuffer, const rt_denoise_params *params, float *out_mean);
int rt_denoise_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                      const float *d_gbuffer, const rt_denoise_params *params, float *d_out_mean, void *stream);
/* The same filter and the 8-bit finish for a caller that holds host arrays and no HIP (the CLI's
 * several-GPU frames): sums, counts (or NULL and spp) and G-buffer are copied to `device`, denoised
 * there (rt_denoise_device), finished at spp = 1 (rt_tonemap_u8_device) and the W * H * 3 bytes
 * copied back; it waits.  The bytes are rt_tonemap_u8(rt_denoise(...), spp = 1)'s.  Refusals as
 * rt_denoise_device's; a device that does not exist RT_ERR_DEVICE. */
int rt_denoise_frame_u8(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                        const float *gbuffer, const rt_denoise_params *params, int32_t device, uint8_t *out_rgb);
/* rt_accum_frame_u8 with the denoiser in front of the finish, for an accumulator that owns the
 * whole frame (world = 1), parity or fast, with uniform or per-pixel counts: the reported sums are
 * denoised with the accumulator's counts and its G-buffer (rendered on first use, kept until
 * rt_accum_free, like the filter's scratch), and the mean frame is finished at spp = 1.  Nothing
 * is written into the accumulator: sums, records, marks and a pending selection are untouched.
 * Falls under "one render per (scene, device) in flight".  With world > 1 RT_ERR_ARG (gather the
 * shards' sums and G-buffers and use the frame-level entry, rt_denoise_device); before the first
 * sample RT_ERR_ARG, like rt_accum_frame_u8. */
int rt_accum_frame_u8_denoised(rt_accum *accum, const rt_denoise_params *params, uint8_t *out_rgb);

/* The variance-guided mode of the denoiser (additive in ABI 6; after SVGF, Schied et al. 2017): the
 * same a-trous filter with three changes.  Surfaces whose radiance is not albedo-modulated pass
 * through; a firefly clamp runs before the filter; and the colour falloff is measured in standard
 * deviations of a per-pixel variance, which is filtered along with the colour.  A preview filter:
 * the clamp removes energy (on cornell 64 x 64 at 8 samples the filtered frame's
 * mean over the clamped range is about three quarters of the converged frame's), and without a
 * caller's variance the variance is a spatial estimate, which cannot tell noise from detail that
 * the albedo does not carry.  rt_denoise and its kin above are untouched by it.
 * csrc/rt_denoise_guided.h is its text, shared by the device kernels and the host function; the
 * arithmetic rules are rt_denoise's (f32 +, -, *, /, comparisons and selects in the order written,
 * nothing contracted, correctly rounded division), so host, device and a restatement agree bit
 * for bit.
 *
 * Parameters.  A NULL params is all defaults.  iterations, sigma_plane, normal_power_log2: as
 * rt_denoise_params.  sigma_var: <= 0 takes the default 2.  firefly: 0 takes the default 8, a
 * negative one switches the clamp off.  A NaN or infinite sigma_var, sigma_plane or firefly is
 * RT_ERR_ARG.  sigma_var = 2 and firefly = 8, and the 5 x 5 and 7 x 7 windows below, come from a
 * coarse sweep on three small fixtures (cornell 64 x 64, sponza_mini 64 x 36, cornell_blob
 * 48 x 48; sigma_var in {1, 2, 4}, firefly in {off, 2, 4, 8, 16}); they were not tuned on the
 * headline frame.
 *
 * Inputs and out_mean as rt_denoise's.  variance: NULL, or W * H floats, the variance of each
 * pixel's demodulated mean L summed over the channels (a moments accumulator measures it:
 * rt_accum_variance below).  out_variance: NULL, or W * H floats (below).
 *
 * Write geo(p, q) = nd * wp with nd and wp exactly rt_denoise's normal and plane terms for centre
 * p and tap q, and lum(L) = (0.2126f * L.x + 0.7152f * L.y) + 0.0722f * L.z.
 * 1. Prepare: rt_denoise's m, a', L and kind, and then: a hit whose three albedo channels are all
 *    not > 1e-3f is of kind pass, whatever its count (an emitter, a black surface: its own mean
 *    goes through and it reaches no other pixel).  Only a valid pixel keeps its L.
 * 2. Firefly clamp, skipped when firefly < 0; every pixel reads the unclamped frame.  For a valid
 *    p, over the 24 taps q = p + (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner, centre skipped,
 *    using a tap that is inside the frame, valid and has g = geo(p, q) > 0:
 *      sg = sg + g;  sl = sl + g * lum(Lq)                         both from +0
 *    and when sg > 0:  mean = sl / sg;  cap = firefly * (mean > 0 ? mean : 0);  when lum(Lp) > cap,
 *    scale = cap / lum(Lp) and each channel of Lp is multiplied by scale.
 * 3. Variance V.  With `variance` given: the caller's value for a valid pixel when it is finite
 *    and > 0, else 0.  With NULL: for a valid p over the 49 taps of the 7 x 7 window on the
 *    clamped L (centre included, dy outer, dx inner), using a tap as in 2:
 *      sg = sg + g;  s1 = s1 + g * Lq;  s2 = s2 + g * (Lq * Lq)   per channel; the tap is counted
 *      mu = s1 / sg;  var = s2 / sg - mu * mu;  var = var > 0 ? var : 0   per channel
 *      V = (var.x + var.y) + var.z;  V = 0 when fewer than 2 taps were counted or V is not finite
 *    A pixel that is not valid holds V = 0.
 * 4. Level k = 0 .. iterations - 1, stride s = 2^k, reading one buffer of (L, kind, V) and writing
 *    the other.  A pass centre is copied.  Otherwise first the variance prefilter over the 3 x 3
 *    taps q = p + (dx, dy) (stride 1, dy outer, dx inner) that are inside and valid in the level's
 *    input, c(0) = 1/2, c(+-1) = 1/4:
 *      gw = gw + c(dx) * c(dy);  gv = gv + (c(dx) * c(dy)) * Vq
 *      vbar = gw > 0 ? gv / gw : 0;  cden = (sigma_var * sigma_var) * vbar + 1e-8f
 *    (no halving per level: the variance shrinks by itself), then rt_denoise's 25 taps with its
 *    skips and its h, nd, wp, and
 *      wc = 1 for a fill centre, else 1 / (1 + ((d.x * d.x + d.y * d.y) + d.z * d.z) / cden)
 *      w  = ((h * nd) * wp) * wc;  a tap whose w is not > 0 is skipped
 *      sw = sw + w;  sL = sL + w * Lq;  sV = sV + (w * w) * Vq
 *    The centre becomes (sL / sw, valid, sV / (sw * sw)) when sw > 0 and the three colour
 *    quotients are finite, keeping its old V when the new one is not finite; (0, 0, 0, its kind,
 *    V = 0) when sw is not > 0; and stays as it was when a colour quotient overflowed.
 * 5. Resolve as rt_denoise.  out_variance receives V after the last level for a pixel that is
 *    valid then and 0 for every other.  With iterations = 0 out_mean is m bit for bit, nothing is
 *    clamped, and out_variance is all zeros.
 *
 * rt_denoise_guided runs on the host; rt_denoise_guided_device on the current HIP device,
 * asynchronously on `stream`, every pointer but params a device pointer, with the host function's
 * bits.  Its scratch (72 B per pixel: rt_denoise's 64 and the two variance words) is the one
 * rt_denoise_device keeps per device, so it only grows and one call of either per device may be in
 * flight.  Refusals as rt_denoise's.  rt_denoise_guided_frame_u8 is rt_denoise_frame_u8 with this
 * mode (variance NULL or W * H host floats); rt_accum_frame_u8_guided is
 * rt_accum_frame_u8_denoised with this mode and variance = NULL: the same accumulator contract
 * (world = 1, nothing written into the accumulator, the G-buffer rendered on first use, world > 1
 * and "no samples" RT_ERR_ARG, a refused call leaves nothing half made). */
typedef struct {
    int32_t iterations;          /* 0..6; < 0: 5 (0 is a value: the mean, bit for bit)             */
    float sigma_var;             /* <= 0: 2.  colour falloff in standard deviations                 */
    float sigma_plane;           /* <= 0: 0.02, as rt_denoise_params                                */
    int32_t normal_power_log2;   /* 1..16; <= 0: 6, as rt_denoise_params                            */
    float firefly;               /* 0: 8.  < 0: no clamp.  > 0: cap = firefly x neighbourhood mean  */
} rt_denoise_guided_params;
int rt_denoise_guided(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                      const float *gbuffer, const float *variance, const rt_denoise_guided_params *params,
                      float *out_mean, float *out_variance);
int rt_denoise_guided_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                             const float *d_gbuffer, const float *d_variance, const rt_denoise_guided_params *params,
                             float *d_out_mean, float *d_out_variance, void *stream);
int rt_denoise_guided_frame_u8(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                               const float *gbuffer, const float *variance, const rt_denoise_guided_params *params,
                               int32_t device, uint8_t *out_rgb);
int rt_accum_frame_u8_guided(rt_accum *accum, const rt_denoise_guided_params *params, uint8_t *out_rgb);

/* --- per-sample second moments: measured variance ----------------------------------------
 * A moments accumulator is a fast accumulator (rt_accum_create_fast) that keeps, beside the sum S
 * of a pixel's sample colours x, the sum Q of their squares.  For sample s of a pixel with colour
 * x (three f32 values), q[ch] = x[ch] * x[ch], one f32 multiply.  Q is the fast fold of q exactly
 * as S is the fast fold of x: with chunk size c, the partials of a chunk are added in sample order
 * from +0.f, the chunk partials in chunk order from +0.f, and an open chunk is carried as open2
 * and reported as total2 + open2 when n % c != 0.  Non-finite samples give non-finite moments;
 * nothing is clamped.  Per pixel the accumulator keeps a moment record of eight words in a buffer
 * of its own (total2 x y z, open2 x y z, 0, 0) and the reported moment (three floats).
 *
 * Variance of the mean, V = variance_of_mean(n, S, Q, albedo, hit), the `variance` input of
 * rt_denoise_guided: a miss (triangle id of the first-hit record < 0) or n < 2 gives 0; otherwise
 * r = 1.f / (float)n, r1 = 1.f / (float)(n - 1) and per channel
 *   m = S * r;  e2 = Q * r;  v = e2 - m * m;  v = v > 0 ? v : 0;  vm = v * r1
 *   a' = albedo > 1e-3f ? albedo : 1e-3f;  d = vm / (a' * a')
 * V = (d0 + d1) + d2, and a V that is not finite gives 0.
 * Relative error, relative_error(n, S, Q), n >= 2, with m and vm as above:
 *   ((sqrtf(vm0) + sqrtf(vm1)) + sqrtf(vm2)) / sqrtf(((m0 + m1) + m2) + 1e-4f)
 * the standard error of the mean normalised as rt_accum_select's estimate is.
 * Known limit: e2 - m * m cancels in f32; the error of vm is bounded by
 * 4 (n + 2) 2^-24 e2 r1 (each of e2 and m * m carries at most n + 2 roundings).
 *
 * rt_accum_create_fast_moments is rt_accum_create_fast with the moment buffers, made once at
 * creation; the same refusals.  On a moments accumulator every other rt_accum_* entry behaves as on
 * a fast one, and its sums are a fast accumulator's bit for bit.  rt_accum_has_moments: 0 or 1.
 * rt_accum_moments writes the reported moments (shard layout, three floats per pixel) to host
 * memory and waits; rt_accum_device_moments is their device buffer, valid until rt_accum_free.  On
 * an accumulator without moments the first is RT_ERR_ARG and the second NULL.
 *
 * rt_variance_from_moments runs on the host: width * height pixels (any pixel range with its own
 * first-hit records: it is per pixel, so a shard is fine), counts or NULL and one spp as
 * rt_denoise's, out width * height floats.  rt_variance_from_moments_device runs on the current
 * HIP device, asynchronously on `stream`, every pointer a device pointer, with the same bits.
 * Refusals as rt_denoise's.  rt_accum_variance writes V of the accumulator's own pixels (its
 * counts, its G-buffer: rendered on first use, for any world) to host memory and waits.
 *
 * rt_accum_frame_u8_guided_measured is rt_accum_frame_u8_guided with `variance` set to the
 * measured V instead of NULL: the same contract (world = 1, nothing written into the accumulator).
 *
 * rt_accum_select_variance is rt_accum_select with its steps 1 and 2 unchanged, then
 *   n_b < 2 -> selected;  otherwise selected iff relative_error(n_b, S_b, Q_b) > threshold
 * (a NaN is never selected).  It needs no mark and ignores one.  rt_accum_add_selected,
 * rt_accum_selection and the pending-selection rules apply unchanged.
 *
 * rt_accum_save on a moments accumulator writes magic "RTMACCUM", version 1: the fast file's
 * header (the chunk size in its place), the fast records verbatim, then the moment records
 * verbatim.  rt_accum_load reads all three kinds and returns that kind; for this one a wrong
 * length, and non-zero open2 or pad words where next % c == 0, are RT_ERR_FORMAT before any
 * device call.  Every entry below that needs moments is RT_ERR_ARG on an accumulator without. */
int rt_accum_create_fast_moments(rt_scene *scene, const rt_params *params, rt_accum **out);
int32_t rt_accum_has_moments(const rt_accum *accum);
int rt_accum_moments(rt_accum *accum, float *out);
const float *rt_accum_device_moments(rt_accum *accum);
int rt_variance_from_moments(const float *sums, const float *moments, const int32_t *counts, int32_t spp, int32_t width,
                             int32_t height, const float *gbuffer, float *out);
int rt_variance_from_moments_device(const float *d_sums, const float *d_moments, const int32_t *d_counts, int32_t spp,
                                    int32_t width, int32_t height, const float *d_gbuffer, float *d_out, void *stream);
int rt_accum_variance(rt_accum *accum, float *out);
int rt_accum_frame_u8_guided_measured(rt_accum *accum, const rt_denoise_guided_params *params, uint8_t *out_rgb);
int rt_accum_select_variance(rt_accum *accum, const rt_select *select, void *stream, int64_t *n_selected);

/* --- reprojected temporal history (additive in ABI 6) ---------------------------------------
 * The temporal half of SVGF (Schied et al. 2017) in front of the filters above: a frame's
 * demodulated radiance is blended with the previous frame's result at the pixel where the same
 * surface point was seen, found through the world position P of the first-hit record and the
 * previous camera.  A pure function of its inputs.  csrc/rt_temporal.h is its text, shared by the
 * device kernel and the host function; the arithmetic rules are rt_denoise's (f32 +, -, *, /,
 * comparisons and selects in the order written, nothing contracted, correctly rounded division).
 * A still camera gains nothing this way: parity frames of one view are identical, and progressive
 * passes (rt_accum_*) are the tool for a still view.  The history is for motion.
 *
 * Parameters.  A NULL params is all defaults.  alpha, alpha_moments: <= 0 takes 0.2, > 1 is
 * RT_ERR_ARG.  sigma_plane: <= 0 takes 0.02.  normal_min: <= 0 takes 0.9.  max_history: <= 0 takes
 * 65536, more than 2^20 is RT_ERR_ARG.  A NaN or infinite float parameter is RT_ERR_ARG.  The
 * thresholds are picked, not measured: 0.2, 0.02 and 0.9, a hard plane test, and the bilinear
 * footprint without SVGF's 3 x 3 fallback.
 *
 * A history is three planes of W * H 16-byte quads, plane-major (RT_HISTORY_WORDS words per
 * pixel): plane 0 (L.xyz, N), plane 1 (M1.xyz, 0), plane 2 (M2.xyz, 0).  L is the temporally
 * integrated demodulated radiance, N the history length in frames (a float), M1 and M2 the
 * integrated per-channel first and second moments of L.  sums, counts / spp, width, height and
 * gbuffer are rt_denoise's inputs for the new frame; cam_prev, gbuffer_prev and history_prev are
 * the previous frame's camera, records and history_out.  With history_prev NULL (a first frame)
 * cam_prev and gbuffer_prev may be NULL; with it given they may not.  out_mean (W * H * 3) and
 * out_variance (W * H) may each be NULL.  history_out must not be history_prev.
 *
 * The rule, per pixel p = (i, j) with record (Np, tp, albedo, E, Pp, mesh):
 * 0. Prepare: rt_denoise's m, a', L and kind.
 * 1. Kind pass: the history record is zero words, out_mean = m, out_variance = 0; done.
 * 2. Look-up ("no history" when history_prev is NULL).  R, U, F: the three axes of cam_prev.
 *      v = Pp - pos per component;  z = (v.x * F.x + v.y * F.y) + v.z * F.z;  no history unless z > 0
 *      cx = ((v.x * R.x + v.y * R.y) + v.z * R.z) / z;  cy likewise with U
 *      fx = ((cx / tan_x + 1.f) * 0.5f) * (float)W - 0.5f      (the inverse of the camera ray)
 *      fy = ((1.f - cy / tan_y) * 0.5f) * (float)H - 0.5f
 *    no history unless fx > -1 && fx < (float)W && fy > -1 && fy < (float)H (a NaN fails; the test
 *    comes before any conversion to int).  x0 = (int)fx, less 1 when (float)x0 > fx;
 *    wx = fx - (float)x0; the same for y.  Four taps, dy = 0, 1 outer, dx = 0, 1 inner, at
 *    q = (x0 + dx, y0 + dy) with b = (dx ? wx : 1.f - wx) * (dy ? wy : 1.f - wy).  A tap is used iff
 *    q is inside the frame; b > 0; history_prev[q].N > 0; the mesh id of gbuffer_prev[q] is >= 0 and
 *    equals p's; (Np.x * Nq.x + Np.y * Nq.y) + Np.z * Nq.z >= normal_min; and |pd| <= sigma_plane * tp
 *    with pd the numerator of rt_denoise's plane term for Pq - Pp.  From +0:
 *      sb += b;  sL += b * Lq;  sN += b * Nq;  sM1 += b * M1q;  sM2 += b * M2q
 *    There is history iff sb > 0 and all ten quotients by sb (Lh, Nh, M1h, M2h) are finite.
 * 3. Integrate, with rN = 1.f / N', a = alpha > rN ? alpha : rN, am likewise from alpha_moments:
 *      valid, history:     N' = min(Nh + 1.f, (float)max_history);  L' = Lh + a * (L - Lh);
 *                          M1' = M1h + am * (L - M1h);  M2' = M2h + am * (L * L - M2h); a non-finite
 *                          result in any of the nine sends the pixel to the next line
 *      valid, no history:  N' = 1;  L' = M1' = L;  M2' = L * L
 *      fill, history:      N' = Nh, and L', M1', M2' are the history's
 *      fill, no history:   the record is zero words (N' = 0)
 * 4. The history record is written as laid out above.  out_mean = L' * a' + E per channel
 *    (rt_denoise's resolve: an unfilled fill pixel gives E).  out_variance, for N' >= 2: per channel
 *    vc = M2' - M1' * M1', taken as 0 unless > 0; V = ((v0 + v1) + v2) * a, taken as 0 when not
 *    finite; 0 otherwise.  That is the variance of the integrated mean were the frames independent,
 *    summed over the channels: the form rt_denoise_guided's `variance` input takes.  out_mean goes
 *    to the denoisers as sums at spp = 1.
 * Known limits: a freshly disoccluded pixel reports V = 0 (one frame measures no variance), and
 * the weighting is by frames, not by sample counts.
 *
 * rt_temporal runs on the host; rt_temporal_device on the current HIP device, asynchronously on
 * `stream`, every pointer but cam_prev and params a device pointer (16-byte aligned histories and
 * records), with the host function's bits and no scratch.  Refusals as rt_denoise's, with
 * history_out in out_mean's place.
 *
 * rt_history is the object callers use: two histories and two G-buffers on one device for a scene's
 * W x H (the scene must be uploaded there).  rt_history_push renders the scene's G-buffer at its
 * current camera into the current slot, runs the step against the previous slot and the previous
 * camera, swaps the slots and remembers the camera; the first push, and the first after
 * rt_history_reset, has no history.  Asynchronous on `stream`; it uses none of the scene's
 * workspace, and a refused call leaves nothing half made.  rt_history_gbuffer_device: the records
 * of the last push's view (NULL before one), for rt_denoise*_device without rendering them twice.
 * rt_history_lengths: N per pixel (W * H floats) to host memory; waits; zeros before a push.  Free
 * a history before its scene.
 * rt_history_push_frame_u8 is the push for a caller that holds host arrays and no HIP (the CLI), as
 * rt_denoise_frame_u8 is for the filter: sums and counts (or NULL and spp) are copied to the
 * history's device and pushed; the integrated mean, at spp = 1 and with the push's records, passes
 * through rt_denoise_device (dparams given), rt_denoise_guided_device with the step's out_variance
 * as its variance (gparams given; DESIGN.md 5.18 has the measurement behind that choice) or neither
 * (both NULL; both given is RT_ERR_ARG), and is finished to W * H * 3 bytes; it waits. */
#define RT_HISTORY_WORDS 12
typedef struct {
    float alpha;           /* <= 0: 0.2.  least weight of the new frame's colour                */
    float alpha_moments;   /* <= 0: 0.2.  the same for the moments                              */
    float sigma_plane;     /* <= 0: 0.02. plane test, fraction of the centre's hit distance     */
    float normal_min;      /* <= 0: 0.9.  least dot product of the two shading normals          */
    int32_t max_history;   /* <= 0: 65536. cap of the history length                            */
} rt_temporal_params;
int rt_temporal(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                const float *gbuffer, const rt_camera *cam_prev, const float *gbuffer_prev,
                const float *history_prev, const rt_temporal_params *params,
                float *history_out, float *out_mean, float *out_variance);
int rt_temporal_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                       const float *d_gbuffer, const rt_camera *cam_prev, const float *d_gbuffer_prev,
                       const float *d_history_prev, const rt_temporal_params *params,
                       float *d_history_out, float *d_out_mean, float *d_out_variance, void *stream);
typedef struct rt_history rt_history;
int rt_history_create(rt_scene *scene, int32_t device, rt_history **out);
int rt_history_push(rt_history *h, const float *d_sums, const int32_t *d_counts, int32_t spp,
                    const rt_temporal_params *params, float *d_out_mean, float *d_out_variance, void *stream);
int rt_history_push_frame_u8(rt_history *h, const float *sums, const int32_t *counts, int32_t spp,
                             const rt_temporal_params *tparams, const rt_denoise_params *dparams,
                             const rt_denoise_guided_params *gparams, uint8_t *out_rgb);
const float *rt_history_gbuffer_device(rt_history *h);
int rt_history_lengths(rt_history *h, float *out);
int rt_history_reset(rt_history *h);
void rt_history_free(rt_history *h);

/* --- per-pixel motion records: the history follows moved geometry (additive in ABI 6) ----------
 * Opt-in.  A history that has not called rt_history_enable_motion, and a call of rt_temporal*
 * without motion records, behave in every bit as written above.  DESIGN.md 5.24.
 *
 * rt_temporal's look-up projects the pixel's current position P through the previous camera; for a
 * surface that rt_scene_update_tris* moved between two frames that is the wrong point of the
 * previous frame.  A motion record carries the point (and the shading normal) the pixel sees now
 * back to where that point of that triangle was, from the triangle id of the first-hit record and
 * the triangle array as it stood before (tri_prev).  csrc/rt_motion.h is the rule's text, shared by
 * the host function, the device kernel and the CPU tests; the arithmetic rules are rt_denoise's
 * (f32 +, -, *, /, comparisons and selects in the order written, nothing contracted, correctly
 * rounded division) and no float is converted to an int.
 *
 * A motion plane is two 16-byte quads per pixel (RT_MOTION_WORDS words), pixel-major like the
 * G-buffer: quad 0 (P_prev.xyz, state as int bits), quad 1 (N_prev.xyz, 0).  States:
 *   0  static   the record is the pixel's own P and N, bit for bit
 *   1  carried
 *   2  lost     no history may be taken for this pixel; P_prev and N_prev are zero words
 * The rule, per pixel with record (N, t, id, P), T = tri[id], T' = tri_prev[id] (words 0..8 of a
 * triangle are used: v0, U, V; primed letters are T' 's):
 *   miss      id < 0 or id >= n_tris (tested, never indexed): state 0 with the record's own words
 *             (zero words for a miss).
 *   unmoved   words 0..8 of T and T' equal as bit patterns: state 0, P_prev = P, N_prev = N.
 *   moved     e = P - v0 per component.  With dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z:
 *               a = dot(U, U); b = dot(U, V); c = dot(V, V); det = a * c - b * b
 *             state 2 unless det > (a * c) * 0x1p-20f and det is finite (a zero edge, parallel edges, and
 *             a sliver whose edges meet at less than 0.06 degrees, where the rounding of det, a few
 *             2^-24 of a * c, would decide: a NaN fails).  d = dot(U, e); f = dot(V, e);
 *               u = (c * d - b * f) / det;  v = (a * f - b * d) / det
 *               dv0 = v0' - v0;  dU = U' - U;  dV = V' - V      per component
 *               P_prev = P + ((dv0 + u * dU) + v * dV)          per component
 *             In exact arithmetic that is v0' + u U' + v V' plus P's own distance from its triangle's
 *             plane; written as a displacement its error scales with the motion, not with the
 *             coordinates, and a translation whose offset is exact in f32 is carried exactly.
 *   normal    W = cross(U, V), W' = cross(U', V') (x = a.y * b.z - b.y * a.z, and cyclically).
 *               dn = dot(U, N); fn = dot(V, N); al = (c * dn - b * fn) / det; be = (a * fn - b * dn) / det
 *               ga = dot(W, N) / dot(W, W);  dW = W' - W
 *               N_prev = N + ((al * dU + be * dV) + ga * dW)    per component
 *             For a rigid motion that is the rotated normal up to rounding; for a deforming triangle
 *             it is an approximation.  It is not renormalised.
 *   lost      any non-finite word of P_prev or N_prev: state 2.  Non-finite and degenerate triangles
 *             and a non-finite P end here or at det.  Otherwise state 1.
 * The look-up with motion is step 2 of rt_temporal with: state 0 (and motion NULL) the pixel's own
 * values, exactly as written there; state 1: P_prev in Pp's place for the projection through
 * cam_prev, and ((N_prev, tp), P_prev, sigma_plane * tp) as the centre of the normal and plane
 * tests (tp the pixel's own hit distance); any other state: no history.  Steps 0, 1, 3, 4 as above.
 *
 * rt_motion runs on the host.  rt_motion_device runs on the current HIP device, asynchronously on
 * `stream`, with the host function's bits: one kernel, every pointer a 16-byte aligned device
 * pointer.  With n_tris == 0 tri and tri_prev may be NULL.  rt_temporal_motion(_device) are
 * rt_temporal(_device) with the motion plane as a further argument; NULL is rt_temporal(_device)
 * exactly.  Refusals, all before any launch: those of rt_temporal; a NULL argument, a bad frame size
 * (RT_ERR_ARG), width * height above 2^31 - 1 (RT_ERR_LIMIT), a misaligned device pointer, and motion
 * given while history_prev is NULL (RT_ERR_ARG).
 *
 * rt_history_enable_motion allocates a copy of the scene's triangles (n_tris x 12 floats) and one
 * motion plane on the history's device.  It is allowed before the first push or directly after
 * rt_history_reset, RT_ERR_ARG otherwise; a failed allocation leaves the history as it was; a second
 * call is RT_OK.  The scene counts its rt_scene_update_tris* calls (a counter of its own, not the
 * epoch the camera also bumps).  A push of such a history, all on the caller's stream: the G-buffer;
 * if there is a previous push and the counter differs from the one the snapshot was taken at, the
 * motion kernel against the snapshot and the step with its records, otherwise exactly the one launch
 * of a history without motion (an unmoved scene pays nothing); then, if the counter differs or there
 * is no snapshot yet, a device-to-device copy of the scene's triangles into the snapshot.  Several
 * updates between two pushes are one motion.  The snapshot copy reads the scene's device copy on the
 * caller's stream: as for every entry, no update may run while it is in flight.
 * rt_history_motion_device: the last push's motion plane on the device, NULL when that push ran
 * without one (the first, an unmoved one, a history that has not opted in).  rt_history_motion: that
 * plane to host memory (W * H * RT_MOTION_WORDS floats); waits; RT_ERR_ARG when there is none.
 * Limits: a triangle is followed by its id, so a changed topology is not followed (there is no
 * rebuild); textures and materials are taken as unmoved. */
#define RT_MOTION_WORDS 8
int rt_motion(const float *gbuffer, int32_t width, int32_t height, const float *tri, const float *tri_prev,
              uint32_t n_tris, float *out_motion);
int rt_motion_device(const float *d_gbuffer, int32_t width, int32_t height, const float *d_tri,
                     const float *d_tri_prev, uint32_t n_tris, float *d_out_motion, void *stream);
int rt_temporal_motion(const float *sums, const int32_t *counts, int32_t spp, int32_t width, int32_t height,
                       const float *gbuffer, const rt_camera *cam_prev, const float *gbuffer_prev,
                       const float *history_prev, const rt_temporal_params *params,
                       float *history_out, float *out_mean, float *out_variance, const float *motion);
int rt_temporal_motion_device(const float *d_sums, const int32_t *d_counts, int32_t spp, int32_t width, int32_t height,
                              const float *d_gbuffer, const rt_camera *cam_prev, const float *d_gbuffer_prev,
                              const float *d_history_prev, const rt_temporal_params *params,
                              float *d_history_out, float *d_out_mean, float *d_out_variance,
                              const float *d_motion, void *stream);
int rt_history_enable_motion(rt_history *h);
const float *rt_history_motion_device(rt_history *h);
int rt_history_motion(rt_history *h, float *out);

/* --- misc --------------------------------------------------------------------------- */
const char *rt_last_error(void);
int32_t rt_abi_version(void);
int32_t rt_device_count(void);
int rt_device_synchronize(void);
/* Device self-check of hardware-dependent arithmetic the kernels rely on for exactness
 * (no reference counterpart; test entry).  which 0: the traversal's fast reciprocal
 * (rt_wavefront.h rcp_ieee) against IEEE division over every float with a normal
 * reciprocal; which 1: the computed linear texel decode (rt_path.h unorm8) against
 * (float)b / 255.f for every byte, and the packed LDS RNG word round trip over every minstd
 * state and both normal-cache flags; which 2: the cooperative leaf step (rt_wavefront.h
 * trav_step_coop) against the per-lane in-order strict-< loop over 2^16 synthetic leaves rich
 * in equal-t ties, NaN and infinite vertices (four launches); which 3: the traversal's
 * root-free cull (rt_wavefront.h far_gt and kFarMax2) against the device's sqrtf(x) > acc over
 * 2^24 generated pairs around the rounding boundary, the special values and the floats
 * around the 1e9 constant; which 4: the material records of every uploaded scene against the
 * scene's own tables; which 5: whole closest-hit queries of 16,384 hashed rays on every
 * uploaded scene through the cooperative step (one and two frames popped per step; 12 and 4
 * stack frames in LDS; with every best frame and with none after a near subtree without a
 * hit: eight launches) against the per-lane step loop (t, triangle, local
 * best, AABB and triangle counts; a query that does not end within 4 x (nodes + triangles) +
 * 64 steps is a mismatch); *mismatches = values (cases) that differ (0 = exact). */
int rt_device_selfcheck(int32_t which, uint64_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif /* RT_HW_H */
