"""raytracing-hw_amd — MI355X-native path-tracing core behind the reference's render seam.

Python host mirror of the reference's hot-path interface (Korinin38/raytracing-hw):

    parse_scene_gltf(path, width, height, samples) -> Scene   # src/io/scene_parser.cpp:25
    Scene.render()                                          # src/core/scene.cpp:17-65
    Scene.draw_into(filename)                               # src/core/scene.cpp:67 / canvas.h:76-89

plus the float-level entry points the tests and the benchmark use
(`Scene.render_sums`, `Scene.render_device`).  Everything runs through the C ABI of
``librt_hw_amd.so`` (include/rt_hw.h); there is no CPU fallback — if the library or a
GPU is missing the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RT_LIB may point at the index-checked debug build (make -C raytracing-hw_amd debug)
LIB_PATH = os.environ.get("RT_LIB") or os.path.join(_HERE, "librt_hw_amd.so")
REPO_ROOT = os.path.dirname(_HERE)

_c_f = ctypes.POINTER(ctypes.c_float)
_c_i = ctypes.POINTER(ctypes.c_int32)
_c_u = ctypes.POINTER(ctypes.c_uint32)
_c_d = ctypes.POINTER(ctypes.c_double)
_c_b = ctypes.POINTER(ctypes.c_uint8)


class RtSceneView(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("samples", ctypes.c_int32), ("ray_depth", ctypes.c_int32),
        ("max_distance", ctypes.c_float), ("cam_pos", ctypes.c_float * 3), ("cam_axes", ctypes.c_float * 9),
        ("cam_fov", ctypes.c_float * 2), ("tan_half_fov", ctypes.c_float * 2),
        ("n_tris", ctypes.c_uint32), ("tri", _c_f), ("tri_attr", _c_f), ("tri_tan", _c_f),
        ("n_nodes", ctypes.c_uint32), ("node", _c_f), ("bvh_depth", ctypes.c_uint32),
        ("n_lights", ctypes.c_uint32), ("light", _c_f), ("n_light_nodes", ctypes.c_uint32), ("light_node", _c_f),
        ("light_bvh_depth", ctypes.c_uint32),
        ("n_meshes", ctypes.c_uint32), ("mesh_f", _c_f), ("mesh_tex", _c_i), ("mesh_normal_transform", _c_d),
        ("n_textures", ctypes.c_uint32), ("tex_info", _c_u), ("texels", _c_b), ("n_texel_bytes", ctypes.c_uint64),
    ]


ABI_VERSION = 6          # include/rt_hw.h RT_ABI_VERSION
KERNEL_LANE = 0          # RT_KERNEL_LANE: lane-resident persistent kernel (default)
KERNEL_WAVEFRONT = 4     # RT_KERNEL_WAVEFRONT: init / extend / shade launches
FLAG_KERNEL_TIMES = 1    # RT_FLAG_KERNEL_TIMES
FLAG_FAST = 2            # RT_FLAG_FAST: per-(pixel, sample) Philox-seeded streams, not bit-identical to the reference
FLAG_LIGHT_SPLIT = 4     # RT_FLAG_LIGHT_SPLIT: light-pdf walk as its own traversal state (same bits)
FLAG_NATURAL_ORDER = 8   # RT_FLAG_NATURAL_ORDER: row-major pixel order instead of the in-frame heaviest-first order
FLAG_NO_RUNAHEAD = 16    # RT_FLAG_NO_RUNAHEAD: no speculative sample runahead in the waves' tails (same bits)
FLAG_HEAVY_ORDER = 32    # RT_FLAG_HEAVY_ORDER: the heaviest-first order below 128 spp too (same bits)
# RtStats.schedule bits (include/rt_hw.h RT_SCHED_*): the kernels that rendered
SCHED_LANE, SCHED_RUNAHEAD, SCHED_FAST, SCHED_LIGHT_SPLIT, SCHED_WAVEFRONT = 1, 2, 4, 8, 16


class RtParams(ctypes.Structure):
    _fields_ = [("spp", ctypes.c_int32), ("rank", ctypes.c_int32), ("world", ctypes.c_int32),
                ("row_block", ctypes.c_int32), ("count", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("fast_chunk", ctypes.c_int32), ("device", ctypes.c_int32)]


class RtSelect(ctypes.Structure):
    """include/rt_hw.h rt_select: what rt_accum_select raises to `target`."""
    _fields_ = [("target", ctypes.c_int32), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("x1", ctypes.c_int32),
                ("y1", ctypes.c_int32), ("mask", _c_b), ("threshold", ctypes.c_float)]


class RtDenoiseParams(ctypes.Structure):
    """include/rt_hw.h rt_denoise_params; iterations < 0 and the other fields <= 0 take the defaults."""
    _fields_ = [("iterations", ctypes.c_int32), ("sigma_color", ctypes.c_float), ("sigma_plane", ctypes.c_float),
                ("normal_power_log2", ctypes.c_int32)]


GBUFFER_WORDS = 16       # RT_GBUFFER_WORDS: 32-bit words of a first-hit record


def denoise_params(iterations=-1, sigma_color=0.0, sigma_plane=0.0, normal_power_log2=0):
    return RtDenoiseParams(int(iterations), float(sigma_color), float(sigma_plane), int(normal_power_log2))


class RtDenoiseGuidedParams(ctypes.Structure):
    """include/rt_hw.h rt_denoise_guided_params; firefly 0 takes the default, a negative one switches the clamp off."""
    _fields_ = [("iterations", ctypes.c_int32), ("sigma_var", ctypes.c_float), ("sigma_plane", ctypes.c_float),
                ("normal_power_log2", ctypes.c_int32), ("firefly", ctypes.c_float)]


def denoise_guided_params(iterations=-1, sigma_var=0.0, sigma_plane=0.0, normal_power_log2=0, firefly=0.0):
    return RtDenoiseGuidedParams(int(iterations), float(sigma_var), float(sigma_plane), int(normal_power_log2), float(firefly))


class RtCamera(ctypes.Structure):
    """include/rt_hw.h rt_camera: position, the axes right, up, forward, the half-angle tangents."""
    _fields_ = [("pos", ctypes.c_float * 3), ("axes", ctypes.c_float * 9), ("tan_half_fov", ctypes.c_float * 2)]


def make_camera(pos, axes, tan_half_fov):
    c = RtCamera()
    c.pos[:] = [float(x) for x in np.asarray(pos, np.float32).reshape(3)]
    c.axes[:] = [float(x) for x in np.asarray(axes, np.float32).reshape(9)]
    c.tan_half_fov[:] = [float(x) for x in np.asarray(tan_half_fov, np.float32).reshape(2)]
    return c


def _camera_arg(cam):
    """A camera dict (Scene.camera()), an RtCamera or None as the rt_camera the library reads."""
    if cam is None or isinstance(cam, RtCamera):
        return cam
    return make_camera(cam["pos"], cam["axes"], cam["tan_half_fov"])


MOTION_WORDS = 8         # RT_MOTION_WORDS: 32-bit words of a pixel's motion record (two quads)
HISTORY_WORDS = 12       # RT_HISTORY_WORDS: 32-bit words of a pixel's temporal history (three planes of quads)


class RtTemporalParams(ctypes.Structure):
    """include/rt_hw.h rt_temporal_params; every field <= 0 takes its default."""
    _fields_ = [("alpha", ctypes.c_float), ("alpha_moments", ctypes.c_float), ("sigma_plane", ctypes.c_float),
                ("normal_min", ctypes.c_float), ("max_history", ctypes.c_int32)]


def temporal_params(alpha=0.0, alpha_moments=0.0, sigma_plane=0.0, normal_min=0.0, max_history=0):
    return RtTemporalParams(float(alpha), float(alpha_moments), float(sigma_plane), float(normal_min), int(max_history))


class RtStats(ctypes.Structure):
    _fields_ = [("pixels", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("rays", ctypes.c_uint64),
                ("aabb_tests", ctypes.c_uint64), ("tri_tests", ctypes.c_uint64), ("light_queries", ctypes.c_uint64),
                ("light_aabb_tests", ctypes.c_uint64), ("light_tri_tests", ctypes.c_uint64), ("shading_hits", ctypes.c_uint64),
                ("render_ms", ctypes.c_double), ("extend_ms", ctypes.c_double), ("shade_ms", ctypes.c_double),
                ("extend_launches", ctypes.c_uint64), ("shade_launches", ctypes.c_uint64), ("extend_rays", ctypes.c_uint64),
                ("order_ms", ctypes.c_double), ("gather_ms", ctypes.c_double), ("devices", ctypes.c_uint64),
                ("schedule", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/rt_hw.h declares, with its ctypes signature
ABI = {
    "rt_scene_load_gltf": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.POINTER(ctypes.c_void_p)]),
    "rt_scene_from_view": (ctypes.c_int, [ctypes.POINTER(RtSceneView), ctypes.POINTER(ctypes.c_void_p)]),
    "rt_scene_get_view": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtSceneView)]),
    "rt_scene_free": (None, [ctypes.c_void_p]),
    "rt_scene_get_camera": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtCamera)]),
    "rt_scene_set_camera": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtCamera)]),
    "rt_scene_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32]),
    "rt_shard_rows": (ctypes.c_int64, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_i]),
    "rt_render": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), _c_f, ctypes.POINTER(RtStats)]),
    "rt_render_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.POINTER(RtStats)]),
    "rt_render_multi": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.c_int32, _c_f,
                                       ctypes.POINTER(RtStats)]),
    "rt_render_frame": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.c_int32, _c_i, _c_b, _c_f,
                                       ctypes.POINTER(RtStats)]),
    "rt_intersect_rays": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _c_f, _c_f, _c_f,
                                         ctypes.POINTER(ctypes.c_int64)]),
    "rt_intersect_rays_via": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, _c_f, _c_f, _c_f,
                                             ctypes.POINTER(ctypes.c_int64)]),
    "rt_sample_frames_via": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, _c_f,
                                            ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), _c_f,
                                            ctypes.POINTER(ctypes.c_int64)]),
    "rt_tonemap_u8": (ctypes.c_int, [_c_f, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_b]),
    "rt_tonemap_u8_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "rt_write_ppm": (ctypes.c_int, [ctypes.c_char_p, _c_b, ctypes.c_int32, ctypes.c_int32]),
    "rt_last_error": (ctypes.c_char_p, []),
    "rt_abi_version": (ctypes.c_int32, []),
    "rt_device_count": (ctypes.c_int32, []),
    "rt_device_synchronize": (ctypes.c_int, []),
    "rt_device_selfcheck": (ctypes.c_int, [ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]),
    # progressive rendering: a shard's per-pixel chain state kept between passes
    "rt_accum_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.POINTER(ctypes.c_void_p)]),
    "rt_accum_add": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(RtStats)]),
    "rt_accum_samples": (ctypes.c_int32, [ctypes.c_void_p]),
    "rt_accum_sums": (ctypes.c_int, [ctypes.c_void_p, _c_f]),
    "rt_accum_device_sums": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rt_accum_frame_u8": (ctypes.c_int, [ctypes.c_void_p, _c_b]),
    "rt_accum_state": (ctypes.c_int, [ctypes.c_void_p, _c_u]),
    "rt_accum_save": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "rt_accum_load": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]),
    "rt_accum_free": (None, [ctypes.c_void_p]),
    "rt_accum_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    # per-pixel sample counts: subset passes and adaptive refinement
    "rt_accum_mark": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rt_accum_select": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtSelect), ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_int64)]),
    "rt_accum_selection": (ctypes.c_int, [ctypes.c_void_p, _c_i]),
    "rt_accum_add_selected": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(RtStats)]),
    "rt_accum_counts": (ctypes.c_int, [ctypes.c_void_p, _c_i]),
    "rt_accum_counts_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rt_accum_sample_range": (ctypes.c_int, [ctypes.c_void_p, _c_i, _c_i]),
    "rt_tonemap_u8_counts": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, _c_b]),
    "rt_tonemap_u8_counts_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                                   ctypes.c_void_p, ctypes.c_void_p]),
    # fast-mode accumulators: progressive and adaptive passes on Philox units
    "rt_accum_create_fast": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.POINTER(ctypes.c_void_p)]),
    "rt_accum_fast_chunk": (ctypes.c_int32, [ctypes.c_void_p]),
    # first-hit feature buffer and frame denoiser
    "rt_gbuffer": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), _c_f]),
    "rt_gbuffer_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.c_void_p, ctypes.c_void_p]),
    "rt_denoise": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f,
                                  ctypes.POINTER(RtDenoiseParams), _c_f]),
    "rt_denoise_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.POINTER(RtDenoiseParams), ctypes.c_void_p, ctypes.c_void_p]),
    "rt_denoise_frame_u8": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f,
                                           ctypes.POINTER(RtDenoiseParams), ctypes.c_int32, _c_b]),
    "rt_accum_frame_u8_denoised": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtDenoiseParams), _c_b]),
    # the denoiser's variance-guided mode
    "rt_denoise_guided": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f, _c_f,
                                         ctypes.POINTER(RtDenoiseGuidedParams), _c_f, _c_f]),
    "rt_denoise_guided_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(RtDenoiseGuidedParams),
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rt_denoise_guided_frame_u8": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f, _c_f,
                                                  ctypes.POINTER(RtDenoiseGuidedParams), ctypes.c_int32, _c_b]),
    "rt_accum_frame_u8_guided": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtDenoiseGuidedParams), _c_b]),
    # per-sample second moments of fast-mode accumulators: measured variance
    "rt_accum_create_fast_moments": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtParams), ctypes.POINTER(ctypes.c_void_p)]),
    "rt_accum_has_moments": (ctypes.c_int32, [ctypes.c_void_p]),
    "rt_accum_moments": (ctypes.c_int, [ctypes.c_void_p, _c_f]),
    "rt_accum_device_moments": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rt_variance_from_moments": (ctypes.c_int, [_c_f, _c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f, _c_f]),
    "rt_variance_from_moments_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                       ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.c_void_p]),
    "rt_accum_variance": (ctypes.c_int, [ctypes.c_void_p, _c_f]),
    "rt_accum_frame_u8_guided_measured": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtDenoiseGuidedParams), _c_b]),
    "rt_accum_select_variance": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(RtSelect), ctypes.c_void_p,
                                                ctypes.POINTER(ctypes.c_int64)]),
    # reprojected temporal history
    "rt_temporal": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f, ctypes.POINTER(RtCamera), _c_f,
                                   _c_f, ctypes.POINTER(RtTemporalParams), _c_f, _c_f, _c_f]),
    "rt_temporal_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.POINTER(RtCamera), ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.POINTER(RtTemporalParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p]),
    "rt_history_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]),
    "rt_history_push": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                       ctypes.POINTER(RtTemporalParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rt_history_push_frame_u8": (ctypes.c_int, [ctypes.c_void_p, _c_f, _c_i, ctypes.c_int32, ctypes.POINTER(RtTemporalParams),
                                                ctypes.POINTER(RtDenoiseParams), ctypes.POINTER(RtDenoiseGuidedParams), _c_b]),
    "rt_history_gbuffer_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rt_history_lengths": (ctypes.c_int, [ctypes.c_void_p, _c_f]),
    "rt_history_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "rt_history_free": (None, [ctypes.c_void_p]),
    # per-pixel motion records: the history follows moved geometry
    "rt_motion": (ctypes.c_int, [_c_f, ctypes.c_int32, ctypes.c_int32, _c_f, _c_f, ctypes.c_uint32, _c_f]),
    "rt_motion_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]),
    "rt_temporal_motion": (ctypes.c_int, [_c_f, _c_i, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _c_f, ctypes.POINTER(RtCamera),
                                          _c_f, _c_f, ctypes.POINTER(RtTemporalParams), _c_f, _c_f, _c_f, _c_f]),
    "rt_temporal_motion_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_void_p, ctypes.POINTER(RtCamera), ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.POINTER(RtTemporalParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p]),
    "rt_history_enable_motion": (ctypes.c_int, [ctypes.c_void_p]),
    "rt_history_motion_device": (ctypes.c_void_p, [ctypes.c_void_p]),
    "rt_history_motion": (ctypes.c_int, [ctypes.c_void_p, _c_f]),
    # movable geometry: triangle updates and the BVH refit
    "rt_scene_update_tris": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, _c_f, _c_f, _c_f]),
    "rt_scene_update_tris_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rt_refit_view": (ctypes.c_int, [ctypes.POINTER(RtSceneView), _c_f]),
    "rt_scene_read_device": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_f, _c_f, _c_f, _c_f]),
    # movable lights: the opt-in, the light map, the light list and light-BVH refit
    "rt_scene_enable_light_updates": (ctypes.c_int, [ctypes.c_void_p]),
    "rt_scene_light_map": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
    "rt_relight_view": (ctypes.c_int, [ctypes.POINTER(RtSceneView), ctypes.POINTER(ctypes.c_uint32), _c_f, _c_f]),
    "rt_scene_read_device_lights": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_f, _c_f]),
    # posable meshes: rest data, per-mesh node matrices, the pose on the device
    "rt_scene_set_rest": (ctypes.c_int, [ctypes.c_void_p, _c_f, ctypes.POINTER(ctypes.c_uint32), _c_d]),
    "rt_scene_get_rest": (ctypes.c_int, [ctypes.c_void_p, _c_f, ctypes.POINTER(ctypes.c_uint32), _c_d]),
    "rt_scene_tri_source": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]),
    "rt_scene_enable_poses": (ctypes.c_int, [ctypes.c_void_p]),
    "rt_scene_get_mesh_transform": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, _c_d]),
    "rt_scene_pose_meshes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), _c_d]),
    "rt_pose_view": (ctypes.c_int, [ctypes.POINTER(RtSceneView), _c_f, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), _c_d,
                                    _c_f, _c_f, _c_d]),
    "rt_trs_matrix": (ctypes.c_int, [_c_f, _c_f, _c_f, _c_d]),
}

_lib_handle = None
# debug builds (make -C raytracing-hw_amd debug, RT_LIB=.../debug/librt_hw_amd.so) export
# rt_debug_take: every render then raises on a recorded device check (rt_path.h RT_CHECK)
# unless debug_raise is cleared (tests that provoke one)
debug_raise = True


def lib():
    """Load librt_hw_amd.so (built in-tree by `make -C raytracing-hw_amd`); raise if absent."""
    global _lib_handle
    if _lib_handle is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: build it with `make -C raytracing-hw_amd` "
                               "(there is no CPU fallback for the render path)")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        if hasattr(h, "rt_debug_take"):
            h.rt_debug_take.restype = ctypes.c_int
            h.rt_debug_take.argtypes = [ctypes.POINTER(ctypes.c_uint64)]
            h.rt_debug_set_poison.restype = ctypes.c_int
            h.rt_debug_set_poison.argtypes = [ctypes.c_int]
        _lib_handle = h
    return _lib_handle


def is_debug_build():
    return hasattr(lib(), "rt_debug_take")


def debug_take():
    """Debug builds: the first device check violation since the last call (code << 56 | value),
    0 = none; None on a release build."""
    if not is_debug_build():
        return None
    w = ctypes.c_uint64(0)
    _check(lib().rt_debug_take(ctypes.byref(w)))
    return int(w.value)


def debug_set_poison(on):
    """Debug builds: poison every lane's traversal phase and stack depth at the lane-resident
    kernel's start (the packing test)."""
    _check(lib().rt_debug_set_poison(int(on)))


def _after_render():
    if debug_raise and _lib_handle is not None and hasattr(_lib_handle, "rt_debug_take"):
        w = debug_take()
        if w:
            raise RtError(f"device check {w >> 56} failed (value {w & ((1 << 56) - 1):#x})")


class RtError(RuntimeError):
    pass


ERR_ARG, ERR_STATE = -1, -6   # include/rt_hw.h rt_status: what RtError.code holds


def _check(rc):
    if rc != 0:
        e = RtError(lib().rt_last_error().decode())
        e.code = rc
        raise e


def shard_rows(height, rank=0, world=1, row_block=8):
    n = lib().rt_shard_rows(height, rank, world, row_block, None)
    if n < 0:
        raise RtError(lib().rt_last_error().decode())
    rows = np.zeros(max(n, 1), np.int32)
    lib().rt_shard_rows(height, rank, world, row_block, rows.ctypes.data_as(_c_i))
    return rows[:n]


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class Scene:
    """Flattened scene (reference `Scene`, src/core/scene.h:14-38) owned by librt_hw_amd."""

    def __init__(self, handle, width, height, samples):
        self._h = ctypes.c_void_p(handle)
        self.width, self.height, self.samples = width, height, samples
        self.canvas = None

    @classmethod
    def load(cls, path, width, height, samples):
        h = ctypes.c_void_p()
        _check(lib().rt_scene_load_gltf(os.fsencode(path), width, height, samples, ctypes.byref(h)))
        return cls(h.value, width, height, samples)

    @classmethod
    def from_view(cls, arrays):
        """Scene from flattened arrays (dict as returned by view()); see rt_scene_from_view."""
        v, keep = make_view(arrays)
        h = ctypes.c_void_p()
        _check(lib().rt_scene_from_view(ctypes.byref(v), ctypes.byref(h)))
        del keep
        return cls(h.value, int(arrays["width"]), int(arrays["height"]), int(arrays["samples"]))

    def intersect_rays(self, org, dirs, path=0):
        """Closest hit + light pdf per ray: returns (f32 n x 4 [t,u,v,light_pdf], i64 n x 6).
        path: the traversal (rt_intersect_rays_via: 0 closest_hit, 1 per-lane steps, 2 coop step;
        ray i is thread i; hit = -2 where a bounded loop of paths 1 and 2 did not end)."""
        org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = org.shape[0]
        out_f = np.zeros((n, 4), np.float32)
        out_i = np.zeros((n, 6), np.int64)
        _check(lib().rt_intersect_rays_via(self._h, int(path), n, org.ctypes.data_as(_c_f), dirs.ctypes.data_as(_c_f),
                                           out_f.ctypes.data_as(_c_f),
                                           out_i.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        _after_render()
        return out_f, out_i

    def sample_frames(self, frame, seed, warm, path=0):
        """Sampled direction + pdf per shading frame (rt_sample_frames_via): frame n x 10 (point, normal,
        eye, roughness2), seed and warm n; returns (f32 n x 6 [dir, pdf, light pdf, next normal],
        i64 n x 4 [status, next engine output, light AABB tests, light triangle tests]).  path 0:
        scene_pdf, 1: the light_step walk and scene_pdf_lp; frame i is thread i; status -2 where
        path 1's walk did not end."""
        frame = np.ascontiguousarray(frame, np.float32).reshape(-1, 10)
        seed = np.ascontiguousarray(seed, np.uint32).reshape(-1)
        warm = np.ascontiguousarray(warm, np.uint32).reshape(-1)
        n = frame.shape[0]
        if seed.shape[0] != n or warm.shape[0] != n:
            raise ValueError("sample_frames: frame, seed and warm differ in length")
        out_f = np.zeros((n, 6), np.float32)
        out_i = np.zeros((n, 4), np.int64)
        c_u = ctypes.POINTER(ctypes.c_uint32)
        _check(lib().rt_sample_frames_via(self._h, int(path), n, frame.ctypes.data_as(_c_f), seed.ctypes.data_as(c_u),
                                          warm.ctypes.data_as(c_u), out_f.ctypes.data_as(_c_f),
                                          out_i.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        _after_render()
        return out_f, out_i

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib_handle is not None:
            _lib_handle.rt_scene_free(h)
            self._h = None

    def view(self):
        """Copies of the flattened arrays (the HBM layout, include/rt_hw.h rt_scene_view)."""
        v = RtSceneView()
        _check(lib().rt_scene_get_view(self._h, ctypes.byref(v)))
        out = {k: getattr(v, k) for k in ("width", "height", "samples", "ray_depth", "max_distance", "bvh_depth",
                                          "light_bvh_depth")}
        out["cam_pos"] = np.array(v.cam_pos[:], np.float32)
        out["cam_axes"] = np.array(v.cam_axes[:], np.float32).reshape(3, 3)
        out["cam_fov"] = np.array(v.cam_fov[:], np.float32)
        out["tan_half_fov"] = np.array(v.tan_half_fov[:], np.float32)
        out["tri"] = _arr(v.tri, 12 * v.n_tris, np.float32).reshape(-1, 12)
        out["tri_attr"] = _arr(v.tri_attr, 16 * v.n_tris, np.float32).reshape(-1, 16)
        out["tri_tan"] = _arr(v.tri_tan, 12 * v.n_tris, np.float32).reshape(-1, 12)
        out["node"] = _arr(v.node, 8 * v.n_nodes, np.float32).reshape(-1, 8)
        out["light"] = _arr(v.light, 16 * v.n_lights, np.float32).reshape(-1, 16)
        out["light_node"] = _arr(v.light_node, 8 * v.n_light_nodes, np.float32).reshape(-1, 8)
        out["mesh_f"] = _arr(v.mesh_f, 12 * v.n_meshes, np.float32).reshape(-1, 12)
        out["mesh_tex"] = _arr(v.mesh_tex, 4 * v.n_meshes, np.int32).reshape(-1, 4)
        out["mesh_normal_transform"] = _arr(v.mesh_normal_transform, 16 * v.n_meshes, np.float64).reshape(-1, 16)
        out["tex_info"] = _arr(v.tex_info, 4 * v.n_textures, np.uint32).reshape(-1, 4)
        out["texels"] = _arr(v.texels, int(v.n_texel_bytes), np.uint8)
        return out

    @property
    def handle(self):
        return self._h

    def camera(self):
        """rt_scene_get_camera: {"pos": (3,), "axes": (3, 3) rows right, up, forward, "tan_half_fov": (2,)}."""
        c = RtCamera()
        _check(lib().rt_scene_get_camera(self._h, ctypes.byref(c)))
        return {"pos": np.array(c.pos[:], np.float32), "axes": np.array(c.axes[:], np.float32).reshape(3, 3),
                "tan_half_fov": np.array(c.tan_half_fov[:], np.float32)}

    def set_camera(self, pos=None, axes=None, tan_half_fov=None):
        """rt_scene_set_camera: look from somewhere else without uploading anything (an omitted part
        is kept).  Not while a render or a pass of the scene is in flight; an accumulator of the
        scene then needs reset() before it renders on."""
        cur = self.camera()
        c = make_camera(cur["pos"] if pos is None else pos, cur["axes"] if axes is None else axes,
                        cur["tan_half_fov"] if tan_half_fov is None else tan_half_fov)
        _check(lib().rt_scene_set_camera(self._h, ctypes.byref(c)))

    def update_triangles(self, first, tri, attr=None, tan=None, device=None, stream_ptr=None):
        """rt_scene_update_tris: replace triangles [first, first + len(tri)) (post-build order) and
        refit every node box (csrc/rt_refit.h); the tree's topology is kept.  tri (n, 12), attr (n, 16)
        or None (kept), tan (n, 12) or None (kept): numpy arrays.  With device given
        (rt_scene_update_tris_device) they are torch tensors on that device (float32, contiguous; their
        data_ptr() is passed), the scene must be on that device alone, and the work is enqueued on
        stream_ptr.  Triangles of an emissive mesh are refused; an accumulator of the scene needs
        reset() before it renders on.  Not while anything reads the scene's device copy."""
        if device is not None:
            def dev_ptr(t, words):
                if t is None:
                    return 0, None
                if t.dtype.itemsize != 4 or not t.is_contiguous() or t.numel() % words:
                    raise ValueError(f"update_triangles: a contiguous float32 tensor of n x {words} words is needed")
                return t.data_ptr(), t.numel() // words
            p_tri, n = dev_ptr(tri, 12)
            p_attr, na = dev_ptr(attr, 16)
            p_tan, nt = dev_ptr(tan, 12)
            if n is None or any(k is not None and k != n for k in (na, nt)):
                raise ValueError("update_triangles: tri is needed, and attr and tan must hold as many records")
            _check(lib().rt_scene_update_tris_device(self._h, int(device), int(first), n, ctypes.c_void_p(p_tri),
                                                     ctypes.c_void_p(p_attr), ctypes.c_void_p(p_tan),
                                                     ctypes.c_void_p(stream_ptr or 0)))
            return
        if tri is None:
            raise ValueError("update_triangles: tri is needed")
        tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 12)
        n = len(tri)
        attr = None if attr is None else np.ascontiguousarray(attr, np.float32).reshape(-1, 16)
        tan = None if tan is None else np.ascontiguousarray(tan, np.float32).reshape(-1, 12)
        if any(x is not None and len(x) != n for x in (attr, tan)):
            raise ValueError("update_triangles: attr and tan must hold as many records as tri")
        _check(lib().rt_scene_update_tris(self._h, int(first), n, tri.ctypes.data_as(_c_f),
                                          attr.ctypes.data_as(_c_f) if attr is not None else None,
                                          tan.ctypes.data_as(_c_f) if tan is not None else None))

    def enable_light_updates(self):
        """rt_scene_enable_light_updates: from now on update_triangles accepts triangles of emissive
        meshes and keeps the light list and the light BVH in step (csrc/rt_relight.h).  Idempotent;
        raises, and leaves the scene as it was, where the light list does not restate the emissive
        triangles one to one."""
        _check(lib().rt_scene_enable_light_updates(self._h))

    def light_map(self):
        """rt_scene_light_map: tri_of_light, the triangle each light restates (needs the opt-in)."""
        v = RtSceneView()
        _check(lib().rt_scene_get_view(self._h, ctypes.byref(v)))
        out = np.zeros(v.n_lights, np.uint32)
        _check(lib().rt_scene_light_map(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return out

    def read_device_lights(self, device=0):
        """rt_scene_read_device_lights (test / inspection): the device copy's light and light_node
        arrays, as a dict."""
        v = RtSceneView()
        _check(lib().rt_scene_get_view(self._h, ctypes.byref(v)))
        out = {"light": np.zeros((v.n_lights, 16), np.float32), "light_node": np.zeros((v.n_light_nodes, 8), np.float32)}
        _check(lib().rt_scene_read_device_lights(self._h, int(device), out["light"].ctypes.data_as(_c_f),
                                                 out["light_node"].ctypes.data_as(_c_f)))
        return out

    def _counts(self):
        v = RtSceneView()
        _check(lib().rt_scene_get_view(self._h, ctypes.byref(v)))
        return int(v.n_tris), int(v.n_meshes)

    def rest(self):
        """rt_scene_get_rest: {"rest": (n_tris, 18) object-space q0 q1 q2 n0 n1 n2 per triangle in post-build
        order, "tri_source": (n_tris,) the triangle's index in load order, "mesh_matrix": (n_meshes, 16) the
        meshes' current node matrices (column storage)}.  Raises (code ERR_STATE) on a scene without rest data."""
        nt, nm = self._counts()
        out = {"rest": np.zeros((nt, 18), np.float32), "tri_source": np.zeros(nt, np.uint32),
               "mesh_matrix": np.zeros((nm, 16), np.float64)}
        _check(lib().rt_scene_get_rest(self._h, out["rest"].ctypes.data_as(_c_f), out["tri_source"].ctypes.data_as(_c_u),
                                       out["mesh_matrix"].ctypes.data_as(_c_d)))
        return out

    def set_rest(self, rest, tri_source=None, mesh_matrix=None):
        """rt_scene_set_rest: hand a from_view scene the rest data of the load its arrays came from; `rest`
        may be the dict rest() returns."""
        if isinstance(rest, dict):
            rest, tri_source, mesh_matrix = rest["rest"], rest["tri_source"], rest["mesh_matrix"]
        nt, nm = self._counts()
        rest = np.ascontiguousarray(rest, np.float32).reshape(-1)
        src = np.ascontiguousarray(tri_source, np.uint32).reshape(-1)
        mm = np.ascontiguousarray(mesh_matrix, np.float64).reshape(-1)
        if len(rest) != 18 * nt or len(src) != nt or len(mm) != 16 * nm:
            raise ValueError("set_rest: rest (n_tris, 18), tri_source (n_tris,) and mesh_matrix (n_meshes, 16) are needed")
        _check(lib().rt_scene_set_rest(self._h, rest.ctypes.data_as(_c_f), src.ctypes.data_as(_c_u), mm.ctypes.data_as(_c_d)))

    def tri_source(self):
        """rt_scene_tri_source: for every triangle (post-build order) its index in load order."""
        out = np.zeros(self._counts()[0], np.uint32)
        _check(lib().rt_scene_tri_source(self._h, out.ctypes.data_as(_c_u)))
        return out

    def enable_poses(self):
        """rt_scene_enable_poses: from now on pose() may give meshes other node matrices; the rest records
        go to every device copy.  Idempotent; raises (code ERR_STATE), the scene untouched, without rest data."""
        _check(lib().rt_scene_enable_poses(self._h))

    def mesh_transform(self, mesh):
        """rt_scene_get_mesh_transform: the mesh's current node matrix, 16 doubles in column storage."""
        m = np.zeros(16, np.float64)
        _check(lib().rt_scene_get_mesh_transform(self._h, int(mesh), m.ctypes.data_as(_c_d)))
        return m

    def pose(self, poses):
        """rt_scene_pose_meshes: {mesh: M, ...}, M the mesh's whole node matrix (16 doubles, column
        storage; trs() makes one).  The records, the boxes, mesh_normal_transform and, for an emissive
        mesh on a scene with enable_light_updates(), the lights follow on the host and on every device
        copy (csrc/rt_pose.h); the tree's topology is kept.  An accumulator of the scene needs reset()
        before it renders on.  Not while anything reads the scene's device copy."""
        ids = np.array([int(k) for k in poses], np.uint32)
        if len(ids) and min(int(k) for k in poses) < 0:
            raise ValueError("pose: negative mesh id")
        m = np.ascontiguousarray([np.asarray(poses[k], np.float64).reshape(16) for k in poses], np.float64).reshape(-1)
        _check(lib().rt_scene_pose_meshes(self._h, len(ids), ids.ctypes.data_as(_c_u), m.ctypes.data_as(_c_d)))

    def translated_records(self, mesh, offset, cover=False, lights=False):
        """The easy way to move an object: [(first, tri), ...], one entry per run of consecutive
        triangles of `mesh`, with v0 + offset (one float32 add per component; U, V and the normals are
        unchanged), for update_triangles.  An emissive mesh is refused (lights do not move) unless
        lights=True, which needs enable_light_updates() and then also lets a covering range run through
        emissive triangles.
        cover=True: the post-build order scatters a mesh's triangles and every update refits the whole
        tree, so the entries are instead the range from the mesh's first to its last triangle, cut only
        at emissive triangles, with the other meshes' records in between as the scene holds them: the
        same result in far fewer calls."""
        v = self.view()
        mesh = int(mesh)
        if not 0 <= mesh < len(v["mesh_f"]):
            raise ValueError(f"translated_records: no mesh {mesh}")
        if lights:
            self.light_map()   # (raises before the opt-in)
        elif np.any(v["mesh_f"][mesh, 3:6] != 0):
            raise ValueError(f"translated_records: mesh {mesh} is emissive; moving lights are not supported")
        ids = np.flatnonzero(v["tri_attr"][:, 15].view(np.int32) == mesh)
        off = np.asarray(offset, np.float32).reshape(3)
        mesh_of = v["tri_attr"][:, 15].view(np.int32)
        mine = mesh_of == mesh
        moved = v["tri"].copy()
        moved[mine, 0:3] = moved[mine, 0:3] + off
        if cover and len(ids):
            lit = np.any(v["mesh_f"][:, 3:6] != 0, axis=1)[mesh_of]
            span = np.arange(ids[0], ids[-1] + 1)
            ids = span if lights else span[~lit[span]]
        return [(int(run[0]), moved[run]) for run in np.split(ids, np.flatnonzero(np.diff(ids) != 1) + 1)] if len(ids) else []

    def read_device(self, device=0):
        """rt_scene_read_device (test / inspection): the device copy's tri, tri_attr, tri_tan and node
        arrays in the host layout (nodes in build order), as a dict."""
        v = RtSceneView()
        _check(lib().rt_scene_get_view(self._h, ctypes.byref(v)))
        out = {"tri": np.zeros((v.n_tris, 12), np.float32), "tri_attr": np.zeros((v.n_tris, 16), np.float32),
               "tri_tan": np.zeros((v.n_tris, 12), np.float32), "node": np.zeros((v.n_nodes, 8), np.float32)}
        _check(lib().rt_scene_read_device(self._h, int(device), *[out[k].ctypes.data_as(_c_f)
                                                                  for k in ("tri", "tri_attr", "tri_tan", "node")]))
        return out

    def history(self, device=0, motion=False):
        """rt_history_create: a reprojected temporal history of this scene's frame on `device`
        (uploaded here if need be).  motion=True: rt_history_enable_motion, the history follows
        triangles that update_triangles moved between two pushes."""
        self.upload(device)
        h = ctypes.c_void_p()
        _check(lib().rt_history_create(self._h, device, ctypes.byref(h)))
        hist = History(self, h.value)
        if motion:
            hist.enable_motion()
        return hist

    def upload(self, device=0):
        _check(lib().rt_scene_upload(self._h, device))

    def _params(self, spp, rank, world, row_block, count, kernel, kernel_times=False, fast=False, fast_chunk=0,
                device=0, light_split=False, natural_order=False, runahead=True, heavy_order=False):
        flags = ((FLAG_KERNEL_TIMES if kernel_times else 0) | (FLAG_FAST if fast else 0) |
                 (FLAG_LIGHT_SPLIT if light_split else 0) | (FLAG_NATURAL_ORDER if natural_order else 0) |
                 (0 if runahead else FLAG_NO_RUNAHEAD) | (FLAG_HEAVY_ORDER if heavy_order else 0))
        return RtParams(spp or 0, rank, world, row_block, int(count), kernel, flags, fast_chunk, device)

    def render_sums(self, spp=None, rank=0, world=1, row_block=8, count=False, kernel=0, device=0, fast=False,
                    fast_chunk=0, light_split=False, natural_order=False, runahead=True, heavy_order=False):
        """Per-pixel float RGB sums of the owned rows (sample_canvas, scene.cpp:20,42).
        fast=True: fast mode (RT_FLAG_FAST, work units of fast_chunk samples): statistically
        equivalent to the reference, not bit-identical.  light_split / natural_order /
        heavy_order / runahead=False: other schedules of the same bits (RT_FLAG_LIGHT_SPLIT,
        RT_FLAG_NATURAL_ORDER, RT_FLAG_HEAVY_ORDER, RT_FLAG_NO_RUNAHEAD)."""
        rows = shard_rows(self.height, rank, world, row_block)
        out = np.zeros((len(rows), self.width, 3), np.float32)
        st = RtStats()
        p = self._params(spp, rank, world, row_block, count, kernel, fast=fast, fast_chunk=fast_chunk, device=device,
                         light_split=light_split, natural_order=natural_order, runahead=runahead,
                         heavy_order=heavy_order)
        _check(lib().rt_render(self._h, ctypes.byref(p), out.ctypes.data_as(_c_f), ctypes.byref(st)))
        _after_render()
        return out, st.as_dict()

    def render_multi(self, spp=None, n_devices=0, row_block=8, count=False, kernel=0, fast=False, fast_chunk=0):
        """The whole frame over devices 0..n_devices-1 (0 = all visible; rt_render_multi):
        one host thread per device, each rendering its row-block shard; (H, W, 3) sums."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        st = RtStats()
        p = self._params(spp, 0, 1, row_block, count, kernel, fast=fast, fast_chunk=fast_chunk)
        _check(lib().rt_render_multi(self._h, ctypes.byref(p), n_devices, out.ctypes.data_as(_c_f), ctypes.byref(st)))
        _after_render()
        return out, st.as_dict()

    def render_frame(self, spp=None, n_shards=0, devices=None, row_block=8, sums=True, rgb=True, kernel=0,
                     fast=False, fast_chunk=0, runahead=True):
        """The whole frame as shards 0..n_shards-1 (0 = one per visible device), shard r on
        device devices[r] (None: device r; rt_render_frame): each shard is finished to 8 bits
        on its device and gathered device-to-device onto devices[0].  Returns (rgb (H, W, 3)
        uint8 or None, sums (H, W, 3) float32 or None, stats)."""
        out_rgb = np.zeros((self.height, self.width, 3), np.uint8) if rgb else None
        out_sum = np.zeros((self.height, self.width, 3), np.float32) if sums else None
        dev = None
        if devices is not None:
            dev = np.ascontiguousarray(devices, np.int32)
            if n_shards and len(dev) != n_shards:
                raise ValueError("devices must name one device per shard")
            n_shards = len(dev)
        st = RtStats()
        p = self._params(spp, 0, 1, row_block, False, kernel, fast=fast, fast_chunk=fast_chunk, runahead=runahead)
        _check(lib().rt_render_frame(self._h, ctypes.byref(p), n_shards,
                                     dev.ctypes.data_as(_c_i) if dev is not None else None,
                                     out_rgb.ctypes.data_as(_c_b) if rgb else None,
                                     out_sum.ctypes.data_as(_c_f) if sums else None, ctypes.byref(st)))
        _after_render()
        return out_rgb, out_sum, st.as_dict()

    def render_device(self, d_out_ptr, stream_ptr=None, spp=None, rank=0, world=1, row_block=8, count=False,
                      kernel=0, stats=False, kernel_times=False, fast=False, fast_chunk=0, device=0,
                      light_split=False, natural_order=False, runahead=True, heavy_order=False):
        """Launch into device memory (e.g. a torch tensor's data_ptr()) on a HIP stream, on
        `device` (upload(device) first).  kernel_times: per-launch HIP-event timing of the
        wavefront kernels (needs stats).  fast: fast mode (RT_FLAG_FAST), see render_sums."""
        p = self._params(spp, rank, world, row_block, count, kernel, kernel_times, fast, fast_chunk, device,
                         light_split, natural_order, runahead, heavy_order)
        st = RtStats() if stats else None
        _check(lib().rt_render_device(self._h, ctypes.byref(p), ctypes.c_void_p(d_out_ptr),
                                      ctypes.c_void_p(stream_ptr or 0), ctypes.byref(st) if st else None))
        _after_render()
        return st.as_dict() if st else None

    def gbuffer(self, rank=0, world=1, row_block=8, device=0):
        """rt_gbuffer: the shard's first-hit records from the pixel-centre rays, as a dict of
        (rows, W[, 3]) arrays: normal, depth (hit distance), albedo, emission, position (float32),
        prim and mesh (int32, -1 on a miss).  See gbuffer_unpack / gbuffer_pack for the records."""
        rows = shard_rows(self.height, rank, world, row_block)
        rec = np.zeros((len(rows), self.width, GBUFFER_WORDS), np.float32)
        p = self._params(0, rank, world, row_block, False, KERNEL_LANE, device=device)
        _check(lib().rt_gbuffer(self._h, ctypes.byref(p), rec.ctypes.data_as(_c_f)))
        return gbuffer_unpack(rec)

    def gbuffer_device(self, d_out_ptr, stream_ptr=None, rank=0, world=1, row_block=8, device=0):
        """rt_gbuffer_device: the same records into device memory (pixels x 16 floats) on a HIP
        stream; upload(device) first."""
        p = self._params(0, rank, world, row_block, False, KERNEL_LANE, device=device)
        _check(lib().rt_gbuffer_device(self._h, ctypes.byref(p), ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(stream_ptr or 0)))

    def accumulator(self, rank=0, world=1, row_block=8, device=0, natural_order=False, heavy_order=False,
                    runahead=True, fast=False, fast_chunk=0, moments=False):
        """Progressive rendering (rt_accum_create): the shard's per-pixel chain state on
        `device` (uploaded here if need be), rendered further in passes of any size; after
        passes of n1 + ... + nk samples the sums are those of render_sums(n1 + ... + nk), bit
        for bit.  fast=True (rt_accum_create_fast): a fast-mode accumulator with chunks of
        fast_chunk samples (0 = 2), fixed for its life; a pixel with n samples then holds the
        fast sum of n samples in chunks of that size, whatever the passes were.  moments=True
        (with fast; rt_accum_create_fast_moments): it also keeps the sum of every sample's squared
        colour (moments(), variance(), select_variance(), frame(measured=True))."""
        if moments and not fast:
            raise ValueError("moments=True needs fast=True (only fast-mode accumulators keep moments)")
        self.upload(device)
        p = self._params(0, rank, world, row_block, False, KERNEL_LANE, device=device, natural_order=natural_order,
                         runahead=runahead, heavy_order=heavy_order, fast=fast, fast_chunk=fast_chunk if fast else 0)
        h = ctypes.c_void_p()
        create = lib().rt_accum_create_fast_moments if moments else lib().rt_accum_create_fast if fast else lib().rt_accum_create
        _check(create(self._h, ctypes.byref(p), ctypes.byref(h)))
        return Accumulator(self, h.value, rank, world, row_block)

    def render_adaptive(self, min_spp, max_spp, step, threshold, device=0, fast=False, fast_chunk=0, moments=False):
        """Adaptive sampling of the whole frame on one shard (the loop of the CLI's RT_ADAPT):
        min_spp samples everywhere in two halves with a mark between them, then rounds of
        select(target = min(max_spp, largest count + step), threshold), mark, add_selected until
        nothing is selected or max_spp is reached.  Returns (sums (H, W, 3), counts (H, W),
        frame (H, W, 3) uint8 finished per pixel by its own count).  fast / fast_chunk: on a
        fast-mode accumulator (see accumulator).  moments (with fast): on a moments accumulator,
        min_spp samples in one pass and then rounds of select_variance, add_selected, with no mark."""
        if min_spp < 2 or max_spp < min_spp or step < 1:
            raise ValueError("render_adaptive: need 2 <= min_spp <= max_spp and step >= 1")
        acc = self.accumulator(device=device, fast=fast, fast_chunk=fast_chunk, moments=moments)
        try:
            if moments:
                acc.add(min_spp)
                while acc.samples < max_spp:
                    target = min(max_spp, acc.samples + step)
                    if acc.select_variance(target, threshold=threshold) == 0:
                        break
                    acc.add_selected()
                return acc.sums(), acc.counts(), acc.frame()
            acc.add(min_spp // 2)
            acc.mark()
            acc.add(min_spp - min_spp // 2)
            while acc.samples < max_spp:
                target = min(max_spp, acc.samples + step)
                if acc.select(target, threshold=threshold) == 0:
                    break
                acc.mark()
                acc.add_selected()
            return acc.sums(), acc.counts(), acc.frame()
        finally:
            acc.free()

    def render(self):
        """Scene::render (scene.cpp:17-65): sample loop on the GPU, then the 8-bit frame finish."""
        sums, _ = self.render_sums(self.samples)
        self.canvas = tonemap(sums, self.samples)
        return self.canvas

    def draw_into(self, filename):
        if self.canvas is None:
            raise RtError("render() first")
        write_ppm(filename, self.canvas)


class Accumulator:
    """A shard's chain state between passes (include/rt_hw.h rt_accum): add(n) renders the
    next n samples of every owned pixel; sums() / frame() are the shard so far."""

    def __init__(self, scene, handle, rank, world, row_block):
        self._scene = scene   # (kept alive: the accumulator is freed before its scene)
        self._h = ctypes.c_void_p(handle)
        self.rank, self.world, self.row_block = rank, world, row_block
        self.rows = shard_rows(scene.height, rank, world, row_block)

    @classmethod
    def load(cls, scene, path, device=0):
        """rt_accum_load: the accumulator rt_accum_save wrote (of any of the three kinds: see
        fast_chunk and has_moments), checked against `scene`."""
        h = ctypes.c_void_p()
        _check(lib().rt_accum_load(scene.handle, device, os.fsencode(path), ctypes.byref(h)))
        with open(path, "rb") as f:   # rank, world, row_block: int32 words 6-8 of the header
            hdr = np.frombuffer(f.read(36), np.int32)
        return cls(scene, h.value, int(hdr[6]), int(hdr[7]), int(hdr[8]))

    def add(self, n, stats=True, stream_ptr=None):
        """Render samples [samples, samples + n) (rt_accum_add); returns the pass's stats
        (waits), or None with stats=False (asynchronous on the stream)."""
        st = RtStats() if stats else None
        _check(lib().rt_accum_add(self._h, int(n), ctypes.c_void_p(stream_ptr or 0), ctypes.byref(st) if st else None))
        _after_render()
        return st.as_dict() if st else None

    @property
    def samples(self):
        return int(lib().rt_accum_samples(self._h))

    @property
    def fast_chunk(self):
        """The chunk size of a fast-mode accumulator (rt_accum_fast_chunk); 0 for a parity one."""
        return int(lib().rt_accum_fast_chunk(self._h))

    @property
    def has_moments(self):
        """True for a moments accumulator (rt_accum_has_moments)."""
        return bool(lib().rt_accum_has_moments(self._h))

    def moments(self):
        """(rows, W, 3) float32: per pixel the sum of its samples' squared colours, folded as the
        sums are (rt_accum_moments; a moments accumulator only)."""
        out = np.zeros((len(self.rows), self._scene.width, 3), np.float32)
        _check(lib().rt_accum_moments(self._h, out.ctypes.data_as(_c_f)))
        return out

    @property
    def device_moments_ptr(self):
        return int(lib().rt_accum_device_moments(self._h) or 0)

    def variance(self):
        """(rows, W) float32: the measured variance of each owned pixel's demodulated mean
        (rt_accum_variance), the `variance` input of denoise_guided."""
        out = np.zeros((len(self.rows), self._scene.width), np.float32)
        _check(lib().rt_accum_variance(self._h, out.ctypes.data_as(_c_f)))
        return out

    def sums(self):
        """(rows, W, 3) float sums so far, as render_sums returns them."""
        out = np.zeros((len(self.rows), self._scene.width, 3), np.float32)
        _check(lib().rt_accum_sums(self._h, out.ctypes.data_as(_c_f)))
        return out

    @property
    def device_sums_ptr(self):
        return int(lib().rt_accum_device_sums(self._h) or 0)

    def frame(self, denoise=None, guided=False, measured=False):
        """(rows, W, 3) uint8: the shard finished at spp = samples (on the device).  denoise: True
        (the default parameters) or a dict of denoise_params' arguments runs the frame denoiser in
        front of the finish (rt_accum_frame_u8_denoised; whole-frame accumulators only).  guided:
        with denoise, the variance-guided mode (rt_accum_frame_u8_guided; the dict then holds
        denoise_guided_params' arguments).  measured: with guided, the filter's variance input is
        the accumulator's measured variance (rt_accum_frame_u8_guided_measured; a moments
        accumulator only)."""
        out = np.zeros((len(self.rows), self._scene.width, 3), np.uint8)
        if measured and not guided:
            raise ValueError("measured=True needs guided=True")
        if denoise is None or denoise is False:
            if guided:
                raise ValueError("guided=True needs denoise=True or a dict of denoise_guided_params' arguments")
            _check(lib().rt_accum_frame_u8(self._h, out.ctypes.data_as(_c_b)))
        elif guided:
            gp = denoise_guided_params(**(denoise if isinstance(denoise, dict) else {}))
            entry = lib().rt_accum_frame_u8_guided_measured if measured else lib().rt_accum_frame_u8_guided
            _check(entry(self._h, ctypes.byref(gp), out.ctypes.data_as(_c_b)))
        else:
            dp = denoise_params(**(denoise if isinstance(denoise, dict) else {}))
            _check(lib().rt_accum_frame_u8_denoised(self._h, ctypes.byref(dp), out.ctypes.data_as(_c_b)))
        return out

    def state(self):
        """(pixels, 4) uint32 per shard pixel: next sample, engine state, cache flag, cached value bits
        (a fast-mode accumulator: next sample and the three words of the open chunk's partial)."""
        out = np.zeros((len(self.rows) * self._scene.width, 4), np.uint32)
        _check(lib().rt_accum_state(self._h, out.ctypes.data_as(_c_u)))
        return out

    def save(self, path):
        _check(lib().rt_accum_save(self._h, os.fsencode(path)))

    def reset(self, stream_ptr=None):
        """rt_accum_reset: back to the state after creation, on the scene's camera as it now stands
        (what an accumulator needs after Scene.set_camera before it renders on)."""
        _check(lib().rt_accum_reset(self._h, ctypes.c_void_p(stream_ptr or 0)))
        self._n_selected = 0

    # --- per-pixel sample counts (include/rt_hw.h rt_accum_select and friends)
    def mark(self, stream_ptr=None):
        """rt_accum_mark: remember the sums and counts as they stand (the selection rule's
        "before" half).  A pending selection stays."""
        _check(lib().rt_accum_mark(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def select(self, target, window=None, mask=None, threshold=0.0, stream_ptr=None):
        """rt_accum_select: choose the pixels the next add_selected() raises to `target` samples:
        those below it, inside window = (x0, y0, x1, y1) (frame coordinates, half-open), with a
        non-zero byte in mask ((rows, W), the shard's layout) and, with threshold > 0, whose
        error estimate since the last mark exceeds it.  Returns how many were selected."""
        return self._select(lib().rt_accum_select, target, window, mask, threshold, stream_ptr)

    def select_variance(self, target, window=None, mask=None, threshold=0.0, stream_ptr=None):
        """rt_accum_select_variance (a moments accumulator only): select() with the error test
        replaced by the relative standard error of the pixel's mean, from its moments: a pixel
        with fewer than 2 samples is selected, any other iff that error exceeds threshold.  It
        needs no mark and ignores one."""
        return self._select(lib().rt_accum_select_variance, target, window, mask, threshold, stream_ptr)

    def _select(self, entry, target, window, mask, threshold, stream_ptr):
        x0, y0, x1, y1 = window if window is not None else (0, 0, 0, 0)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8).reshape(-1)
            if m.size != len(self.rows) * self._scene.width:
                raise ValueError("mask must have one byte per owned pixel")
        sel = RtSelect(int(target), int(x0), int(y0), int(x1), int(y1), m.ctypes.data_as(_c_b) if m is not None else None,
                       float(threshold))
        n = ctypes.c_int64(0)
        _check(entry(self._h, ctypes.byref(sel), ctypes.c_void_p(stream_ptr or 0), ctypes.byref(n)))
        self._n_selected = int(n.value)
        return self._n_selected

    def selection(self):
        """The pending list: shard pixels, ascending (test / inspection)."""
        out = np.zeros(max(getattr(self, "_n_selected", 0), 1), np.int32)
        _check(lib().rt_accum_selection(self._h, out.ctypes.data_as(_c_i)))
        return out[:self._n_selected]

    def add_selected(self, stats=True, stream_ptr=None):
        """rt_accum_add_selected: render the pending list's pixels up to its target; returns the
        pass's stats (waits), or None with stats=False."""
        st = RtStats() if stats else None
        _check(lib().rt_accum_add_selected(self._h, ctypes.c_void_p(stream_ptr or 0), ctypes.byref(st) if st else None))
        self._n_selected = 0
        _after_render()
        return st.as_dict() if st else None

    def counts(self):
        """(rows, W) int32: every owned pixel's sample count."""
        out = np.zeros((len(self.rows), self._scene.width), np.int32)
        _check(lib().rt_accum_counts(self._h, out.ctypes.data_as(_c_i)))
        return out

    @property
    def sample_range(self):
        """(smallest, largest) sample count."""
        lo, hi = ctypes.c_int32(0), ctypes.c_int32(0)
        _check(lib().rt_accum_sample_range(self._h, ctypes.byref(lo), ctypes.byref(hi)))
        return int(lo.value), int(hi.value)

    def free(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib_handle is not None:
            _lib_handle.rt_accum_free(h)
        self._h = None

    def __del__(self):
        self.free()


class History:
    """A reprojected temporal history (include/rt_hw.h rt_history): push() renders the scene's
    G-buffer at its current camera and blends the frame's sums with the previous push's result."""

    def __init__(self, scene, handle):
        self._scene = scene   # (kept alive: the history is freed before its scene)
        self._h = ctypes.c_void_p(handle)

    def push(self, d_sums_ptr, d_counts_ptr, spp, d_out_ptr, d_var_ptr=0, stream_ptr=None, **params):
        """rt_history_push: device pointers (d_counts_ptr 0 / None: one spp; d_out_ptr, d_var_ptr 0 /
        None: not wanted), asynchronous on the stream.  params: temporal_params' arguments."""
        tp = temporal_params(**params)
        _check(lib().rt_history_push(self._h, ctypes.c_void_p(d_sums_ptr), ctypes.c_void_p(d_counts_ptr or 0), int(spp),
                                     ctypes.byref(tp), ctypes.c_void_p(d_out_ptr or 0), ctypes.c_void_p(d_var_ptr or 0),
                                     ctypes.c_void_p(stream_ptr or 0)))

    def push_accumulator(self, acc, d_out_ptr, d_var_ptr=0, stream_ptr=None, d_counts_ptr=0, **params):
        """push() of a whole-frame accumulator's device sums and counts.  While every pixel holds one
        sample count that count is the spp; after subset passes d_counts_ptr must name a device
        buffer of H * W int32, which receives the count map (rt_accum_counts_device) on the stream."""
        lo, hi = acc.sample_range
        if acc.world != 1:
            raise ValueError("push_accumulator needs a whole-frame accumulator (world = 1)")
        if lo != hi and not d_counts_ptr:
            raise ValueError("the pixels hold different sample counts: pass d_counts_ptr, a device buffer for the count map")
        if lo != hi:
            _check(lib().rt_accum_counts_device(acc._h, ctypes.c_void_p(d_counts_ptr), ctypes.c_void_p(stream_ptr or 0)))
        self.push(acc.device_sums_ptr, d_counts_ptr if lo != hi else 0, hi, d_out_ptr, d_var_ptr, stream_ptr, **params)

    def push_frame_u8(self, sums, counts_or_spp, denoise=None, guided=False, **params):
        """rt_history_push_frame_u8: host sums in, the pushed frame's (H, W, 3) bytes out (waits).
        denoise: True or a dict of the filter's parameters runs rt_denoise_device on the integrated
        mean, with guided=True the guided mode with the step's variance.  params: temporal_params'."""
        sums = np.ascontiguousarray(sums, np.float32)
        h, w = self._scene.height, self._scene.width
        if sums.size != h * w * 3:
            raise ValueError("sums must be the scene's (H, W, 3) frame")
        counts, spp = None, 0
        if np.ndim(counts_or_spp) == 0:
            spp = int(counts_or_spp)
        else:
            counts = np.ascontiguousarray(counts_or_spp, np.int32)
        tp = temporal_params(**params)
        kw = denoise if isinstance(denoise, dict) else {}
        dp = denoise_params(**kw) if denoise and not guided else None
        gp = denoise_guided_params(**kw) if denoise and guided else None
        rgb = np.zeros((h, w, 3), np.uint8)
        _check(lib().rt_history_push_frame_u8(self._h, sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None,
                                              spp, ctypes.byref(tp), ctypes.byref(dp) if dp is not None else None,
                                              ctypes.byref(gp) if gp is not None else None, rgb.ctypes.data_as(_c_b)))
        return rgb

    def lengths(self):
        """(H, W) float32: every pixel's history length in frames (waits)."""
        out = np.zeros((self._scene.height, self._scene.width), np.float32)
        _check(lib().rt_history_lengths(self._h, out.ctypes.data_as(_c_f)))
        return out

    def gbuffer_ptr(self):
        """The device records of the last push's view (0 before one), for denoise*_device."""
        return int(lib().rt_history_gbuffer_device(self._h) or 0)

    def enable_motion(self):
        """rt_history_enable_motion: before the first push or directly after reset()."""
        _check(lib().rt_history_enable_motion(self._h))

    def motion_ptr(self):
        """The device motion plane of the last push (0 when it ran without one)."""
        return int(lib().rt_history_motion_device(self._h) or 0)

    def motion(self):
        """The last push's motion records on the host, as motion() returns them, or None when that
        push ran without them (waits for the device)."""
        ptr = self.motion_ptr()
        if not ptr:
            return None
        h, w = self._scene.height, self._scene.width
        out = np.zeros((h, w, MOTION_WORDS), np.float32)
        _check(lib().rt_history_motion(self._h, out.ctypes.data_as(_c_f)))
        return motion_unpack(out)

    def reset(self):
        _check(lib().rt_history_reset(self._h))

    def free(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib_handle is not None:
            _lib_handle.rt_history_free(h)
        self._h = None

    def __del__(self):
        self.free()


def make_view(a):
    """Build an RtSceneView over numpy arrays (dict layout of Scene.view()); returns (view, keepalive)."""
    keep = {}

    def ptr(name, dtype, ctype):
        arr = np.ascontiguousarray(a[name], dtype).reshape(-1)
        if arr.size == 0:
            arr = np.zeros(1, dtype)
        keep[name] = arr
        return arr.ctypes.data_as(ctype)

    v = RtSceneView()
    v.width, v.height, v.samples, v.ray_depth = int(a["width"]), int(a["height"]), int(a["samples"]), int(a["ray_depth"])
    v.max_distance = float(a["max_distance"])
    v.cam_pos[:] = [float(x) for x in np.asarray(a["cam_pos"], np.float32)]
    v.cam_axes[:] = [float(x) for x in np.asarray(a["cam_axes"], np.float32).reshape(-1)]
    v.cam_fov[:] = [float(x) for x in np.asarray(a["cam_fov"], np.float32)]
    v.tan_half_fov[:] = [float(x) for x in np.asarray(a["tan_half_fov"], np.float32)]
    v.n_tris = len(a["tri"])
    v.tri, v.tri_attr, v.tri_tan = ptr("tri", np.float32, _c_f), ptr("tri_attr", np.float32, _c_f), ptr("tri_tan", np.float32, _c_f)
    v.n_nodes, v.node = len(a["node"]), ptr("node", np.float32, _c_f)
    v.bvh_depth = int(a.get("bvh_depth", 0))
    v.n_lights, v.light = len(a["light"]), ptr("light", np.float32, _c_f)
    v.n_light_nodes, v.light_node = len(a["light_node"]), ptr("light_node", np.float32, _c_f)
    v.light_bvh_depth = int(a.get("light_bvh_depth", 0))
    v.n_meshes = len(a["mesh_f"])
    v.mesh_f, v.mesh_tex = ptr("mesh_f", np.float32, _c_f), ptr("mesh_tex", np.int32, _c_i)
    v.mesh_normal_transform = ptr("mesh_normal_transform", np.float64, _c_d)
    v.n_textures, v.tex_info = len(a["tex_info"]), ptr("tex_info", np.uint32, _c_u)
    v.texels, v.n_texel_bytes = ptr("texels", np.uint8, _c_b), int(np.asarray(a["texels"]).size)
    return v, keep


def refit_view(arrays):
    """rt_refit_view (a pure host function): the (n_nodes, 8) node array of the view's topology with
    every box recomputed from its triangles by the refit rule (csrc/rt_refit.h); a and b copied."""
    v, keep = make_view(arrays)
    out = np.zeros((len(arrays["node"]), 8), np.float32)
    _check(lib().rt_refit_view(ctypes.byref(v), out.ctypes.data_as(_c_f)))
    del keep
    return out


def relight_view(arrays, tri_of_light):
    """rt_relight_view (a pure host function): (light, light_node) of the view with words 0..12 of every
    light restated from triangle tri_of_light[k] and every light box recomputed (csrc/rt_relight.h);
    words 13..15, a and b copied."""
    v, keep = make_view(arrays)
    tl = np.ascontiguousarray(tri_of_light, np.uint32)
    if len(tl) != len(arrays["light"]):
        raise ValueError("relight_view: tri_of_light must hold one triangle per light")
    light = np.zeros((len(arrays["light"]), 16), np.float32)
    lnode = np.zeros((len(arrays["light_node"]), 8), np.float32)
    _check(lib().rt_relight_view(ctypes.byref(v), tl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                 light.ctypes.data_as(_c_f), lnode.ctypes.data_as(_c_f)))
    del keep
    return light, lnode


def pose_view(arrays, rest, poses):
    """rt_pose_view (a pure host function): (tri, tri_attr, mesh_normal_transform) of the view with the
    meshes of `poses` ({mesh: M}) under their matrices (csrc/rt_pose.h); rest is (n_tris, 18).  Words
    9..15 of tri_attr and every other mesh's records are copied."""
    v, keep = make_view(arrays)
    nt, nm = len(arrays["tri"]), len(arrays["mesh_f"])
    rest = np.ascontiguousarray(rest, np.float32).reshape(-1)
    if len(rest) != 18 * nt:
        raise ValueError("pose_view: rest must hold 18 words per triangle")
    ids = np.array([int(k) for k in poses], np.uint32)
    m = np.ascontiguousarray([np.asarray(poses[k], np.float64).reshape(16) for k in poses], np.float64).reshape(-1)
    tri = np.zeros((nt, 12), np.float32)
    attr = np.zeros((nt, 16), np.float32)
    mnt = np.zeros((nm, 16), np.float64)
    _check(lib().rt_pose_view(ctypes.byref(v), rest.ctypes.data_as(_c_f), len(ids), ids.ctypes.data_as(_c_u),
                              m.ctypes.data_as(_c_d), tri.ctypes.data_as(_c_f), attr.ctypes.data_as(_c_f),
                              mnt.ctypes.data_as(_c_d)))
    del keep
    return tri, attr, mnt


def trs(t=(0, 0, 0), r=(0, 0, 0, 1), s=(1, 1, 1)):
    """rt_trs_matrix: the node matrix the loader makes of a glTF translation, rotation (quaternion
    x y z w) and scale (float32 arithmetic, stored to double): 16 doubles in column storage."""
    t, r, s = (np.ascontiguousarray(x, np.float32).reshape(k) for x, k in ((t, 3), (r, 4), (s, 3)))
    out = np.zeros(16, np.float64)
    _check(lib().rt_trs_matrix(t.ctypes.data_as(_c_f), r.ctypes.data_as(_c_f), s.ctypes.data_as(_c_f), out.ctypes.data_as(_c_d)))
    return out


def parse_scene_gltf(path, width, height, samples):
    return Scene.load(path, width, height, samples)


def tonemap(sums, spp):
    sums = np.ascontiguousarray(sums, np.float32)
    h, w = sums.shape[0], sums.shape[1]
    rgb = np.zeros((h, w, 3), np.uint8)
    _check(lib().rt_tonemap_u8(sums.ctypes.data_as(_c_f), w, h, spp, rgb.ctypes.data_as(_c_b)))
    return rgb


def tonemap_counts(sums, counts):
    """rt_tonemap_u8_counts: the frame finish with a per-pixel sample count (0 samples: black)."""
    sums = np.ascontiguousarray(sums, np.float32)
    h, w = sums.shape[0], sums.shape[1]
    counts = np.ascontiguousarray(counts, np.int32)
    if counts.size != h * w:
        raise ValueError("counts must have one entry per pixel")
    rgb = np.zeros((h, w, 3), np.uint8)
    _check(lib().rt_tonemap_u8_counts(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i), w, h, rgb.ctypes.data_as(_c_b)))
    return rgb


def gbuffer_unpack(records):
    """First-hit records (..., 16) float32 as the dict Scene.gbuffer returns ("records": the input)."""
    rec = np.ascontiguousarray(records, np.float32)
    ids = rec.view(np.int32)
    return {"normal": rec[..., 0:3].copy(), "depth": rec[..., 3].copy(), "albedo": rec[..., 4:7].copy(),
            "prim": ids[..., 7].copy(), "emission": rec[..., 8:11].copy(), "mesh": ids[..., 11].copy(),
            "position": rec[..., 12:15].copy(), "records": rec}


def gbuffer_pack(g):
    """The (H, W, 16) float32 records of a Scene.gbuffer dict (or of an array of records)."""
    if not isinstance(g, dict):
        return np.ascontiguousarray(g, np.float32)
    if "records" in g:
        return np.ascontiguousarray(g["records"], np.float32)
    n = np.asarray(g["normal"], np.float32)
    rec = np.zeros(n.shape[:-1] + (GBUFFER_WORDS,), np.float32)
    rec[..., 0:3], rec[..., 3] = n, g["depth"]
    rec[..., 4:7], rec[..., 8:11], rec[..., 12:15] = g["albedo"], g["emission"], g["position"]
    rec.view(np.int32)[..., 7] = g["prim"]
    rec.view(np.int32)[..., 11] = g["mesh"]
    return rec


def denoise(sums, counts_or_spp, gbuffer, **params):
    """rt_denoise (the host function): the (H, W, 3) float32 mean frame of the whole frame's sums,
    filtered by the edge-avoiding a-trous filter its G-buffer guides.  counts_or_spp: an (H, W)
    array of per-pixel sample counts, or one spp.  params: denoise_params' arguments."""
    sums, counts, spp, rec = _denoise_inputs(sums, counts_or_spp, gbuffer)
    h, w = sums.shape[0], sums.shape[1]
    out = np.zeros((h, w, 3), np.float32)
    dp = denoise_params(**params)
    _check(lib().rt_denoise(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None, spp, w, h,
                            rec.ctypes.data_as(_c_f), ctypes.byref(dp), out.ctypes.data_as(_c_f)))
    return out


def _denoise_inputs(sums, counts_or_spp, gbuffer):
    sums = np.ascontiguousarray(sums, np.float32)
    h, w = sums.shape[0], sums.shape[1]
    rec = gbuffer_pack(gbuffer)
    if rec.size != h * w * GBUFFER_WORDS:
        raise ValueError("gbuffer must have one record per pixel")
    counts, spp = None, 0
    if np.ndim(counts_or_spp) == 0:
        spp = int(counts_or_spp)
    else:
        counts = np.ascontiguousarray(counts_or_spp, np.int32)
        if counts.size != h * w:
            raise ValueError("counts must have one entry per pixel")
    return sums, counts, spp, rec


def denoise_frame_u8(sums, counts_or_spp, gbuffer, device=0, **params):
    """rt_denoise_frame_u8: host arrays in, the denoised frame's (H, W, 3) bytes out, filtered and
    finished on `device`."""
    sums, counts, spp, rec = _denoise_inputs(sums, counts_or_spp, gbuffer)
    h, w = sums.shape[0], sums.shape[1]
    rgb = np.zeros((h, w, 3), np.uint8)
    dp = denoise_params(**params)
    _check(lib().rt_denoise_frame_u8(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None, spp,
                                     w, h, rec.ctypes.data_as(_c_f), ctypes.byref(dp), device, rgb.ctypes.data_as(_c_b)))
    return rgb


def denoise_device(d_sums_ptr, d_counts_ptr, spp, width, height, d_gbuffer_ptr, d_out_ptr, stream_ptr=None, **params):
    """rt_denoise_device: the same filter on the current HIP device (device pointers, e.g. torch
    tensors; d_counts_ptr 0 / None: one spp), asynchronous on the stream."""
    dp = denoise_params(**params)
    _check(lib().rt_denoise_device(ctypes.c_void_p(d_sums_ptr), ctypes.c_void_p(d_counts_ptr or 0), int(spp), width, height,
                                   ctypes.c_void_p(d_gbuffer_ptr), ctypes.byref(dp), ctypes.c_void_p(d_out_ptr),
                                   ctypes.c_void_p(stream_ptr or 0)))


def motion_unpack(records):
    """(H, W, 8) motion records as a dict: prev_position, prev_normal (H, W, 3) and state (H, W) int32."""
    rec = np.ascontiguousarray(records, np.float32)
    return {"prev_position": rec[..., 0:3].copy(), "prev_normal": rec[..., 4:7].copy(),
            "state": rec.view(np.int32)[..., 3].copy(), "records": rec}


def _motion_arg(motion, h, w):
    if motion is None:
        return None
    rec = np.ascontiguousarray(motion["records"] if isinstance(motion, dict) else motion, np.float32)
    if rec.size != h * w * MOTION_WORDS:
        raise ValueError("motion must have two quads per pixel")
    return rec


def motion(gbuffer, tri, tri_prev):
    """rt_motion (the host function): every pixel's motion record from its first-hit record, the
    triangles as they stand (n x 12) and as they stood.  Returns a dict: prev_position, prev_normal,
    state (0 static, 1 carried, 2 lost) and the packed (H, W, 8) `records` temporal(motion=) takes."""
    rec = gbuffer_pack(gbuffer)
    if rec.ndim != 3:
        raise ValueError("gbuffer must be (H, W, 16) records")
    h, w = rec.shape[0], rec.shape[1]
    tri, tri_prev = np.ascontiguousarray(tri, np.float32), np.ascontiguousarray(tri_prev, np.float32)
    if tri.size % 12 or tri.size != tri_prev.size:
        raise ValueError("tri and tri_prev must hold the same number of 12-word records")
    out = np.zeros((h, w, MOTION_WORDS), np.float32)
    _check(lib().rt_motion(rec.ctypes.data_as(_c_f), w, h, tri.ctypes.data_as(_c_f), tri_prev.ctypes.data_as(_c_f), tri.size // 12,
                           out.ctypes.data_as(_c_f)))
    return motion_unpack(out)


def temporal(sums, counts_or_spp, gbuffer, cam_prev=None, gbuffer_prev=None, history_prev=None, motion=None, **params):
    """rt_temporal (the host function): one step of the reprojected temporal history.  cam_prev (a
    Scene.camera() dict or RtCamera), gbuffer_prev and history_prev ((3, H, W, 4) float32) describe
    the previous frame; all None: a first frame.  motion: motion()'s result or its packed records
    (rt_temporal_motion); None: rt_temporal.  Returns (history (3, H, W, 4), mean (H, W, 3),
    variance (H, W)).  params: temporal_params' arguments."""
    sums, counts, spp, rec = _denoise_inputs(sums, counts_or_spp, gbuffer)
    h, w = sums.shape[0], sums.shape[1]
    cam = _camera_arg(cam_prev)
    gp = hp = None
    if gbuffer_prev is not None:
        gp = gbuffer_pack(gbuffer_prev)
        if gp.size != h * w * GBUFFER_WORDS:
            raise ValueError("gbuffer_prev must have one record per pixel")
    if history_prev is not None:
        hp = np.ascontiguousarray(history_prev, np.float32)
        if hp.size != h * w * HISTORY_WORDS:
            raise ValueError("history_prev must have three planes of one quad per pixel")
    hist, mean, var = np.zeros((3, h, w, 4), np.float32), np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    tp = temporal_params(**params)
    mo = _motion_arg(motion, h, w)
    if mo is not None:
        _check(lib().rt_temporal_motion(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None, spp, w, h,
                                        rec.ctypes.data_as(_c_f), ctypes.byref(cam) if cam is not None else None,
                                        gp.ctypes.data_as(_c_f) if gp is not None else None,
                                        hp.ctypes.data_as(_c_f) if hp is not None else None, ctypes.byref(tp),
                                        hist.ctypes.data_as(_c_f), mean.ctypes.data_as(_c_f), var.ctypes.data_as(_c_f),
                                        mo.ctypes.data_as(_c_f)))
        return hist, mean, var
    _check(lib().rt_temporal(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None, spp, w, h,
                             rec.ctypes.data_as(_c_f), ctypes.byref(cam) if cam is not None else None,
                             gp.ctypes.data_as(_c_f) if gp is not None else None, hp.ctypes.data_as(_c_f) if hp is not None else None,
                             ctypes.byref(tp), hist.ctypes.data_as(_c_f), mean.ctypes.data_as(_c_f), var.ctypes.data_as(_c_f)))
    return hist, mean, var


def motion_device(d_gbuffer_ptr, width, height, d_tri_ptr, d_tri_prev_ptr, n_tris, d_out_ptr, stream_ptr=None):
    """rt_motion_device: the motion records on the current HIP device (16-byte aligned device
    pointers), asynchronous on the stream."""
    V = ctypes.c_void_p
    _check(lib().rt_motion_device(V(d_gbuffer_ptr), width, height, V(d_tri_ptr or 0), V(d_tri_prev_ptr or 0), int(n_tris), V(d_out_ptr),
                                  V(stream_ptr or 0)))


def temporal_device(d_sums_ptr, d_counts_ptr, spp, width, height, d_gbuffer_ptr, d_history_out_ptr, d_out_ptr=0, d_var_ptr=0,
                    cam_prev=None, d_gbuffer_prev_ptr=0, d_history_prev_ptr=0, stream_ptr=None, d_motion_ptr=None, **params):
    """rt_temporal_device: the same step on the current HIP device (device pointers; 0 / None: not
    given), asynchronous on the stream.  d_motion_ptr given: rt_temporal_motion_device."""
    cam = _camera_arg(cam_prev)
    tp = temporal_params(**params)
    V = ctypes.c_void_p
    if d_motion_ptr:
        _check(lib().rt_temporal_motion_device(V(d_sums_ptr), V(d_counts_ptr or 0), int(spp), width, height, V(d_gbuffer_ptr),
                                               ctypes.byref(cam) if cam is not None else None, V(d_gbuffer_prev_ptr or 0),
                                               V(d_history_prev_ptr or 0), ctypes.byref(tp), V(d_history_out_ptr), V(d_out_ptr or 0),
                                               V(d_var_ptr or 0), V(d_motion_ptr), V(stream_ptr or 0)))
        return
    _check(lib().rt_temporal_device(V(d_sums_ptr), V(d_counts_ptr or 0), int(spp), width, height, V(d_gbuffer_ptr),
                                    ctypes.byref(cam) if cam is not None else None, V(d_gbuffer_prev_ptr or 0),
                                    V(d_history_prev_ptr or 0), ctypes.byref(tp), V(d_history_out_ptr), V(d_out_ptr or 0),
                                    V(d_var_ptr or 0), V(stream_ptr or 0)))


def variance_from_moments(sums, moments, counts_or_spp, gbuffer):
    """rt_variance_from_moments (the host function): the (H, W) float32 variance of each pixel's
    demodulated mean, from its (H, W, 3) sums and moments (Accumulator.sums / moments), its count
    and its first-hit record.  Per pixel, so any pixel range with its own records will do."""
    sums, counts, spp, rec = _denoise_inputs(sums, counts_or_spp, gbuffer)
    moments = np.ascontiguousarray(moments, np.float32)
    if moments.shape != sums.shape:
        raise ValueError("moments must have the sums' shape")
    h, w = sums.shape[0], sums.shape[1]
    out = np.zeros((h, w), np.float32)
    _check(lib().rt_variance_from_moments(sums.ctypes.data_as(_c_f), moments.ctypes.data_as(_c_f),
                                          counts.ctypes.data_as(_c_i) if counts is not None else None, spp, w, h,
                                          rec.ctypes.data_as(_c_f), out.ctypes.data_as(_c_f)))
    return out


def variance_from_moments_device(d_sums_ptr, d_moments_ptr, d_counts_ptr, spp, width, height, d_gbuffer_ptr, d_out_ptr,
                                 stream_ptr=None):
    """rt_variance_from_moments_device: the same on the current HIP device (device pointers;
    d_counts_ptr 0 / None: one spp), asynchronous on the stream."""
    _check(lib().rt_variance_from_moments_device(ctypes.c_void_p(d_sums_ptr), ctypes.c_void_p(d_moments_ptr),
                                                 ctypes.c_void_p(d_counts_ptr or 0), int(spp), width, height,
                                                 ctypes.c_void_p(d_gbuffer_ptr), ctypes.c_void_p(d_out_ptr),
                                                 ctypes.c_void_p(stream_ptr or 0)))


def _variance_input(variance, h, w):
    if variance is None:
        return None
    variance = np.ascontiguousarray(variance, np.float32)
    if variance.size != h * w:
        raise ValueError("variance must have one entry per pixel")
    return variance


def denoise_guided(sums, counts_or_spp, gbuffer, variance=None, return_variance=False, **params):
    """rt_denoise_guided (the host function): the variance-guided mode of the denoiser, with its
    firefly clamp.  variance: None (the spatial estimate) or an (H, W) array, the variance of each
    pixel's demodulated mean.  return_variance: also the (H, W) filtered variance.  params:
    denoise_guided_params' arguments."""
    sums, counts, spp, rec = _denoise_inputs(sums, counts_or_spp, gbuffer)
    h, w = sums.shape[0], sums.shape[1]
    variance = _variance_input(variance, h, w)
    out = np.zeros((h, w, 3), np.float32)
    out_v = np.zeros((h, w), np.float32) if return_variance else None
    gp = denoise_guided_params(**params)
    _check(lib().rt_denoise_guided(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None, spp, w, h,
                                   rec.ctypes.data_as(_c_f), variance.ctypes.data_as(_c_f) if variance is not None else None,
                                   ctypes.byref(gp), out.ctypes.data_as(_c_f),
                                   out_v.ctypes.data_as(_c_f) if return_variance else None))
    return (out, out_v) if return_variance else out


def denoise_guided_frame_u8(sums, counts_or_spp, gbuffer, variance=None, device=0, **params):
    """rt_denoise_guided_frame_u8: host arrays in, the guided mode's (H, W, 3) bytes out, filtered
    and finished on `device`."""
    sums, counts, spp, rec = _denoise_inputs(sums, counts_or_spp, gbuffer)
    h, w = sums.shape[0], sums.shape[1]
    variance = _variance_input(variance, h, w)
    rgb = np.zeros((h, w, 3), np.uint8)
    gp = denoise_guided_params(**params)
    _check(lib().rt_denoise_guided_frame_u8(sums.ctypes.data_as(_c_f), counts.ctypes.data_as(_c_i) if counts is not None else None,
                                            spp, w, h, rec.ctypes.data_as(_c_f),
                                            variance.ctypes.data_as(_c_f) if variance is not None else None, ctypes.byref(gp),
                                            device, rgb.ctypes.data_as(_c_b)))
    return rgb


def denoise_guided_device(d_sums_ptr, d_counts_ptr, spp, width, height, d_gbuffer_ptr, d_out_ptr, stream_ptr=None,
                          d_variance_ptr=None, d_out_variance_ptr=None, **params):
    """rt_denoise_guided_device: the guided mode on the current HIP device (device pointers;
    d_counts_ptr, d_variance_ptr, d_out_variance_ptr 0 / None: not given), asynchronous on the stream."""
    gp = denoise_guided_params(**params)
    _check(lib().rt_denoise_guided_device(ctypes.c_void_p(d_sums_ptr), ctypes.c_void_p(d_counts_ptr or 0), int(spp), width, height,
                                          ctypes.c_void_p(d_gbuffer_ptr), ctypes.c_void_p(d_variance_ptr or 0), ctypes.byref(gp),
                                          ctypes.c_void_p(d_out_ptr), ctypes.c_void_p(d_out_variance_ptr or 0),
                                          ctypes.c_void_p(stream_ptr or 0)))


def tonemap_device(d_sum_ptr, width, height, spp, d_rgb_ptr, stream_ptr=None):
    """rt_tonemap_u8_device: the frame finish on the GPU (device pointers, e.g. torch tensors)."""
    _check(lib().rt_tonemap_u8_device(ctypes.c_void_p(d_sum_ptr), width, height, spp, ctypes.c_void_p(d_rgb_ptr),
                                      ctypes.c_void_p(stream_ptr or 0)))


def write_ppm(filename, rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    _check(lib().rt_write_ppm(os.fsencode(filename), rgb.ctypes.data_as(_c_b), rgb.shape[1], rgb.shape[0]))


def device_count():
    return int(lib().rt_device_count())


def device_selfcheck(which=0):
    """rt_device_selfcheck: mismatches of the kernels' hardware-dependent exact arithmetic
    (0: the fast reciprocal over every float with a normal reciprocal; 1: the computed linear
    texel decode over every byte and the packed LDS RNG word over every minstd state; 2: the
    cooperative leaf step over synthetic leaves; 3: the traversal's root-free cull, far_gt and
    the squared 1e9 constant, against sqrtf(x) > acc over 2^24 pairs at the rounding boundary;
    4: the material records of every scene that is on a device, dword for dword against the
    scene's tables there; an error where no scene is uploaded; 5: whole closest-hit queries
    of 16,384 hashed rays on every uploaded scene through the cooperative step, against the
    per-lane step loop)."""
    n = ctypes.c_uint64(0)
    _check(lib().rt_device_selfcheck(which, ctypes.byref(n)))
    return int(n.value)
