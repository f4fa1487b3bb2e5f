"""The frame denoiser without a GPU: rt_denoise (the host function of librt_hw_amd.so, whose text is
raytracing-hw_amd/csrc/rt_denoise.h) against a numpy float32 restatement written from
include/rt_hw.h, bit for bit; the filter's properties (what it passes through, fills, keeps apart);
and the argument refusals of every new entry point, all decided before any device call."""
import ctypes

import numpy as np
import pytest

import rtref
from denoise_util import DEFAULTS, f32, np_denoise, synthetic

ERR_ARG, ERR_DEVICE, ERR_LIMIT = -1, -4, -5
bits = rtref.bits


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def frames():
    return {(w, h): synthetic(w, h) for w, h in [(5, 3), (32, 8), (37, 23), (70, 45)]}


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("w,h", [(5, 3), (32, 8), (37, 23), (70, 45)])
def test_host_function_is_the_specification(rt, frames, w, h, iterations):
    """Division is correctly rounded on both sides and nothing is contracted: no tolerance."""
    sums, counts, rec, _ = frames[w, h]
    got = rt.denoise(sums, counts, rec, iterations=iterations)
    want = np_denoise(sums, counts, 0, rec, **dict(DEFAULTS, iterations=iterations))
    assert same_bits(got, want), f"{(bits(got) != bits(want)).any(-1).sum()} pixels differ"


def test_host_function_other_parameters_and_uniform_spp(rt, frames):
    sums, counts, rec, _ = frames[37, 23]
    p = dict(iterations=3, sigma_color=0.35, sigma_plane=0.5, normal_power_log2=2)
    assert same_bits(rt.denoise(sums, counts, rec, **p), np_denoise(sums, counts, 0, rec, **p))
    assert same_bits(rt.denoise(sums, 8, rec, **p), np_denoise(sums, None, 8, rec, **p))


def test_zero_iterations_return_the_mean(rt, frames):
    sums, counts, rec, _ = frames[37, 23]
    with np.errstate(all="ignore"):
        rn = np.where(counts > 0, f32(1) / np.maximum(counts, 1).astype(f32), f32(0)).astype(f32)
        assert same_bits(rt.denoise(sums, counts, rec, iterations=0), sums * rn[..., None])
        assert same_bits(rt.denoise(sums, 4, rec, iterations=0), sums * (f32(1) / f32(4)))


def test_defaults(rt, frames):
    """Zeroed sigmas and exponent, a negative iteration count and no parameters at all are the
    documented defaults."""
    sums, counts, rec, _ = frames[37, 23]
    want = rt.denoise(sums, counts, rec, **DEFAULTS)
    assert same_bits(rt.denoise(sums, counts, rec), want)
    assert same_bits(rt.denoise(sums, counts, rec, iterations=-1, sigma_color=0, sigma_plane=-1, normal_power_log2=0), want)
    out = np.zeros_like(want)
    c = np.ascontiguousarray(counts)
    assert rt.lib().rt_denoise(sums.ctypes.data_as(rt._c_f), c.ctypes.data_as(rt._c_i), 0, 37, 23, rec.ctypes.data_as(rt._c_f),
                               None, out.ctypes.data_as(rt._c_f)) == 0
    assert same_bits(out, want)


def test_pure_function(rt, frames):
    sums, counts, rec, _ = frames[70, 45]
    keep = sums.copy(), counts.copy(), rec.copy()
    a = rt.denoise(sums, counts, rec)
    b = rt.denoise(sums, counts, rec)
    assert same_bits(a, b)
    assert same_bits(sums, keep[0]) and np.array_equal(counts, keep[1]) and same_bits(rec, keep[2])


def test_non_finite_pixels_stay_alone(rt, frames):
    """A NaN and an inf pixel are the only non-finite pixels of the output, with their own means."""
    sums, counts, rec, info = frames[70, 45]
    out = rt.denoise(sums, counts, rec)
    bad = ~np.isfinite(out).all(-1)
    assert sorted(map(tuple, np.argwhere(bad))) == sorted([info["nan_at"], info["inf_at"]])
    for at in (info["nan_at"], info["inf_at"]):
        assert same_bits(out[at], sums[at] * (f32(1) / f32(counts[at])))


def test_miss_pixels_pass_through(rt, frames):
    sums, counts, rec, info = frames[70, 45]
    out = rt.denoise(sums, counts, rec)
    miss = info["miss"]
    with np.errstate(all="ignore"):
        rn = np.where(counts > 0, f32(1) / np.maximum(counts, 1).astype(f32), f32(0)).astype(f32)
    assert miss.sum() >= 4 and same_bits(out[miss], (sums * rn[..., None])[miss])


def two_faces(w, h, values=(1.5, 0.25)):
    """A wall over a floor, constant albedo and a constant mean on each, every pixel at 4 samples."""
    sums, counts, rec, info = synthetic(w, h, seed=3)
    rec = rec.copy()
    ids = rec.view(np.int32)
    left = np.zeros((h, w), bool)
    left[:, :(2 * w) // 3] = True
    ids[..., 7] = np.where(ids[..., 7] < 0, 0, ids[..., 7])   # no misses
    ids[..., 11] = np.maximum(ids[..., 11], 0)
    face = info["face"]
    N = np.array([[0, 0, -1], [0, -1, 0], [0, 0, -1]], f32)[face]
    rec[..., 0:3] = N
    rec[..., 3] = np.where(rec[..., 3] > 0, rec[..., 3], f32(4))
    rec[..., 4:7] = f32(0.5)
    rec[..., 8:11] = 0
    counts = np.full((h, w), 4, np.int32)
    mean = np.where(face == 1, f32(values[1]), f32(values[0])).astype(f32)
    sums = np.repeat((mean * f32(4))[..., None], 3, -1).astype(f32)
    return sums, counts, rec, face, mean


def test_constant_faces_stay_constant_and_apart(rt):
    """A weighted mean of equal values is that value up to the rounding of 25 taps (a few 1e-7
    relative): a constant over a plane stays constant to 1e-5, and two perpendicular faces with
    different constants do not mix to the same bound, because their normal term is exactly 0."""
    sums, counts, rec, face, mean = two_faces(37, 23)
    out = rt.denoise(sums, counts, rec)
    assert np.abs(out / mean[..., None] - 1).max() <= 1e-5
    # the two rows that meet at the wall / floor edge keep their own face's value
    y, xs = 23 // 2 + 1, slice(0, (2 * 37) // 3)
    assert (face[y, xs] == 0).all() and (face[y + 1, xs] == 1).all()
    assert np.abs(out[y, xs] / np.float32(1.5) - 1).max() <= 1e-5
    assert np.abs(out[y + 1, xs] / np.float32(0.25) - 1).max() <= 1e-5


def test_pixel_without_samples_is_filled(rt):
    sums, counts, rec, face, mean = two_faces(37, 23)
    at = (5, 9)
    assert face[at] == 0
    counts[at] = 0
    sums[at] = 0
    for it in (1, 5):
        out = rt.denoise(sums, counts, rec, iterations=it)
        assert np.abs(out[at] / mean[at] - 1).max() <= 1e-5
    assert (rt.denoise(sums, counts, rec, iterations=0)[at] == 0).all()   # (unfiltered: black, as the finish gives)


def test_argument_refusals(rt):
    """Every new entry refuses bad arguments before any device work, as include/rt_hw.h says."""
    lib = rt.lib()
    sums, counts, rec, _ = synthetic(37, 23)
    out = np.zeros_like(sums)
    S, C, G, O = sums.ctypes.data_as(rt._c_f), counts.ctypes.data_as(rt._c_i), rec.ctypes.data_as(rt._c_f), out.ctypes.data_as(rt._c_f)
    dp = rt.denoise_params

    def host(s=S, c=C, spp=0, w=37, h=23, g=G, p=None, o=O):
        return lib.rt_denoise(s, c, spp, w, h, g, ctypes.byref(p) if p is not None else None, o)

    def device(s=1, c=1, spp=0, w=37, h=23, g=1, p=None, o=1):
        V = ctypes.c_void_p
        return lib.rt_denoise_device(V(s), V(c), spp, w, h, V(g), ctypes.byref(p) if p is not None else None, V(o), None)

    def frame(s=S, c=C, spp=0, w=37, h=23, g=G, p=None, o=np.zeros(37 * 23 * 3, np.uint8).ctypes.data_as(rt._c_b)):
        return lib.rt_denoise_frame_u8(s, c, spp, w, h, g, ctypes.byref(p) if p is not None else None, 0, o)

    for call in (host, device, frame):
        assert call(s=None) == ERR_ARG and call(g=None) == ERR_ARG and call(o=None) == ERR_ARG
        assert call(w=0) == ERR_ARG and call(h=-1) == ERR_ARG
        assert call(c=None, spp=0) == ERR_ARG
        assert call(p=dp(iterations=7)) == ERR_ARG and call(p=dp(normal_power_log2=17)) == ERR_ARG
        assert call(p=dp(sigma_color=float("nan"))) == ERR_ARG and call(p=dp(sigma_plane=float("inf"))) == ERR_ARG
        assert b"rt_denoise" in lib.rt_last_error()
        assert call(w=1 << 16, h=1 << 15) == ERR_LIMIT
    assert host() == 0
    if rt.device_count() == 0:
        assert device() == ERR_DEVICE and frame() == ERR_DEVICE
    # the feature buffer
    s = rt.Scene.load(rtref.scene_path("cornell"), 8, 8, 1)
    p = rt.RtParams(0, 0, 1, 8, 0, 0, 0, 0, 0)
    g = np.zeros((64, 16), f32)
    assert lib.rt_gbuffer(None, ctypes.byref(p), g.ctypes.data_as(rt._c_f)) == ERR_ARG
    assert lib.rt_gbuffer(s.handle, None, g.ctypes.data_as(rt._c_f)) == ERR_ARG
    assert lib.rt_gbuffer(s.handle, ctypes.byref(p), None) == ERR_ARG
    assert lib.rt_gbuffer_device(s.handle, ctypes.byref(p), None, None) == ERR_ARG
    bad = rt.RtParams(0, 2, 2, 8, 0, 0, 0, 0, 0)   # rank outside the world
    assert lib.rt_gbuffer(s.handle, ctypes.byref(bad), g.ctypes.data_as(rt._c_f)) == ERR_ARG
    assert lib.rt_gbuffer_device(s.handle, ctypes.byref(bad), ctypes.c_void_p(1), None) == ERR_ARG
    assert lib.rt_gbuffer_device(s.handle, ctypes.byref(p), ctypes.c_void_p(1), None) == ERR_ARG   # not uploaded
    assert b"not uploaded" in lib.rt_last_error()
    nodev = rt.RtParams(0, 0, 1, 8, 0, 0, 0, 0, 63)
    assert lib.rt_gbuffer(s.handle, ctypes.byref(nodev), g.ctypes.data_as(rt._c_f)) == ERR_DEVICE
    if rt.device_count() == 0:
        assert lib.rt_gbuffer(s.handle, ctypes.byref(p), g.ctypes.data_as(rt._c_f)) == ERR_DEVICE
    # the accumulator's denoised finish
    rgb = np.zeros(8 * 8 * 3, np.uint8)
    assert lib.rt_accum_frame_u8_denoised(None, None, rgb.ctypes.data_as(rt._c_b)) == ERR_ARG
    for name in ("rt_gbuffer", "rt_gbuffer_device", "rt_denoise", "rt_denoise_device", "rt_denoise_frame_u8",
                 "rt_accum_frame_u8_denoised"):
        assert name in rt.ABI
