"""The denoiser's variance-guided mode without a GPU: rt_denoise_guided (the host function, whose
text is raytracing-hw_amd/csrc/rt_denoise_guided.h) against the numpy float32 restatement written
from include/rt_hw.h, bit for bit, out_mean and out_variance; the mode's properties (what passes
through, what the clamp caps, what stays apart); the refusals and defaults of its entry points; and
that it beats the plain filter on CPU-oracle renders of two fixtures."""
import ctypes

import numpy as np
import pytest

import rtref
from denoise_guided_util import GUIDED_DEFAULTS, np_denoise_guided
from denoise_util import arrays_of, f32, host_gbuffer, synthetic, twin
from test_denoise import two_faces

ERR_ARG, ERR_DEVICE, ERR_LIMIT = -1, -4, -5
bits = rtref.bits
# 5 x 3: smaller than every window; 20 x 7: inside one 32 x 8 tile; 33 x 17: one column past a tile;
# 70 x 45: straddles tiles in both axes
SIZES = [(5, 3), (20, 7), (33, 17), (70, 45)]


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def frames():
    return {(w, h): synthetic(w, h) for w, h in SIZES}


def given_variance(w, h):
    """A caller's variance with entries the rule replaces by 0: zero, negative, NaN, inf."""
    v = np.random.default_rng(5).random((h, w)).astype(f32) * f32(0.5)
    flat = v.reshape(-1)
    flat[0::7], flat[1::11], flat[2::13], flat[3::17] = 0, -1.5, np.nan, np.inf
    return v


def check_against_numpy(rt, sums, counts_or_spp, rec, variance=None, **params):
    got, got_v = rt.denoise_guided(sums, counts_or_spp, rec, variance=variance, return_variance=True, **params)
    counts, spp = (None, counts_or_spp) if np.ndim(counts_or_spp) == 0 else (counts_or_spp, 0)
    want, want_v = np_denoise_guided(sums, counts, spp, rec, variance=variance, **dict(GUIDED_DEFAULTS, **params))
    assert same_bits(got, want), f"out_mean: {(bits(got) != bits(want)).any(-1).sum()} pixels differ"
    assert same_bits(got_v, want_v), f"out_variance: {(bits(got_v) != bits(want_v)).sum()} pixels differ"
    assert same_bits(rt.denoise_guided(sums, counts_or_spp, rec, variance=variance, **params), want)   # (out_variance NULL)
    return got, got_v


@pytest.mark.parametrize("iterations", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("w,h", SIZES)
def test_host_function_is_the_specification(rt, frames, w, h, iterations):
    """Division is correctly rounded on both sides and nothing is contracted: no tolerance."""
    sums, counts, rec, _ = frames[w, h]
    _, v = check_against_numpy(rt, sums, counts, rec, iterations=iterations)
    if iterations and w >= 20:
        assert (v > 0).any(), "the spatial estimate found no variance in a noisy frame"


@pytest.mark.parametrize("w,h", SIZES)
def test_host_function_other_inputs(rt, frames, w, h):
    sums, counts, rec, _ = frames[w, h]
    check_against_numpy(rt, sums, 8, rec)                                   # uniform spp
    check_against_numpy(rt, sums, counts, rec, firefly=-1.0)                # clamp off
    check_against_numpy(rt, sums, counts, rec, firefly=2.0, iterations=2)   # a clamp that bites
    check_against_numpy(rt, sums, counts, rec, variance=given_variance(w, h))
    check_against_numpy(rt, sums, counts, rec, variance=given_variance(w, h), firefly=-1.0, iterations=3)
    check_against_numpy(rt, sums, counts, rec, iterations=3, sigma_var=0.7, sigma_plane=0.5, normal_power_log2=2, firefly=3.0)


def test_clamp_and_variance_input_matter(rt, frames):
    """The cases above would pass with a clamp or a variance input that did nothing."""
    sums, counts, rec, _ = frames[70, 45]
    base = rt.denoise_guided(sums, counts, rec)
    assert not same_bits(base, rt.denoise_guided(sums, counts, rec, firefly=2.0))   # (no pixel here is 8 times its neighbours)
    assert not same_bits(base, rt.denoise_guided(sums, counts, rec, variance=given_variance(70, 45)))
    assert not same_bits(base, rt.denoise(sums, counts, rec))


# ------------------------------------------------------------------------ properties
def mean_of(sums, counts):
    with np.errstate(all="ignore"):
        rn = np.where(counts > 0, f32(1) / np.maximum(counts, 1).astype(f32), f32(0)).astype(f32)
        return sums * rn[..., None]


def test_zero_iterations_return_the_mean(rt, frames):
    sums, counts, rec, _ = frames[33, 17]
    out, v = rt.denoise_guided(sums, counts, rec, iterations=0, return_variance=True)
    assert same_bits(out, mean_of(sums, counts)) and (bits(v) == 0).all()
    out, v = rt.denoise_guided(sums, 4, rec, iterations=0, firefly=2.0, variance=given_variance(33, 17), return_variance=True)
    assert same_bits(out, sums * (f32(1) / f32(4))) and (bits(v) == 0).all()


@pytest.mark.parametrize("firefly", [0.0, -1.0])
def test_non_finite_and_miss_pixels_stay_alone(rt, frames, firefly):
    """The NaN and the inf pixel are the only non-finite pixels of the output, with their own
    means, so neither reached a neighbour; a miss keeps its mean."""
    sums, counts, rec, info = frames[70, 45]
    out, v = rt.denoise_guided(sums, counts, rec, firefly=firefly, return_variance=True)
    bad = ~np.isfinite(out).all(-1)
    assert sorted(map(tuple, np.argwhere(bad))) == sorted([info["nan_at"], info["inf_at"]])
    m = mean_of(sums, counts)
    for at in (info["nan_at"], info["inf_at"]):
        assert same_bits(out[at], m[at]) and v[at] == 0
    miss = info["miss"]
    assert miss.sum() >= 4 and same_bits(out[miss], m[miss]) and (v[miss] == 0).all()
    assert np.isfinite(v).all()


def test_unmodulated_surface_passes_through(rt):
    """A hit whose albedo is at the floor in every channel (an emitter) inside a lit coplanar face:
    its own mean, bit for bit, and its neighbours' outputs are those of the frame in which it is a
    miss.  The plain filter lets its demodulated value, mean / 1e-3, flood the face."""
    sums, counts, rec, face, mean = two_faces(37, 23)
    at = (5, 9)
    assert face[at] == 0
    rec[at][4:7] = [0.0005, 0.001, 0.0]
    rec[at][8:11] = 5.0
    sums[at] = f32(5.04) * 4
    as_miss = rec.copy()
    as_miss[at] = 0
    as_miss.view(np.int32)[at][7] = as_miss.view(np.int32)[at][11] = -1
    for it in (1, 5):
        out = rt.denoise_guided(sums, counts, rec, iterations=it)
        assert same_bits(out[at], sums[at] * (f32(1) / f32(4)))
        other = rt.denoise_guided(sums, counts, as_miss, iterations=it)
        rest = np.ones(face.shape, bool)
        rest[at] = False
        assert same_bits(out[rest], other[rest])
        assert np.abs(out[rest] / mean[rest][..., None] - 1).max() <= 1e-5


def test_constant_faces_stay_constant_and_apart(rt):
    """As test_denoise.py: a weighted mean of equal values is that value up to the rounding of 25
    taps, so a constant stays constant to 1e-5, and perpendicular faces do not mix, because their
    normal term is exactly 0.  Nothing is clamped (no pixel is above 8 times its neighbours' mean)
    and the variance of a constant is 0 up to rounding: s2 / sg and mu * mu are each L^2 = 9 within
    the rounding of 49 taps, about 50 * 2^-23 relative, in three channels: below 3.3e-4."""
    sums, counts, rec, face, mean = two_faces(37, 23)
    out, v = rt.denoise_guided(sums, counts, rec, return_variance=True)
    assert np.abs(out / mean[..., None] - 1).max() <= 1e-5
    y, xs = 23 // 2 + 1, slice(0, (2 * 37) // 3)
    assert (face[y, xs] == 0).all() and (face[y + 1, xs] == 1).all()
    assert np.abs(out[y, xs] / np.float32(1.5) - 1).max() <= 1e-5
    assert np.abs(out[y + 1, xs] / np.float32(0.25) - 1).max() <= 1e-5
    assert (v >= 0).all() and v.max() <= 3.3e-4


def test_pixel_without_samples_is_filled(rt):
    sums, counts, rec, face, mean = two_faces(37, 23)
    at = (5, 9)
    assert face[at] == 0
    counts[at] = 0
    sums[at] = 0
    for it in (1, 5):
        out = rt.denoise_guided(sums, counts, rec, iterations=it)
        assert np.abs(out[at] / mean[at] - 1).max() <= 1e-5
    assert (rt.denoise_guided(sums, counts, rec, iterations=0)[at] == 0).all()


def test_firefly_is_capped(rt):
    """One pixel at 1000 times its constant face.  The clamp scales its demodulated colour to a
    luminance of firefly times its neighbours' mean, and every level replaces it by a weighted
    mean of values that are at most that, so it comes out at most firefly times the face's value
    (up to rounding: the luminance weights sum to 1 within 1e-7, the taps' roundings as above)."""
    sums, counts, rec, face, mean = two_faces(37, 23)
    at = (5, 9)
    assert face[at] == 0
    sums[at] = sums[at] * f32(1000)
    for firefly in (8.0, 3.0):
        for it in (1, 5):
            out = rt.denoise_guided(sums, counts, rec, iterations=it, firefly=firefly)
            assert out[at].max() <= firefly * mean[at] * (1 + 1e-5), (firefly, it, out[at])
            assert np.isfinite(out).all()
    on = rt.denoise_guided(sums, counts, rec)
    off = rt.denoise_guided(sums, counts, rec, firefly=-1.0)
    assert not same_bits(on, off) and off[at].max() > on[at].max()


def test_pure_function(rt, frames):
    sums, counts, rec, _ = frames[70, 45]
    var = given_variance(70, 45)
    keep = sums.copy(), counts.copy(), rec.copy(), var.copy()
    for variance in (None, var):
        a = rt.denoise_guided(sums, counts, rec, variance=variance, return_variance=True)
        b = rt.denoise_guided(sums, counts, rec, variance=variance, return_variance=True)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    assert same_bits(sums, keep[0]) and np.array_equal(counts, keep[1]) and same_bits(rec, keep[2]) and same_bits(var, keep[3])


# ------------------------------------------------------------------------ refusals and defaults
def test_defaults(rt, frames):
    """Zeroed fields, a negative iteration count and no parameters at all are the documented defaults."""
    sums, counts, rec, _ = frames[33, 17]
    want, want_v = rt.denoise_guided(sums, counts, rec, return_variance=True, **GUIDED_DEFAULTS)
    assert same_bits(rt.denoise_guided(sums, counts, rec), want)
    assert same_bits(rt.denoise_guided(sums, counts, rec, iterations=-1, sigma_var=0, sigma_plane=-1, normal_power_log2=0, firefly=0),
                     want)
    out, out_v = np.zeros_like(want), np.zeros_like(want_v)
    c = np.ascontiguousarray(counts)
    F = rt._c_f
    assert rt.lib().rt_denoise_guided(sums.ctypes.data_as(F), c.ctypes.data_as(rt._c_i), 0, 33, 17, rec.ctypes.data_as(F), None, None,
                                      out.ctypes.data_as(F), out_v.ctypes.data_as(F)) == 0
    assert same_bits(out, want) and same_bits(out_v, want_v)


def test_argument_refusals(rt):
    """Every entry of the mode refuses bad arguments before any device work, as include/rt_hw.h says."""
    lib = rt.lib()
    sums, counts, rec, _ = synthetic(37, 23)
    out = np.zeros_like(sums)
    S, C, G, O = sums.ctypes.data_as(rt._c_f), counts.ctypes.data_as(rt._c_i), rec.ctypes.data_as(rt._c_f), out.ctypes.data_as(rt._c_f)
    gp = rt.denoise_guided_params

    def host(s=S, c=C, spp=0, w=37, h=23, g=G, p=None, o=O):
        return lib.rt_denoise_guided(s, c, spp, w, h, g, None, ctypes.byref(p) if p is not None else None, o, None)

    def device(s=1, c=1, spp=0, w=37, h=23, g=1, p=None, o=1):
        V = ctypes.c_void_p
        return lib.rt_denoise_guided_device(V(s), V(c), spp, w, h, V(g), None, ctypes.byref(p) if p is not None else None, V(o), None,
                                            None)

    def frame(s=S, c=C, spp=0, w=37, h=23, g=G, p=None, o=np.zeros(37 * 23 * 3, np.uint8).ctypes.data_as(rt._c_b)):
        return lib.rt_denoise_guided_frame_u8(s, c, spp, w, h, g, None, ctypes.byref(p) if p is not None else None, 0, o)

    for call in (host, device, frame):
        assert call(s=None) == ERR_ARG and call(g=None) == ERR_ARG and call(o=None) == ERR_ARG
        assert call(w=0) == ERR_ARG and call(h=-1) == ERR_ARG
        assert call(c=None, spp=0) == ERR_ARG
        assert call(p=gp(iterations=7)) == ERR_ARG and call(p=gp(normal_power_log2=17)) == ERR_ARG
        assert call(p=gp(sigma_var=float("nan"))) == ERR_ARG and call(p=gp(sigma_var=float("inf"))) == ERR_ARG
        assert call(p=gp(sigma_plane=float("inf"))) == ERR_ARG and call(p=gp(sigma_plane=float("nan"))) == ERR_ARG
        assert call(p=gp(firefly=float("nan"))) == ERR_ARG and call(p=gp(firefly=float("-inf"))) == ERR_ARG
        assert b"rt_denoise_guided" in lib.rt_last_error()
        assert call(w=1 << 16, h=1 << 15) == ERR_LIMIT
    assert host() == 0 and host(p=gp(iterations=6, normal_power_log2=16, firefly=-1.0)) == 0
    if rt.device_count() == 0:
        assert device() == ERR_DEVICE and frame() == ERR_DEVICE
    rgb = np.zeros(8 * 8 * 3, np.uint8)
    assert lib.rt_accum_frame_u8_guided(None, None, rgb.ctypes.data_as(rt._c_b)) == ERR_ARG
    for name in ("rt_denoise_guided", "rt_denoise_guided_device", "rt_denoise_guided_frame_u8", "rt_accum_frame_u8_guided"):
        assert name in rt.ABI
    assert lib.rt_abi_version() == 6


# ------------------------------------------------------------------------ it beats the plain filter
@pytest.fixture(scope="module")
def gh(tmp_path_factory):
    return twin(tmp_path_factory)


@pytest.mark.parametrize("name,w,h", [("cornell", 64, 64), ("sponza_mini", 64, 36)])
def test_it_beats_the_plain_filter(rt, oracle, gh, name, w, h):
    """8 samples against 512, both rendered by the CPU oracle; the metric of
    test_gpu_denoise.py rmse_ratio (hit pixels, finite values, means clamped to [0, 4]).  `plain`
    is rt_denoise, which this mode does not touch."""
    arrays = arrays_of(rt, name, w, h)
    rec = host_gbuffer(rt, gh, name, w, h)[0].reshape(h, w, 16)
    truth = oracle.render(arrays, 512)[0].reshape(h, w, 3) * (f32(1) / f32(512))
    sums = oracle.render(arrays, 8)[0].reshape(h, w, 3)
    raw = sums * (f32(1) / f32(8))
    plain = rt.denoise(sums, 8, rec)
    guided = rt.denoise_guided(sums, 8, rec)
    use = (rec.view(np.int32)[..., 7] >= 0) & np.isfinite(truth).all(-1)
    for x in (raw, plain, guided):
        use = use & np.isfinite(x).all(-1)
    assert use.mean() > 0.5

    def rmse(x):
        d = np.clip(x[use].astype(np.float64), 0, 4) - np.clip(truth[use].astype(np.float64), 0, 4)
        return float(np.sqrt((d * d).mean()))

    e_raw, e_plain, e_guided = rmse(raw), rmse(plain), rmse(guided)
    print(f"\n{name} {w}x{h}, 8 samples against 512: RMSE raw {e_raw:.4f}, plain {e_plain:.4f}, guided {e_guided:.4f}")
    assert e_guided < e_plain and e_guided < e_raw
