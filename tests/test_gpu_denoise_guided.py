"""The denoiser's variance-guided mode on the GPU (include/rt_hw.h rt_denoise_guided_device,
rt_denoise_guided_frame_u8, rt_accum_frame_u8_guided): the kernels against the host function, bit
for bit, out_mean and out_variance; the scratch it shares with rt_denoise_device; the
accumulator's guided finish, which must leave the accumulator as it was; and that the mode beats
the plain filter on the GPU's own low-sample frames."""
import numpy as np
import pytest

import rtref
from denoise_util import f32, synthetic
from test_denoise_guided import given_variance
from test_gpu_accum import gpu   # noqa: F401  (fixture)
from test_gpu_denoise import assert_unchanged, device_denoise, real_frame, scene_of, snapshot

pytestmark = pytest.mark.gpu
bits = rtref.bits
GUARD = 64   # words after each output that must stay untouched

_cache = {}


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def frame_of(gpu, which):
    if which == "real":
        return real_frame(gpu)
    if which not in _cache:
        _cache[which] = synthetic(*which)[:3]
    return _cache[which]


def device_guided(gpu, sums, counts, spp, rec, variance=None, **params):
    """rt_denoise_guided_device on torch buffers: (out_mean, out_variance), guard words checked."""
    import torch
    h, w = sums.shape[:2]
    d_s = torch.from_numpy(np.ascontiguousarray(sums)).cuda()
    d_g = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    d_c = torch.from_numpy(np.ascontiguousarray(counts)).cuda() if counts is not None else None
    d_v = torch.from_numpy(np.ascontiguousarray(variance)).cuda() if variance is not None else None
    d_o = torch.full((h * w * 3 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    d_ov = torch.full((h * w + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu.denoise_guided_device(d_s.data_ptr(), d_c.data_ptr() if d_c is not None else 0, spp, w, h, d_g.data_ptr(), d_o.data_ptr(),
                              torch.cuda.current_stream().cuda_stream, d_variance_ptr=d_v.data_ptr() if d_v is not None else 0,
                              d_out_variance_ptr=d_ov.data_ptr(), **params)
    torch.cuda.synchronize()
    o, ov = d_o.cpu().numpy(), d_ov.cpu().numpy()
    assert (o[h * w * 3:] == -7.0).all() and (ov[h * w:] == -7.0).all(), "wrote past an output"
    return o[:h * w * 3].reshape(h, w, 3), ov[:h * w].reshape(h, w)


def check_device(gpu, sums, counts_or_spp, rec, variance=None, runs=1, **params):
    want, want_v = gpu.denoise_guided(sums, counts_or_spp, rec, variance=variance, return_variance=True, **params)
    counts, spp = (None, counts_or_spp) if np.ndim(counts_or_spp) == 0 else (counts_or_spp, 0)
    for run in range(runs):
        got, got_v = device_guided(gpu, sums, counts, spp, rec, variance=variance, **params)
        assert same_bits(got, want), f"{params} run {run}: out_mean, {(bits(got) != bits(want)).any(-1).sum()} pixels differ"
        assert same_bits(got_v, want_v), f"{params} run {run}: out_variance, {(bits(got_v) != bits(want_v)).sum()} pixels differ"


# 5 x 3: smaller than every window; 20 x 7: inside one 32 x 8 tile; 33 x 17: one column past a tile;
# 70 x 45: straddles tiles in both axes
@pytest.mark.parametrize("which", [(5, 3), (20, 7), (32, 8), (33, 17), (70, 45), "real"])
def test_device_filter_matches_the_host_function(gpu, which):
    """Iterations 0 .. 6 cover the staged levels (strides 1 and 2) and the levels that read through
    L2; the second run reuses the scratch."""
    sums, counts, rec = frame_of(gpu, which)
    for it in range(0, 7):
        check_device(gpu, sums, counts, rec, runs=2, iterations=it)
        check_device(gpu, sums, 8, rec, iterations=it)


@pytest.mark.parametrize("which", [(5, 3), (33, 17), (70, 45), "real"])
def test_device_filter_other_inputs(gpu, which):
    sums, counts, rec = frame_of(gpu, which)
    h, w = sums.shape[:2]
    check_device(gpu, sums, counts, rec, firefly=-1.0)
    check_device(gpu, sums, counts, rec, firefly=2.0, iterations=2)
    check_device(gpu, sums, counts, rec, variance=given_variance(w, h))
    check_device(gpu, sums, 8, rec, variance=given_variance(w, h), firefly=-1.0, iterations=3)
    check_device(gpu, sums, counts, rec, iterations=4, sigma_var=0.7, sigma_plane=0.5, normal_power_log2=2, firefly=3.0)


def test_scratch_across_sizes_and_modes(gpu):
    """The per-device scratch only grows, and the plain filter runs on the same one."""
    for which in [(70, 45), (33, 17), (70, 45)]:
        sums, counts, rec = frame_of(gpu, which)
        check_device(gpu, sums, counts, rec)
    sums, counts, rec = frame_of(gpu, (70, 45))
    assert same_bits(device_denoise(gpu, sums, counts, 0, rec), gpu.denoise(sums, counts, rec))
    check_device(gpu, sums, counts, rec)


def test_host_arrays_to_bytes(gpu):
    """rt_denoise_guided_frame_u8: the host function's frame, finished at spp 1."""
    for which, it in [((70, 45), 5), ("real", 3)]:
        sums, counts, rec = frame_of(gpu, which)
        h, w = sums.shape[:2]
        assert np.array_equal(gpu.denoise_guided_frame_u8(sums, counts, rec, iterations=it),
                              gpu.tonemap(gpu.denoise_guided(sums, counts, rec, iterations=it), 1))
        assert np.array_equal(gpu.denoise_guided_frame_u8(sums, 8, rec, iterations=it, firefly=2.0),
                              gpu.tonemap(gpu.denoise_guided(sums, 8, rec, iterations=it, firefly=2.0), 1))
        var = given_variance(w, h)
        assert np.array_equal(gpu.denoise_guided_frame_u8(sums, counts, rec, variance=var, iterations=it),
                              gpu.tonemap(gpu.denoise_guided(sums, counts, rec, variance=var, iterations=it), 1))


# ------------------------------------------------------------------------ accumulator
def check_guided_frame(gpu, acc, rec, pending=False, **params):
    before = snapshot(acc, pending)
    got = acc.frame(denoise=params or True, guided=True)
    want = gpu.tonemap(gpu.denoise_guided(before["sums"], before["counts"], rec, **params), 1)
    assert np.array_equal(got, want), f"{(got != want).any(-1).sum()} pixels differ"
    assert_unchanged(acc, before, pending)
    return got


@pytest.mark.parametrize("fast", [False, True])
def test_accumulator_guided_frame(gpu, fast):
    scene = scene_of(gpu, "cornell", 64, 64)
    rec = scene.gbuffer()["records"]
    acc = scene.accumulator(fast=fast)
    try:
        acc.add(4)
        first = check_guided_frame(gpu, acc, rec)
        assert (first != acc.frame()).any(), "the filter changed nothing"
        assert (first != acc.frame(denoise=True)).any(), "the guided mode is the plain filter"
        check_guided_frame(gpu, acc, rec, iterations=2, sigma_var=0.5, firefly=-1.0)
        # a subset pass: the counts differ and a window has been refined; then a pending selection
        acc.mark()
        assert acc.select(12, window=(8, 8, 40, 40)) == 32 * 32
        acc.add_selected()
        assert acc.sample_range == (4, 12)
        n = acc.select(16, window=(0, 0, 20, 20))
        assert n == 400
        check_guided_frame(gpu, acc, rec, pending=True)
        assert acc.add_selected()["pixels"] == n   # the pending selection is still the one made
        check_guided_frame(gpu, acc, rec)
        # the plain mode on the same accumulator's scratch afterwards
        assert np.array_equal(acc.frame(denoise=True), gpu.tonemap(gpu.denoise(acc.sums(), acc.counts(), rec), 1))
    finally:
        acc.free()


@pytest.mark.parametrize("fast", [False, True])
def test_refused_call_leaves_later_calls_correct(gpu, fast):
    """A call refused for its parameters, as the first guided frame of a fresh accumulator, leaves
    no G-buffer behind that was allocated and never rendered."""
    scene = scene_of(gpu, "cornell", 64, 64)
    rec = scene.gbuffer()["records"]
    acc = scene.accumulator(fast=fast)
    try:
        acc.add(4)
        for bad in (dict(iterations=7), dict(normal_power_log2=17), dict(sigma_var=float("nan")), dict(firefly=float("inf"))):
            with pytest.raises(gpu.RtError, match="rt_accum_frame_u8_guided"):
                acc.frame(denoise=bad, guided=True)
        check_guided_frame(gpu, acc, rec)
        with pytest.raises(gpu.RtError):
            acc.frame(denoise=dict(sigma_plane=float("inf")), guided=True)
        check_guided_frame(gpu, acc, rec, iterations=3)
    finally:
        acc.free()


def test_accumulator_guided_frame_needs_the_whole_frame(gpu):
    scene = scene_of(gpu, "cornell", 64, 64)
    acc = scene.accumulator(rank=0, world=2)
    try:
        acc.add(1)
        with pytest.raises(gpu.RtError, match="rt_denoise_guided_device"):
            acc.frame(denoise=True, guided=True)
        assert acc.frame().shape == (32, 64, 3)
    finally:
        acc.free()
    acc = scene.accumulator()
    try:
        with pytest.raises(gpu.RtError, match="no samples"):
            acc.frame(denoise=True, guided=True)
    finally:
        acc.free()


# ------------------------------------------------------------------------ it beats the plain filter
@pytest.mark.parametrize("name,w,h", [("cornell", 64, 64), ("sponza_mini", 64, 36)])
def test_it_beats_the_plain_filter(gpu, name, w, h, spp=8, truth_spp=2048):
    """The metric of test_gpu_denoise.py rmse_ratio on the GPU's own parity renders: hit pixels with
    finite values, means clamped to [0, 4].  `plain` is rt_denoise, which this mode does not touch."""
    scene = scene_of(gpu, name, w, h)
    truth = scene.render_sums(truth_spp)[0] * (f32(1) / f32(truth_spp))
    sums = scene.render_sums(spp)[0]
    g = scene.gbuffer()
    raw = sums * (f32(1) / f32(spp))
    plain, guided = gpu.denoise(sums, spp, g), gpu.denoise_guided(sums, spp, g)
    use = (g["prim"] >= 0) & np.isfinite(truth).all(-1)
    for x in (raw, plain, guided):
        use = use & np.isfinite(x).all(-1)
    assert use.mean() > 0.5

    def rmse(x):
        d = np.clip(x[use].astype(np.float64), 0, 4) - np.clip(truth[use].astype(np.float64), 0, 4)
        return float(np.sqrt((d * d).mean()))

    e_raw, e_plain, e_guided = rmse(raw), rmse(plain), rmse(guided)
    print(f"\n{name} {w}x{h}, {spp} samples against {truth_spp}: RMSE raw {e_raw:.4f}, plain {e_plain:.4f}, guided {e_guided:.4f}")
    assert e_guided < e_plain
