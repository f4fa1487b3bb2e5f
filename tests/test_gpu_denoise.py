"""The first-hit feature buffer and the frame denoiser on the GPU (include/rt_hw.h rt_gbuffer*,
rt_denoise_device, rt_accum_frame_u8_denoised): the G-buffer kernel against its host twin
(tests/native/gbuffer_host.cpp) and the filter kernels against the host function, both bit for
bit; the accumulator's denoised finish, which must leave the accumulator as it was; and that the
filter does its job on a low-sample frame."""
import numpy as np
import pytest

import rtref
from denoise_util import FIXTURES, arrays_of, f32, host_gbuffer, synthetic, twin
from test_gpu_accum import gpu   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
bits = rtref.bits

_scenes = {}
_cache = {}


@pytest.fixture(scope="module")
def gh(tmp_path_factory):
    return twin(tmp_path_factory)


def scene_of(gpu, name, w, h):
    if (name, w, h) not in _scenes:
        _scenes[name, w, h] = gpu.Scene.from_view(arrays_of(gpu, name, w, h))
    return _scenes[name, w, h]


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------ feature buffer
@pytest.mark.parametrize("name,w,h", FIXTURES)
def test_gbuffer_matches_the_host_twin(gpu, gh, name, w, h):
    want = host_gbuffer(gpu, gh, name, w, h)[0]
    g = scene_of(gpu, name, w, h).gbuffer()
    assert np.array_equal(g["records"].reshape(-1, 16).view(np.uint32), want.view(np.uint32))
    ids = want.view(np.int32)
    assert np.array_equal(g["prim"].reshape(-1), ids[:, 7]) and np.array_equal(g["mesh"].reshape(-1), ids[:, 11])
    assert same_bits(g["normal"].reshape(-1, 3), want[:, 0:3]) and same_bits(g["depth"].reshape(-1), want[:, 3])
    assert same_bits(g["albedo"].reshape(-1, 3), want[:, 4:7]) and same_bits(g["emission"].reshape(-1, 3), want[:, 8:11])
    assert same_bits(g["position"].reshape(-1, 3), want[:, 12:15])
    assert same_bits(gpu.gbuffer_pack({k: v for k, v in g.items() if k != "records"}).reshape(-1, 16), want)


@pytest.mark.parametrize("name,w,h,rank,world,row_block", [
    ("sponza_mini", 64, 36, 0, 3, 8), ("sponza_mini", 64, 36, 1, 3, 8), ("sponza_mini", 64, 36, 2, 3, 8),
    ("sponza_mini", 64, 36, 1, 5, 1),
    ("cornell", 33, 17, 4, 5, 1)])   # 3 rows of 33: fewer pixels than one block, a width that is no multiple of 64
def test_gbuffer_shards(gpu, gh, name, w, h, rank, world, row_block):
    """The shard layout of rt_render: the rows a (rank, world, row_block) shard owns, in order."""
    want = host_gbuffer(gpu, gh, name, w, h, rank, world, row_block)[0]
    g = scene_of(gpu, name, w, h).gbuffer(rank=rank, world=world, row_block=row_block)
    assert np.array_equal(g["records"].reshape(-1, 16).view(np.uint32), want.view(np.uint32))


def test_gbuffer_device_on_a_stream(gpu, gh):
    import torch
    name, w, h = "cornell", 33, 17
    want = host_gbuffer(gpu, gh, name, w, h)[0]
    scene = scene_of(gpu, name, w, h)
    scene.upload(0)
    stream = torch.cuda.Stream()
    guard = 64   # floats after the records that must stay untouched
    buf = torch.full((w * h * 16 + guard,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        scene.gbuffer_device(buf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:w * h * 16].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert (got[w * h * 16:] == -7.0).all()


# ------------------------------------------------------------------------ the filter
def real_frame(gpu, spp=8):
    """cornell 64 x 64 at `spp` samples with its G-buffer: (sums, counts, records)."""
    if ("real", spp) not in _cache:
        scene = scene_of(gpu, "cornell", 64, 64)
        sums, _ = scene.render_sums(spp)
        _cache["real", spp] = (sums, np.full((64, 64), spp, np.int32), scene.gbuffer()["records"])
    return _cache["real", spp]


def frame_of(gpu, which):
    if which == "real":
        return real_frame(gpu)
    w, h = which
    if which not in _cache:
        _cache[which] = synthetic(w, h)[:3]
    return _cache[which]


def device_denoise(gpu, sums, counts, spp, rec, **params):
    import torch
    h, w = sums.shape[:2]
    d_s = torch.from_numpy(np.ascontiguousarray(sums)).cuda()
    d_g = torch.from_numpy(np.ascontiguousarray(rec)).cuda()
    d_c = torch.from_numpy(np.ascontiguousarray(counts)).cuda() if counts is not None else None
    d_o = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu.denoise_device(d_s.data_ptr(), d_c.data_ptr() if d_c is not None else 0, spp, w, h, d_g.data_ptr(), d_o.data_ptr(),
                       torch.cuda.current_stream().cuda_stream, **params)
    torch.cuda.synchronize()
    return d_o.cpu().numpy()


# 5 x 3: smaller than every window; 20 x 7: inside one 32 x 8 tile; 32 x 8: exactly one tile, every
# halo slot outside the frame; 33 x 17: one column past a tile, smaller than the stride-16 reach;
# 70 x 45: straddles tiles in both axes
@pytest.mark.parametrize("which", [(5, 3), (20, 7), (32, 8), (33, 17), (70, 45), "real"])
def test_device_filter_matches_the_host_function(gpu, which):
    """Iterations 0 .. 6 cover the staged levels (strides 1 and 2) and the levels that read
    through L2 (strides 4 to 32); the second run reuses the cached scratch."""
    sums, counts, rec = frame_of(gpu, which)
    for it in range(0, 7):
        want = gpu.denoise(sums, counts, rec, iterations=it)
        for run in range(2):
            got = device_denoise(gpu, sums, counts, 0, rec, iterations=it)
            assert same_bits(got, want), f"iterations {it} run {run}: {(bits(got) != bits(want)).any(-1).sum()} pixels differ"
        want = gpu.denoise(sums, 8, rec, iterations=it)
        assert same_bits(device_denoise(gpu, sums, None, 8, rec, iterations=it), want), f"iterations {it}, uniform spp"


def test_device_filter_scratch_across_sizes(gpu):
    """The per-device scratch only grows: a small frame after a large one, and the large one again."""
    for which in [(70, 45), (33, 17), (70, 45)]:
        sums, counts, rec = frame_of(gpu, which)
        assert same_bits(device_denoise(gpu, sums, counts, 0, rec), gpu.denoise(sums, counts, rec))


def test_device_filter_other_parameters(gpu):
    sums, counts, rec = frame_of(gpu, (70, 45))
    p = dict(iterations=4, sigma_color=0.35, sigma_plane=0.5, normal_power_log2=2)
    assert same_bits(device_denoise(gpu, sums, counts, 0, rec, **p), gpu.denoise(sums, counts, rec, **p))


def test_host_arrays_to_bytes(gpu):
    """rt_denoise_frame_u8 (the CLI's several-GPU seam): the host function's frame, finished at spp 1."""
    for which, it in [((70, 45), 5), ("real", 3)]:
        sums, counts, rec = frame_of(gpu, which)
        assert np.array_equal(gpu.denoise_frame_u8(sums, counts, rec, iterations=it),
                              gpu.tonemap(gpu.denoise(sums, counts, rec, iterations=it), 1))
        assert np.array_equal(gpu.denoise_frame_u8(sums, 8, rec, iterations=it),
                              gpu.tonemap(gpu.denoise(sums, 8, rec, iterations=it), 1))


# ------------------------------------------------------------------------ accumulator
def snapshot(acc, pending):
    s = dict(sums=acc.sums(), state=acc.state(), counts=acc.counts(), frame=acc.frame(), range=acc.sample_range)
    if pending:
        s["selection"] = acc.selection().copy()
    return s


def assert_unchanged(acc, before, pending):
    after = snapshot(acc, pending)
    assert same_bits(after["sums"], before["sums"]) and np.array_equal(after["state"], before["state"])
    assert np.array_equal(after["counts"], before["counts"]) and np.array_equal(after["frame"], before["frame"])
    assert after["range"] == before["range"]
    if pending:
        assert np.array_equal(after["selection"], before["selection"])


def check_denoised_frame(gpu, acc, rec, pending=False, **params):
    before = snapshot(acc, pending)
    got = acc.frame(denoise=params or True)
    want = gpu.tonemap(gpu.denoise(before["sums"], before["counts"], rec, **params), 1)
    assert np.array_equal(got, want), f"{(got != want).any(-1).sum()} pixels differ"
    assert_unchanged(acc, before, pending)
    return got


@pytest.mark.parametrize("fast", [False, True])
def test_accumulator_denoised_frame(gpu, fast):
    scene = scene_of(gpu, "cornell", 64, 64)
    rec = scene.gbuffer()["records"]
    acc = scene.accumulator(fast=fast)
    try:
        acc.add(4)
        first = check_denoised_frame(gpu, acc, rec)
        assert (first != acc.frame()).any(), "the filter changed nothing"
        check_denoised_frame(gpu, acc, rec, iterations=2, sigma_color=0.5)
        # a subset pass: the counts differ and a window has been refined; then a pending selection
        acc.mark()
        assert acc.select(12, window=(8, 8, 40, 40)) == 32 * 32
        acc.add_selected()
        assert acc.sample_range == (4, 12)
        n = acc.select(16, window=(0, 0, 20, 20))
        assert n == 400
        check_denoised_frame(gpu, acc, rec, pending=True)
        assert acc.add_selected()["pixels"] == n   # the pending selection is still the one made
        check_denoised_frame(gpu, acc, rec)
    finally:
        acc.free()


@pytest.mark.parametrize("fast", [False, True])
def test_refused_call_leaves_no_half_made_gbuffer(gpu, fast):
    """A call refused for its parameters, as the first denoised frame of a fresh accumulator, must
    not leave a G-buffer behind that was allocated and never rendered: the good calls after it are
    the host filter's frame."""
    scene = scene_of(gpu, "cornell", 64, 64)
    rec = scene.gbuffer()["records"]
    acc = scene.accumulator(fast=fast)
    try:
        acc.add(4)
        for bad in (dict(iterations=7), dict(normal_power_log2=17), dict(sigma_color=float("nan"))):
            with pytest.raises(gpu.RtError, match="rt_accum_frame_u8_denoised"):
                acc.frame(denoise=bad)
        check_denoised_frame(gpu, acc, rec)
        with pytest.raises(gpu.RtError):
            acc.frame(denoise=dict(sigma_plane=float("inf")))
        check_denoised_frame(gpu, acc, rec, iterations=3)
    finally:
        acc.free()


def test_accumulator_denoised_frame_needs_the_whole_frame(gpu):
    scene = scene_of(gpu, "cornell", 64, 64)
    acc = scene.accumulator(rank=0, world=2)
    try:
        acc.add(1)
        with pytest.raises(gpu.RtError, match="rt_denoise_device"):
            acc.frame(denoise=True)
        assert acc.frame().shape == (32, 64, 3)
    finally:
        acc.free()
    acc = scene.accumulator()
    try:
        with pytest.raises(gpu.RtError, match="no samples"):
            acc.frame(denoise=True)
    finally:
        acc.free()


# ------------------------------------------------------------------------ it denoises
def rmse_ratio(gpu, name, w, h, spp=8, truth_spp=2048):
    """RMSE against the GPU's own parity render at truth_spp samples (existing code, pinned to the
    reference), over hit pixels with finite values, means clamped to [0, 4] so that one firefly
    does not decide it: (raw, denoised)."""
    scene = scene_of(gpu, name, w, h)
    truth = scene.render_sums(truth_spp)[0] * (f32(1) / f32(truth_spp))
    sums = scene.render_sums(spp)[0]
    g = scene.gbuffer()
    raw = sums * (f32(1) / f32(spp))
    den = gpu.denoise(sums, spp, g)
    use = (g["prim"] >= 0) & np.isfinite(raw).all(-1) & np.isfinite(den).all(-1) & np.isfinite(truth).all(-1)
    assert use.mean() > 0.5

    def rmse(x):
        d = np.clip(x[use].astype(np.float64), 0, 4) - np.clip(truth[use].astype(np.float64), 0, 4)
        return float(np.sqrt((d * d).mean()))

    return rmse(raw), rmse(den)


def test_it_denoises_cornell(gpu):
    raw, den = rmse_ratio(gpu, "cornell", 64, 64)
    print(f"\ncornell 64x64, 8 samples against 2048: RMSE raw {raw:.5f}, denoised {den:.5f}, ratio {den / raw:.3f}")
    assert den < raw


def test_texture_detail_ratio_sponza_mini(gpu):
    """Recorded only: whether texture detail survives the demodulation."""
    raw, den = rmse_ratio(gpu, "sponza_mini", 64, 36)
    print(f"\nsponza_mini 64x36, 8 samples against 2048: RMSE raw {raw:.5f}, denoised {den:.5f}, ratio {den / raw:.3f}")
    assert np.isfinite(raw) and np.isfinite(den)
