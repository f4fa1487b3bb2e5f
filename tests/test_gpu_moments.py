"""Moments accumulators on the GPU (include/rt_hw.h rt_accum_create_fast_moments): after any
sequence of full and subset passes a pixel with n samples holds, bit for bit, the fast fold of its
samples' squared colours, the colours being the CPU ground truth of tests/native/moments_host.cpp
(pinned to the oracle by tests/test_moments.py); its sums stay a fast accumulator's.  On that rest
the measured variance, the variance selection rule, the measured-variance frame and the new
checkpoint kind.  Every comparison is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

import rtref
from moments_util import (MOMENT_MAGIC, colours, f32, np_fold, np_relative_error, np_variance_records, squares, twin)
from test_gpu_accum import SOLUTION, gpu   # noqa: F401  (fixture)
from test_gpu_fast_accum import cornell_steps, fast_sums, ref_scene
from test_gpu_select import _pgm, add_selected, select

pytestmark = pytest.mark.gpu
bits = rtref.bits


@pytest.fixture(scope="module")
def mh(tmp_path_factory):
    return twin(tmp_path_factory)


def truth(gpu, mh, name, w, h, n, c, n_max=None):
    """(S, Q, total2, open2) of the whole frame at (n, c), each (H * W, 3), from the ground truth."""
    arrays = ref_scene(gpu, name, w, h)[1]
    x = colours(gpu, mh, name, w, h, max(n, n_max or 0, 1), arrays=arrays)
    if n == 0:
        z = np.zeros((w * h, 3), f32)
        return z, z, z, z
    total2, open2, Q = np_fold(squares(x), n, c)
    return np_fold(x, n, c)[2], Q, total2, open2


def records(acc, tmp_path):
    """The accumulator's fast records and moment records, (P, 8) uint32 each, from its checkpoint."""
    path = str(tmp_path / "records.acc")
    acc.save(path)
    raw = open(path, "rb").read()
    P = len(acc.rows) * acc._scene.width
    assert raw[:8] == MOMENT_MAGIC and len(raw) == 128 + 64 * P
    return (np.frombuffer(raw, "<u4", 8 * P, 128).reshape(P, 8), np.frombuffer(raw, "<u4", 8 * P, 128 + 32 * P).reshape(P, 8))


def check_moments(gpu, mh, acc, key, counts, c, tmp_path, rows=None, n_max=None):
    """Per distinct count n: the pixels at n hold the ground truth's sums, moments and moment record."""
    name, w, h = key
    counts = np.asarray(counts).reshape(-1)
    got_S, got_Q = acc.sums().reshape(-1, 3), acc.moments().reshape(-1, 3)
    fast, mom = records(acc, tmp_path)
    assert np.array_equal(fast[:, 1], counts)
    assert not mom[:, 6:].any()
    pick = slice(None) if rows is None else (np.asarray(rows)[:, None] * w + np.arange(w)[None, :]).reshape(-1)
    for n in np.unique(counts):
        S, Q, total2, open2 = (a[pick] for a in truth(gpu, mh, name, w, h, int(n), c, n_max))
        at = counts == n
        assert np.array_equal(bits(got_S[at]), bits(S[at])), f"sums differ at {n} samples"
        bad = (bits(got_Q[at]) != bits(Q[at])).any(1)
        assert bad.sum() == 0, f"{bad.sum()} of {at.sum()} pixels' moments differ from the fold of squares at ({n}, {c})"
        assert np.array_equal(mom[at, 0:3], bits(total2[at])) and np.array_equal(mom[at, 3:6], bits(open2[at]))
        if n % c == 0:
            assert not mom[at, 3:6].any(), "open2 words at a chunk boundary"
    return got_S, got_Q


# (scene, W, H, c, passes): as test_gpu_fast_accum.py's, for the second partial
PASSES = [("cornell", 64, 64, 3, (2, 5, 1, 4)), ("cornell", 33, 17, 2, (1, 1, 3)), ("cornell", 64, 64, 1, (2, 5)),
          ("cornell", 64, 64, 8, (3, 3, 3)), ("sponza_mini", 64, 36, 2, (3, 1))]


@pytest.mark.parametrize("name,w,h,c,passes", PASSES)
def test_passes_across_chunk_boundaries(gpu, oracle, mh, tmp_path, name, w, h, c, passes):
    scene, arrays = ref_scene(gpu, name, w, h)
    acc = scene.accumulator(fast=True, fast_chunk=c, moments=True)
    plain = scene.accumulator(fast=True, fast_chunk=c)
    try:
        assert acc.has_moments and not plain.has_moments and acc.fast_chunk == c
        assert not acc.moments().any() and not acc.sums().any()
        with pytest.raises(gpu.RtError, match="no moments"):
            plain.moments()
        assert plain.device_moments_ptr == 0 and acc.device_moments_ptr != 0
        n = 0
        some_open = False
        for k in passes:
            stats = acc.add(k)
            plain.add(k)
            n += k
            assert stats["schedule"] == gpu.SCHED_FAST and stats["samples"] == w * h * k
            S, Q = check_moments(gpu, mh, acc, (name, w, h), np.full(w * h, n), c, tmp_path, n_max=sum(passes))
            assert np.array_equal(bits(S), bits(fast_sums(oracle, arrays, (name, w, h), n, c).reshape(-1, 3)))
            assert np.array_equal(bits(S), bits(plain.sums().reshape(-1, 3)))
            assert np.array_equal(acc.state(), plain.state())
            assert (Q > 0).any() and np.isfinite(Q).all()
            some_open |= n % c != 0
        assert some_open == (c != 1)
    finally:
        acc.free()
        plain.free()


def test_subset_passes_with_unequal_starts(gpu, mh, tmp_path):
    key = ("cornell", 64, 64)
    scene, _ = ref_scene(gpu, *key)
    acc = scene.accumulator(fast=True, fast_chunk=3, moments=True)
    try:
        acc.add(2)
        counts = np.full(64 * 64, 2, np.int32)
        for target, kw in cornell_steps():
            lst, before = select(acc, target, **kw)
            mom_before, Q_before = records(acc, tmp_path)[1], acc.moments().reshape(-1, 3)
            add_selected(acc, lst, before, target)
            counts[lst] = target
            check_moments(gpu, mh, acc, key, counts, 3, tmp_path, n_max=9)
            keep = np.ones(64 * 64, bool)
            keep[lst] = False
            assert keep.any() or target == 9
            assert np.array_equal(records(acc, tmp_path)[1][keep], mom_before[keep]), "an unlisted pixel's moment record changed"
            assert np.array_equal(bits(acc.moments().reshape(-1, 3)[keep]), bits(Q_before[keep]))
        assert (counts == 9).all()
    finally:
        acc.free()


def test_more_than_128_units_in_one_pass(gpu, mh, tmp_path):
    key = ("cornell", 16, 8)
    scene, _ = ref_scene(gpu, *key)
    acc = scene.accumulator(fast=True, fast_chunk=1, moments=True)
    try:
        acc.add(130)   # 130 units per pixel: two launches, 128 + 2
        check_moments(gpu, mh, acc, key, np.full(128, 130), 1, tmp_path, n_max=131)
        acc.add(1)
        check_moments(gpu, mh, acc, key, np.full(128, 131), 1, tmp_path, n_max=131)
    finally:
        acc.free()


@pytest.mark.parametrize("world", [2, 3])
def test_shards(gpu, mh, tmp_path, world):
    key = ("sponza_mini", 64, 36)
    scene, _ = ref_scene(gpu, *key)
    for rank in range(world):
        acc = scene.accumulator(rank=rank, world=world, row_block=4, fast=True, fast_chunk=2, moments=True)
        try:
            n = 0
            for k in (3, 2):
                acc.add(k)
                n += k
                check_moments(gpu, mh, acc, key, np.full(len(acc.rows) * 64, n), 2, tmp_path, rows=acc.rows, n_max=5)
            # the shard's variance: its own rows' records
            rec = scene.gbuffer(rank=rank, world=world, row_block=4)["records"]
            want = np_variance_records(np.full(len(acc.rows) * 64, n), acc.sums().reshape(-1, 3), acc.moments().reshape(-1, 3), rec)
            assert np.array_equal(bits(acc.variance().reshape(-1)), bits(want)) and (want > 0).any()
        finally:
            acc.free()


def device_variance(gpu, acc, counts, spp, rec, w, h):
    """rt_variance_from_moments_device on the accumulator's own device sums and moments."""
    import torch
    d_g = torch.from_numpy(np.ascontiguousarray(rec, f32)).cuda()
    d_c = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda() if counts is not None else None
    d_o = torch.full((h * w + 64,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    gpu.variance_from_moments_device(acc.device_sums_ptr, acc.device_moments_ptr, d_c.data_ptr() if d_c is not None else 0, spp, w, h,
                                     d_g.data_ptr(), d_o.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_o.cpu().numpy()
    assert (out[h * w:] == -7.0).all(), "wrote past the frame"
    return out[:h * w]


def test_variance_device_host_and_accumulator(gpu, mh):
    key = ("cornell", 64, 64)
    scene, _ = ref_scene(gpu, *key)
    rec = scene.gbuffer()["records"]
    acc = scene.accumulator(fast=True, fast_chunk=3, moments=True)
    try:
        acc.add(2)
        for step, (target, kw) in enumerate([(0, None)] + cornell_steps()[:2]):
            if kw is not None:
                acc.select(target, **kw)
                acc.add_selected()
            counts, S, Q = acc.counts(), acc.sums(), acc.moments()
            want = np_variance_records(counts.reshape(-1), S.reshape(-1, 3), Q.reshape(-1, 3), rec)
            host = gpu.variance_from_moments(S, Q, counts, rec)
            assert np.array_equal(bits(host.reshape(-1)), bits(want))
            assert np.array_equal(bits(device_variance(gpu, acc, counts, 0, rec, 64, 64)), bits(want))
            assert np.array_equal(bits(acc.variance().reshape(-1)), bits(want))
            assert (want > 0).sum() > 1000 and np.isfinite(want).all()
            if step == 0:   # uniform counts: NULL + spp is the same
                assert np.array_equal(bits(device_variance(gpu, acc, None, 2, rec, 64, 64)), bits(want))
                assert np.array_equal(bits(gpu.variance_from_moments(S, Q, 2, rec).reshape(-1)), bits(want))
        assert set(np.unique(acc.counts())) == {2, 5, 7}
    finally:
        acc.free()


# (scene, W, H, threshold, pixels the rule selects): the threshold chosen on the CPU from the ground
# truth at (8, 3) so that the guards below hold; the count pinned
RULE_CASES = [("cornell", 64, 64, 0.5, 1385), ("sponza_mini", 64, 36, 0.5, 1624)]


def guarded_variance_rule(S, Q, n, threshold):
    """The numpy rule's list with test_select.guarded_rule's guards: no estimate within 1e-4
    relative of the threshold, none non-finite, a selected share in [0.2, 0.8]."""
    e = np_relative_error(np.full(len(S), n), S, Q)
    assert np.isfinite(e).all()
    assert (np.abs(e.astype(np.float64) - threshold) > 1e-4 * threshold).all(), "an estimate too close to the threshold"
    want = np.nonzero(e > f32(threshold))[0]
    assert 0.2 <= len(want) / len(S) <= 0.8, len(want) / len(S)
    return want


@pytest.mark.parametrize("name,w,h,threshold,count", RULE_CASES)
def test_select_variance(gpu, mh, tmp_path, name, w, h, threshold, count):
    key = (name, w, h)
    scene, _ = ref_scene(gpu, *key)
    S, Q, _, _ = truth(gpu, mh, name, w, h, 8, 3, n_max=12)
    want = guarded_variance_rule(S, Q, 8, threshold)
    print(f"{name}: the variance rule selects {len(want)} of {w * h} pixels at threshold {threshold}")
    assert len(want) == count
    acc = scene.accumulator(fast=True, fast_chunk=3, moments=True)
    plain = scene.accumulator(fast=True, fast_chunk=3)
    try:
        acc.add(8)
        n = acc.select_variance(12, threshold=threshold)
        lst = acc.selection()
        assert n == len(lst) and np.array_equal(lst, want)
        # a mark set before must not change the list; threshold 0 and a window as rt_accum_select
        acc.mark()
        assert acc.select_variance(12, threshold=threshold) == len(want) and np.array_equal(acc.selection(), want)
        assert acc.select_variance(12) == w * h
        assert acc.select_variance(8, threshold=threshold) == 0
        assert acc.select_variance(12, window=(0, 0, 10, 10)) == 100
        acc.select_variance(12, threshold=threshold)
        before = acc.state()[:, 0].astype(np.int64)
        add_selected(acc, want, before, 12)
        counts = np.full(w * h, 8, np.int32)
        counts[want] = 12
        check_moments(gpu, mh, acc, key, counts, 3, tmp_path, n_max=12)
        with pytest.raises(gpu.RtError, match="no pending selection"):
            acc.add_selected()
        plain.add(2)
        with pytest.raises(gpu.RtError, match="rt_accum_select_variance.*no moments"):
            plain.select_variance(4)
        with pytest.raises(gpu.RtError, match="rt_accum_variance.*no moments"):
            plain.variance()
        with pytest.raises(gpu.RtError, match="rt_accum_frame_u8_guided_measured.*no moments"):
            plain.frame(denoise=True, guided=True, measured=True)
    finally:
        acc.free()
        plain.free()


def test_measured_frame(gpu):
    scene, _ = ref_scene(gpu, "cornell", 64, 64)
    rec = scene.gbuffer()["records"]
    acc = scene.accumulator(fast=True, fast_chunk=2, moments=True)
    try:
        with pytest.raises(gpu.RtError, match="no samples"):
            acc.frame(denoise=True, guided=True, measured=True)
        acc.add(4)
        acc.select(8, window=(8, 8, 40, 40))
        acc.add_selected()
        for params in (dict(), dict(iterations=2, sigma_var=0.5, firefly=-1.0)):
            before = dict(state=acc.state(), sums=acc.sums(), moments=acc.moments(), counts=acc.counts())
            got = acc.frame(denoise=params or True, guided=True, measured=True)
            V = acc.variance()
            want = gpu.tonemap(gpu.denoise_guided(before["sums"], before["counts"], rec, variance=V, **params), 1)
            assert np.array_equal(got, want), f"{(got != want).any(-1).sum()} pixels differ"
            assert np.array_equal(acc.state(), before["state"]) and np.array_equal(acc.counts(), before["counts"])
            assert np.array_equal(bits(acc.sums()), bits(before["sums"])) and np.array_equal(bits(acc.moments()), bits(before["moments"]))
        spatial = acc.frame(denoise=True, guided=True)
        assert (spatial != acc.frame(denoise=True, guided=True, measured=True)).any(), "the measured variance changed nothing"
        with pytest.raises(gpu.RtError, match="rt_accum_frame_u8_guided_measured"):
            acc.frame(denoise=dict(iterations=7), guided=True, measured=True)
    finally:
        acc.free()
    half = scene.accumulator(rank=0, world=2, fast=True, moments=True)
    try:
        half.add(2)
        with pytest.raises(gpu.RtError, match="world = 1"):
            half.frame(denoise=True, guided=True, measured=True)
    finally:
        half.free()


def test_save_and_load_mid_chunk_and_with_unequal_counts(gpu, mh, tmp_path):
    key = ("cornell", 64, 64)
    scene, _ = ref_scene(gpu, *key)
    path = str(tmp_path / "moments.acc")
    acc = scene.accumulator(fast=True, fast_chunk=3, moments=True)
    acc.add(4)   # (saved inside chunk 1)
    acc.select(7, window=(10, 20, 40, 50))
    acc.add_selected()
    counts = acc.counts()
    assert set(np.unique(counts)) == {4, 7}
    state, S, Q, recs = acc.state(), acc.sums(), acc.moments(), records(acc, tmp_path)
    assert recs[1][:, 3:6].any()
    acc.save(path)
    raw = open(path, "rb").read()
    assert raw[:8] == MOMENT_MAGIC and len(raw) == 128 + 64 * 64 * 64
    assert np.frombuffer(raw[8:12], "<u4")[0] == 1 and np.frombuffer(raw[120:128], "<i4").tolist() == [3, 0]
    acc.select(9)
    acc.add_selected()
    uninterrupted = (acc.sums(), acc.moments())
    acc.free()
    acc = gpu.Accumulator.load(scene, path)
    try:
        assert acc.has_moments and acc.fast_chunk == 3 and acc.sample_range == (4, 7)
        assert np.array_equal(acc.state(), state) and np.array_equal(acc.counts(), counts)
        assert np.array_equal(bits(acc.sums()), bits(S)) and np.array_equal(bits(acc.moments()), bits(Q))
        again = records(acc, tmp_path)
        assert np.array_equal(again[0], recs[0]) and np.array_equal(again[1], recs[1])
        acc.select(9)
        acc.add_selected()
        assert np.array_equal(bits(acc.sums()), bits(uninterrupted[0])) and np.array_equal(bits(acc.moments()), bits(uninterrupted[1]))
        check_moments(gpu, mh, acc, key, np.full(64 * 64, 9), 3, tmp_path, n_max=12)
    finally:
        acc.free()
    # a fast file still loads as a fast accumulator, without moments
    plain = scene.accumulator(fast=True, fast_chunk=3)
    plain.add(4)
    fast_path = str(tmp_path / "fast.acc")
    plain.save(fast_path)
    plain.free()
    plain = gpu.Accumulator.load(scene, fast_path)
    try:
        assert not plain.has_moments and plain.fast_chunk == 3
    finally:
        plain.free()
    other, _ = ref_scene(gpu, "cornell", 33, 17)
    with pytest.raises(gpu.RtError, match="64 x 64"):
        gpu.Accumulator.load(other, path)


# ---------------------------------------------------------------- CLI
def _cli(out, samples, ok=True, **env_add):
    env = dict(os.environ)
    for k in ("RT_PASS_SPP", "RT_CHECKPOINT", "RT_ADAPT", "RT_COUNTS_OUT", "RT_FAST", "RT_MOMENTS", "RT_VARIANCE_OUT", "RT_DENOISE",
              "RT_DENOISE_GUIDED"):
        env.pop(k, None)
    env["RT_GPUS"] = "1"
    env.update(env_add)
    r = subprocess.run([SOLUTION, rtref.scene_path("cornell"), "33", "17", str(samples), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def _pfm(path, w, h):
    data = open(path, "rb").read()
    header = b"Pf\n%d %d\n-1.0\n" % (w, h)
    assert data.startswith(header) and len(data) == len(header) + 4 * w * h
    return np.frombuffer(data, "<f4", w * h, len(header)).reshape(h, w)[::-1]


def test_cli_moments(gpu, tmp_path):
    out, cnt, var = str(tmp_path / "out.ppm"), str(tmp_path / "counts.pgm"), str(tmp_path / "v.pfm")
    assert "RT_MOMENTS needs a pass mode" in _cli(out, 3, ok=False, RT_MOMENTS="1", RT_FAST="2")
    assert "RT_MOMENTS needs RT_FAST" in _cli(out, 3, ok=False, RT_MOMENTS="1", RT_PASS_SPP="1")
    assert "RT_VARIANCE_OUT needs RT_MOMENTS" in _cli(out, 3, ok=False, RT_FAST="2", RT_PASS_SPP="1", RT_VARIANCE_OUT=var)
    # the frames of a moments run are the fast run's, byte for byte
    plain = str(tmp_path / "plain.ppm")
    _cli(plain, 3, RT_FAST="2", RT_PASS_SPP="1")
    _cli(out, 3, RT_FAST="2", RT_PASS_SPP="1", RT_MOMENTS="1", RT_VARIANCE_OUT=var)
    assert open(out, "rb").read() == open(plain, "rb").read()
    # the accumulator the CLI ran: the CLI's own loader, one shard
    scene = gpu.Scene.load(rtref.scene_path("cornell"), 33, 17, 3)
    acc = scene.accumulator(fast=True, fast_chunk=2, moments=True)
    try:
        for _ in range(3):
            acc.add(1)
        V = acc.variance()
        assert np.array_equal(bits(_pfm(var, 33, 17)), bits(V)) and (V > 0).any()
        # RT_DENOISE_GUIDED: the measured variance into the filter
        _cli(out, 3, RT_FAST="2", RT_PASS_SPP="1", RT_MOMENTS="1", RT_DENOISE_GUIDED="3")
        want = gpu.tonemap(gpu.denoise_guided(acc.sums(), 3, scene.gbuffer()["records"], variance=V, iterations=3), 1)
        assert open(out, "rb").read() == b"P6\n33 17\n255\n" + want.tobytes()
        spatial = str(tmp_path / "spatial.ppm")
        _cli(spatial, 3, RT_FAST="2", RT_PASS_SPP="1", RT_DENOISE_GUIDED="3")
        assert open(spatial, "rb").read() != open(out, "rb").read()
    finally:
        acc.free()
    # adaptive: threshold 0 raises every pixel every round; one nothing exceeds stops after the two first passes
    _cli(out, 3, RT_FAST="2", RT_MOMENTS="1", RT_ADAPT="0", RT_PASS_SPP="1", RT_COUNTS_OUT=cnt)
    assert open(out, "rb").read() == open(plain, "rb").read() and (_pgm(cnt, 33, 17) == 3).all()
    stdout = _cli(out, 3, RT_FAST="2", RT_MOMENTS="1", RT_ADAPT="1e30", RT_PASS_SPP="1", RT_COUNTS_OUT=cnt)
    assert "refined" not in stdout and (_pgm(cnt, 33, 17) == 2).all()
    # a moments checkpoint resumes to identical bytes, and only into its own kind and chunk
    prefix = str(tmp_path / "ck")
    _cli(out, 2, RT_FAST="2", RT_PASS_SPP="1", RT_MOMENTS="1", RT_CHECKPOINT=prefix)
    assert open(prefix + ".0of1", "rb").read(8) == MOMENT_MAGIC
    stdout = _cli(out, 3, RT_FAST="2", RT_PASS_SPP="1", RT_MOMENTS="1", RT_CHECKPOINT=prefix, RT_VARIANCE_OUT=var)
    assert "Resumed from" in stdout and "at 2 samples" in stdout
    assert open(out, "rb").read() == open(plain, "rb").read() and np.array_equal(bits(_pfm(var, 33, 17)), bits(V))
    stderr = _cli(out, 3, ok=False, RT_FAST="2", RT_PASS_SPP="1", RT_CHECKPOINT=prefix)
    assert "checkpoint" in stderr and "fast accumulator with chunks of 2 and moments" in stderr and "without RT_MOMENTS" in stderr
    stderr = _cli(out, 3, ok=False, RT_FAST="3", RT_PASS_SPP="1", RT_MOMENTS="1", RT_CHECKPOINT=prefix)
    assert "checkpoint" in stderr and "chunks of 2 and moments" in stderr and "RT_FAST=3 with RT_MOMENTS" in stderr
    # and a fast checkpoint does not resume into a moments run
    fast_prefix = str(tmp_path / "fck")
    _cli(out, 2, RT_FAST="2", RT_PASS_SPP="1", RT_CHECKPOINT=fast_prefix)
    stderr = _cli(out, 3, ok=False, RT_FAST="2", RT_PASS_SPP="1", RT_MOMENTS="1", RT_CHECKPOINT=fast_prefix)
    assert "fast accumulator with chunks of 2, the run asks for RT_FAST=2 with RT_MOMENTS" in stderr


def test_render_adaptive_moments(gpu, mh):
    key = ("cornell", 64, 64)
    scene, _ = ref_scene(gpu, *key)
    sums, counts, frame = scene.render_adaptive(8, 16, 4, 0.5, fast=True, fast_chunk=2, moments=True)
    assert counts.min() == 8 and set(np.unique(counts).tolist()) <= {8, 12, 16} and len(np.unique(counts)) > 1
    for n in np.unique(counts):
        at = (counts == n).reshape(-1)
        want = truth(gpu, mh, *key, int(n), 2, n_max=16)[0]
        assert np.array_equal(bits(sums.reshape(-1, 3)[at]), bits(want[at]))
    assert np.array_equal(frame, gpu.tonemap_counts(sums, counts))
