"""Fast-mode accumulators on the GPU (include/rt_hw.h rt_accum_create_fast): after any sequence
of full and subset passes of any sizes, a pixel that has n samples holds, bit for bit, the CPU
oracle's fast sum of n samples in chunks of the accumulator's c (rt_oracle_render_fast), wherever
the passes stopped, in or between chunks.  Every comparison is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

import rtref
from test_gpu_accum import SOLUTION, gpu   # noqa: F401  (fixture)
from test_gpu_select import _pgm, add_selected, check_invariant, select
from test_select import THRESHOLD, guarded_rule

pytestmark = pytest.mark.gpu
f32 = np.float32

_scenes, _fast = {}, {}


def ref_scene(gpu, name, w, h):
    """(scene on the reference's own flattened arrays, those arrays), made once per frame."""
    if (name, w, h) not in _scenes:
        arrays = rtref.ref_arrays(gpu, name, w, h, 4)
        _scenes[name, w, h] = (gpu.Scene.from_view(arrays), arrays)
    return _scenes[name, w, h]


def fast_sums(oracle, arrays, key, n, c):
    """The oracle's fast sums of the whole frame at (n, c), (H, W, 3), made once and never changed."""
    if (key, n, c) not in _fast:
        h, w = int(arrays["height"]), int(arrays["width"])
        out = oracle.render_fast(arrays, n, c)[0].reshape(h, w, 3) if n else np.zeros((h, w, 3), f32)
        out.setflags(write=False)
        _fast[key, n, c] = out
    return _fast[key, n, c]


def check_pass(gpu, oracle, acc, arrays, key, n, c, stats, added, rows=None):
    """After a full pass that brought every pixel to n samples."""
    want = fast_sums(oracle, arrays, key, n, c)
    want = want if rows is None else want[rows]
    got = acc.sums()
    bad = (rtref.bits(got) != rtref.bits(want)).any(2)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ from the oracle at ({n}, {c})"
    st = acc.state()
    assert (st[:, 0] == n).all() and acc.samples == n and acc.sample_range == (n, n)
    if n % c == 0:
        assert not st[:, 1:].any(), "open words at a chunk boundary"
    else:   # reported = total + open, total being the sum at the last boundary
        total = fast_sums(oracle, arrays, key, n - n % c, c)
        total = (total if rows is None else total[rows]).reshape(-1, 3)
        opn = st[:, 1:].copy().view(f32)
        assert st[:, 1:].any()
        with np.errstate(invalid="ignore"):
            assert np.array_equal(rtref.bits((total + opn).astype(f32)), rtref.bits(got.reshape(-1, 3)))
    assert stats["schedule"] == gpu.SCHED_FAST and stats["order_ms"] == 0
    assert stats["pixels"] == st.shape[0] and stats["samples"] == st.shape[0] * added


# (scene, W, H, c, passes): passes that end inside a chunk, lie wholly inside an open chunk, end on a
# boundary and carry `open` over two passes (c = 3: counts 2, 7, 8, 12); c = 1 (never open) and
# c = 8 (open throughout, counts 3, 6, 9); frames whose items are no multiple of 64; textures
PASSES = [("cornell", 64, 64, 3, (2, 5, 1, 4)), ("cornell", 64, 64, 1, (2, 5, 1, 4)), ("cornell", 64, 64, 8, (3, 3, 3)),
          ("cornell", 33, 17, 2, (1, 1, 3)), ("sponza_mini", 64, 36, 2, (3, 1)), ("practice6_1", 96, 96, 4, (2, 2))]


@pytest.mark.parametrize("name,w,h,c,passes", PASSES)
def test_passes_across_chunk_boundaries(gpu, oracle, name, w, h, c, passes):
    scene, arrays = ref_scene(gpu, name, w, h)
    acc = scene.accumulator(fast=True, fast_chunk=c)
    assert acc.fast_chunk == c and acc.samples == 0 and not acc.sums().any() and not acc.state().any()
    n = 0
    for k in passes:
        stats = acc.add(k)
        n += k
        check_pass(gpu, oracle, acc, arrays, (name, w, h), n, c, stats, k)
    acc.free()


def test_default_chunk_is_two_and_parity_reports_zero(gpu):
    scene, _ = ref_scene(gpu, "cornell", 33, 17)
    acc = scene.accumulator(fast=True)
    assert acc.fast_chunk == 2
    acc.free()
    acc = scene.accumulator()
    assert acc.fast_chunk == 0
    acc.free()


@pytest.mark.parametrize("n,c", [(8, 3), (5, 1)])
def test_one_shot_equivalence(gpu, n, c):
    scene, _ = ref_scene(gpu, "cornell", 64, 64)
    want, st = scene.render_sums(n, fast=True, fast_chunk=c)
    assert st["schedule"] == gpu.SCHED_FAST
    acc = scene.accumulator(fast=True, fast_chunk=c)
    acc.add(n)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(want))
    acc.free()


def test_more_than_128_units_in_one_pass(gpu, oracle):
    scene, arrays = ref_scene(gpu, "cornell", 16, 8)
    acc = scene.accumulator(fast=True, fast_chunk=1)
    stats = acc.add(130)   # 130 units per pixel: two launches, 128 + 2
    check_pass(gpu, oracle, acc, arrays, ("cornell", 16, 8), 130, 1, stats, 130)
    stats = acc.add(1)
    check_pass(gpu, oracle, acc, arrays, ("cornell", 16, 8), 131, 1, stats, 1)
    acc.free()


def run_subsets(gpu, oracle, acc, arrays, key, c, first, steps, rows=None):
    """add(first), then the subset steps [(target, select arguments)]; after each the list's
    properties (before it renders), the untouched pixels, the stats and the invariant."""
    w = int(arrays["width"])
    rows = acc.rows if rows is None else rows
    ys, xs = np.meshgrid(rows, np.arange(w), indexing="ij")
    sums_at = lambda n: fast_sums(oracle, arrays, key, n, c)
    acc.add(first)
    counts = np.full((len(rows), w), first, np.int32)
    check_invariant(acc, counts, sums_at, rows)
    starts = []
    for target, kw in steps:
        lst, before = select(acc, target, **kw)
        chosen = counts < target
        if "window" in kw:
            x0, y0, x1, y1 = kw["window"]
            chosen &= (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
        if "mask" in kw:
            chosen &= kw["mask"] != 0
        assert np.array_equal(lst, np.nonzero(chosen.reshape(-1))[0])
        starts.append(set(np.unique(counts[chosen]).tolist()))
        stats = add_selected(acc, lst, before, target)   # (pixels, samples, order_ms, the unlisted records and sums)
        assert stats["schedule"] == gpu.SCHED_FAST
        counts = np.where(chosen, target, counts).astype(np.int32)
        check_invariant(acc, counts, sums_at, rows)
        st = acc.state()
        at_boundary = st[:, 0] % c == 0
        assert not st[at_boundary, 1:].any()
    return counts, starts


def cornell_steps():
    even = np.zeros((64, 64), np.uint8)
    even[:, ::2] = 1
    return [(5, dict(mask=even)), (7, dict(window=(10, 20, 40, 50))), (9, dict())]


def test_subset_passes_with_unequal_starts(gpu, oracle):
    scene, arrays = ref_scene(gpu, "cornell", 64, 64)
    acc = scene.accumulator(fast=True, fast_chunk=3)
    counts, starts = run_subsets(gpu, oracle, acc, arrays, ("cornell", 64, 64), 3, 2, cornell_steps())
    # the last list held items with different unit counts (2 -> 9: chunks 0, 1, 2; 7 -> 9: chunk 2
    # only, so units that start nothing)
    assert starts[-1] == {2, 5, 7}
    assert (counts == 9).all() and acc.sample_range == (9, 9)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(fast_sums(oracle, arrays, ("cornell", 64, 64), 9, 3)))
    stats = acc.add(1)   # (a full pass after subset passes)
    check_pass(gpu, oracle, acc, arrays, ("cornell", 64, 64), 10, 3, stats, 1)
    acc.free()


@pytest.mark.parametrize("world", [2, 3])
def test_shards(gpu, oracle, world):
    scene, arrays = ref_scene(gpu, "sponza_mini", 64, 36)
    for rank in range(world):
        acc = scene.accumulator(rank=rank, world=world, row_block=4, fast=True, fast_chunk=2)
        n = 0
        for k in (3, 2):
            stats = acc.add(k)
            n += k
            check_pass(gpu, oracle, acc, arrays, ("sponza_mini", 64, 36), n, 2, stats, k, rows=acc.rows)
        acc.free()


# (scene, W, H, pixels the rule selects: from the oracle's fast sums at (4, 3) and (8, 3))
RULE_CASES = [("cornell", 64, 64, 2261), ("sponza_mini", 64, 36, 1558)]


@pytest.mark.parametrize("name,w,h,count", RULE_CASES)
def test_adaptive_rule_on_fast_sums(gpu, oracle, name, w, h, count):
    scene, arrays = ref_scene(gpu, name, w, h)
    key = (name, w, h)
    S_a, S_b = fast_sums(oracle, arrays, key, 4, 3).reshape(-1, 3), fast_sums(oracle, arrays, key, 8, 3).reshape(-1, 3)
    want, _ = guarded_rule(S_a, 4, S_b, 8, THRESHOLD)
    assert len(want) == count
    acc = scene.accumulator(fast=True, fast_chunk=3)
    acc.add(4)
    acc.mark()
    acc.add(4)
    lst, before = select(acc, 12, threshold=THRESHOLD)
    assert np.array_equal(lst, want)
    add_selected(acc, lst, before, 12)
    counts = np.full(w * h, 8, np.int32)
    counts[want] = 12
    check_invariant(acc, counts.reshape(h, w), lambda n: fast_sums(oracle, arrays, key, n, 3))
    acc.free()


def test_save_and_load_mid_chunk(gpu, oracle, tmp_path):
    scene, arrays = ref_scene(gpu, "cornell", 64, 64)
    key = ("cornell", 64, 64)
    path = str(tmp_path / "fast.acc")
    acc = scene.accumulator(fast=True, fast_chunk=3)
    acc.add(4)
    state, sums = acc.state(), acc.sums()
    assert state[:, 1:].any()   # (saved inside chunk 1)
    acc.save(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"RTFACCUM" and len(raw) == 128 + 32 * 64 * 64
    assert np.frombuffer(raw[8:12], "<u4")[0] == 1 and np.frombuffer(raw[120:128], "<i4").tolist() == [3, 0]
    acc.add(4)
    uninterrupted = acc.sums()
    acc.free()
    acc = gpu.Accumulator.load(scene, path)
    assert acc.fast_chunk == 3 and acc.samples == 4 and acc.sample_range == (4, 4)
    assert np.array_equal(acc.state(), state) and np.array_equal(rtref.bits(acc.sums()), rtref.bits(sums))
    stats = acc.add(4)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(uninterrupted))
    check_pass(gpu, oracle, acc, arrays, key, 8, 3, stats, 4)
    acc.free()
    # a fast file does not load into a scene it does not fit
    other, _ = ref_scene(gpu, "cornell", 33, 17)
    with pytest.raises(gpu.RtError, match="64 x 64"):
        gpu.Accumulator.load(other, path)


def test_save_and_load_with_unequal_counts(gpu, oracle, tmp_path):
    scene, arrays = ref_scene(gpu, "cornell", 64, 64)
    key = ("cornell", 64, 64)
    acc = scene.accumulator(fast=True, fast_chunk=3)
    counts, _ = run_subsets(gpu, oracle, acc, arrays, key, 3, 2, cornell_steps()[:2])
    assert set(np.unique(counts)) == {2, 5, 7}
    path = str(tmp_path / "mixed.acc")
    state, sums = acc.state(), acc.sums()
    acc.save(path)
    acc.free()
    hdr = np.fromfile(path, np.int32, 16)
    assert (hdr[14], hdr[15]) == (7, 1)   # samples done = the largest count; the count form
    acc = gpu.Accumulator.load(scene, path)
    assert acc.fast_chunk == 3 and acc.sample_range == (2, 7)
    assert np.array_equal(acc.counts(), counts) and np.array_equal(acc.state(), state)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(sums))
    with pytest.raises(gpu.RtError, match="level"):
        acc.add(1)
    lst, before = select(acc, 7)   # level
    add_selected(acc, lst, before, 7)
    assert acc.sample_range == (7, 7)
    assert np.array_equal(rtref.bits(acc.sums()), rtref.bits(fast_sums(oracle, arrays, key, 7, 3)))
    acc.free()


def test_frame_finish_by_count(gpu, oracle):
    scene, arrays = ref_scene(gpu, "cornell", 64, 64)
    key = ("cornell", 64, 64)
    acc = scene.accumulator(fast=True, fast_chunk=3)
    counts, _ = run_subsets(gpu, oracle, acc, arrays, key, 3, 2, cornell_steps()[:2])
    frame = acc.frame()
    assert np.array_equal(frame, gpu.tonemap_counts(acc.sums(), acc.counts()))
    for n in (2, 5, 7):
        assert np.array_equal(frame[counts == n], gpu.tonemap(fast_sums(oracle, arrays, key, n, 3), n)[counts == n])
    acc.free()


def test_render_adaptive_fast(gpu, oracle):
    scene, arrays = ref_scene(gpu, "cornell", 64, 64)
    sums, counts, frame = scene.render_adaptive(8, 16, 4, THRESHOLD, fast=True, fast_chunk=2)
    assert counts.min() == 8 and set(np.unique(counts).tolist()) <= {8, 12, 16}
    assert len(np.unique(counts)) > 1
    for n in np.unique(counts):
        at = counts == n
        want = fast_sums(oracle, arrays, ("cornell", 64, 64), int(n), 2)
        assert np.array_equal(rtref.bits(sums[at]), rtref.bits(want[at]))
    assert np.array_equal(frame, gpu.tonemap_counts(sums, counts))


# ---------------------------------------------------------------- CLI
def _cli(out, samples, ok=True, **env_add):
    env = dict(os.environ)
    for k in ("RT_PASS_SPP", "RT_CHECKPOINT", "RT_ADAPT", "RT_COUNTS_OUT", "RT_FAST"):
        env.pop(k, None)
    env["RT_GPUS"] = "1"
    env.update(env_add)
    r = subprocess.run([SOLUTION, rtref.scene_path("cornell"), "33", "17", str(samples), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def test_cli_fast(gpu, oracle, tmp_path):
    arrays = gpu.Scene.load(rtref.scene_path("cornell"), 33, 17, 3).view()   # (the CLI's own loader)
    ppm = lambda n: b"P6\n33 17\n255\n" + gpu.tonemap(fast_sums(oracle, arrays, "cli", n, 2), n).tobytes()
    out, cnt = str(tmp_path / "out.ppm"), str(tmp_path / "counts.pgm")
    stdout = _cli(out, 3, RT_FAST="2", RT_PASS_SPP="1")
    assert "Progress: 3 / 3 samples" in stdout
    assert open(out, "rb").read() == ppm(3)
    # RT_FAST alone: the one-shot fast frame (3 <= 128 x 2: the same sum)
    _cli(out, 3, RT_FAST="2")
    assert open(out, "rb").read() == ppm(3)
    # adaptive: threshold 0 raises every pixel every round
    _cli(out, 3, RT_FAST="2", RT_ADAPT="0", RT_PASS_SPP="1", RT_COUNTS_OUT=cnt)
    assert open(out, "rb").read() == ppm(3) and (_pgm(cnt, 33, 17) == 3).all()
    # a threshold nothing exceeds: the two first passes only
    stdout = _cli(out, 3, RT_FAST="2", RT_ADAPT="1e30", RT_PASS_SPP="1", RT_COUNTS_OUT=cnt)
    assert "refined" not in stdout and (_pgm(cnt, 33, 17) == 2).all()
    assert open(out, "rb").read() == ppm(2)
    # a checkpointed run resumes to identical bytes, and only into its own kind
    prefix = str(tmp_path / "ck")
    _cli(out, 2, RT_FAST="2", RT_PASS_SPP="1", RT_CHECKPOINT=prefix)
    assert open(prefix + ".0of1", "rb").read(8) == b"RTFACCUM"
    stdout = _cli(out, 3, RT_FAST="2", RT_PASS_SPP="1", RT_CHECKPOINT=prefix)
    assert "Resumed from" in stdout and "at 2 samples" in stdout
    assert open(out, "rb").read() == ppm(3)
    for other in (dict(), dict(RT_FAST="3")):
        stderr = _cli(out, 3, ok=False, RT_PASS_SPP="1", RT_CHECKPOINT=prefix, **other)
        assert "checkpoint" in stderr and "fast accumulator with chunks of 2" in stderr
